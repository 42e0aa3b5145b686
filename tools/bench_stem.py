"""Per-launch cost of the stem convolution and its weight gradient straight from the images (u2_stem_conv_fwd +
u2_stem_conv_wgrad) against the three launches they replace (u2_stem_im2col_batch + u2_conv_igemm + u2_conv_wgrad), at the
benchmark shape of the training step (batch 16 of 3 x 800 x 1333 uint8 images on the 800 x 1344 canvas, 4 300 800 output pixels).
Both forms alternate in one process; device events go round `--launches` back-to-back launches and the medians over `--reps`
such groups are reported per launch.  Writes profiles/stem_direct.json.

    python tools/bench_stem.py [--batch 16] [--launches 20] [--reps 9] [--out profiles/stem_direct.json]

Byte floors (what each direct launch has to move, at the 5.5 TB/s the streaming kernels sustain): the forward writes the
[M][64] bf16 output and reads the images, the weight gradient reads the same number of gradient bytes and the images.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2seg_amd import _hip  # noqa: E402

BF16 = torch.bfloat16
N, KP = 64, 160
SUSTAINED_TB_S = 5.5


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stem_direct.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    _hip.load()
    g = torch.Generator(device=dev).manual_seed(0)
    b, h, w = args.batch, args.height, args.width
    hpad, wpad = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    ho, wo = (hpad + 6 - 7) // 2 + 1, (wpad + 6 - 7) // 2 + 1
    m = b * ho * wo
    images = [torch.randint(0, 256, (3, h, w), generator=g, device=dev, dtype=torch.uint8) for _ in range(b)]
    ptrs = (ctypes.c_void_p * b)(*[im.data_ptr() for im in images])
    hs, ws = (ctypes.c_int * b)(*[h] * b), (ctypes.c_int * b)(*[w] * b)
    mean = torch.tensor([123.675, 116.28, 103.53], device=dev)
    std = torch.tensor([58.395, 57.12, 57.375], device=dev)
    wk = torch.zeros((N, 1, KP), dtype=BF16, device=dev)
    wk[:, 0, :147] = (0.05 * torch.randn((N, 147), generator=g, device=dev)).to(BF16)
    dy = (torch.randn((m, N), generator=g, device=dev) * 2.0 ** -6).to(BF16)
    out = torch.empty((m, N), dtype=BF16, device=dev)
    stats = torch.zeros((2, N), device=dev)
    dw = torch.zeros((N, 1, KP), device=dev)
    col = torch.empty((m, KP), dtype=BF16, device=dev)

    def im2col():
        _hip.call("u2_stem_im2col_batch", ptrs, hs, ws, b, 1, mean, std, col, hpad, wpad, KP)

    def gemm():
        _hip.call("u2_conv_igemm", col, wk, out, None, stats, 1, m, 1, KP, KP, m, 1, N, N, 1, 1, 0, 0, 1, 1, 0, 0, 0)

    def wgrad():
        _hip.call("u2_conv_wgrad", col, dy, dw, 1, m, 1, KP, KP, m, 1, N, N, 1, 1, 0, 0, 1, 0)

    def fwd():
        assert _hip.call_status("u2_stem_conv_fwd", ptrs, hs, ws, b, 1, mean, std, wk, out, stats, hpad, wpad, N, KP) == 0

    def dwd():
        assert _hip.call_status("u2_stem_conv_wgrad", ptrs, hs, ws, b, 1, mean, std, dy, dw, hpad, wpad, N, KP) == 0

    def old():
        im2col()
        gemm()
        wgrad()

    def new():
        fwd()
        dwd()

    for fn in (old, new):   # warm-up
        fn()
    torch.cuda.synchronize()
    parts = {"old": old, "new": new, "im2col": im2col, "gemm": gemm, "wgrad": wgrad, "direct_fwd": fwd, "direct_wgrad": dwd}
    t = {k: [] for k in parts}
    for _ in range(args.reps):
        for k, fn in parts.items():
            t[k].append(timed(fn, args.launches))
    med = {k: statistics.median(v) for k, v in t.items()}
    img_bytes = sum(im.numel() for im in images)
    floor_us = (m * N * 2 + img_bytes) / SUSTAINED_TB_S / 1e6
    result = {"launches_per_group": args.launches, "groups": args.reps, "unit": "us per call (median of the groups)",
              "device": torch.cuda.get_device_name(0), "batch": b, "canvas": [hpad, wpad], "M": m,
              "old_im2col_gemm_wgrad_us": round(med["old"], 1), "new_fwd_wgrad_us": round(med["new"], 1),
              "old_us_per_group": [round(v, 1) for v in t["old"]], "new_us_per_group": [round(v, 1) for v in t["new"]],
              "new_lower_in_every_group": bool(all(n < o for n, o in zip(t["new"], t["old"]))),
              "alone_us": {k: round(med[k], 1) for k in ("im2col", "gemm", "wgrad", "direct_fwd", "direct_wgrad")},
              "byte_floor_us_each": round(floor_us, 1),
              "direct_fwd_tb_per_s": round((m * N * 2 + img_bytes) / med["direct_fwd"] / 1e6, 2),
              "direct_wgrad_tb_per_s": round((m * N * 2 + img_bytes) / med["direct_wgrad"] / 1e6, 2),
              "matrix_bytes": m * KP * 2}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
