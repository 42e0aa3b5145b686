"""Per-layer cost of the residual tails' backward reduce folded into the next conv1 data gradient (u2_conv_dgrad_tail) against
the two launches it replaces (u2_conv_igemm + u2_norm_bwd_reduce), at the three production shapes of the training step
(batch 16, 800 x 1344 canvas).  Both forms alternate in one process; device events go round `--launches` back-to-back launches
and the medians over `--reps` such groups are reported per launch.  Writes profiles/tail_bwd_fuse.json.

    python tools/bench_tail_bwd.py [--launches 20] [--reps 9] [--out profiles/tail_bwd_fuse.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from u2seg_amd import _hip  # noqa: E402

SHAPES = [("res2", 1075200, 64, 256), ("res3", 268800, 128, 512), ("res4", 67200, 256, 1024)]
FORCED = 1 << 17   # lift the launchers' size rules (among them the one that keeps a shape on two launches): both forms are timed
BF16 = torch.bfloat16


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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tail_bwd_fuse.json"))
    args = ap.parse_args()
    dev = "cuda:0"
    _hip.load()
    g = torch.Generator(device=dev).manual_seed(0)
    result = {"launches_per_group": args.launches, "groups": args.reps, "unit": "us per launch (median of the groups)",
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, m, c, n in SHAPES:
        y = torch.randn((m, n), generator=g, device=dev, dtype=BF16)
        res = torch.randn((m, n), generator=g, device=dev, dtype=BF16)
        g2 = torch.randn((m, n), generator=g, device=dev, dtype=BF16)
        dy = torch.randn((m, c), generator=g, device=dev, dtype=BF16)
        wt = (0.1 * torch.randn((n, c), generator=g, device=dev)).to(BF16)
        stats = torch.stack([y.float().sum(0), (y.float() ** 2).sum(0)]).contiguous()
        gamma, beta = torch.ones(n, device=dev), torch.zeros(n, device=dev)
        rm, rv = torch.zeros(n, device=dev), torch.ones(n, device=dev)
        mean, invstd, scale, shift = (torch.empty(n, device=dev) for _ in range(4))
        out = torch.empty_like(y)
        bits = torch.empty((m, n // 8), dtype=torch.uint8, device=dev)
        _hip.call("u2_bn_act_fused", y, stats, float(m), None, gamma, beta, rm, rv, 0.1, 1e-5, mean, invstd, scale, shift, res, out,
                  m, n, n, 1, bits)
        del out, res
        g1, dz = torch.empty_like(y), torch.empty_like(y)
        sums = torch.zeros((2, n), device=dev)

        def conv():
            _hip.call("u2_conv_igemm", dy, wt, g1, None, None, 1, 1, m, c, c, 1, m, n, n, 1, 1, 0, 0, 1, 1, 0, 0, FORCED)

        def reduce():
            _hip.call("u2_norm_bwd_reduce", g1, bits, y, mean, invstd, sums, 1, m, n, n, 1, None, None, g2, dz, None, 1)

        def two():
            conv()
            reduce()

        def fused():
            rc = _hip.call_status("u2_conv_dgrad_tail", dy, wt, g2, y, bits, mean, invstd, dz, sums, 1, 1, m, c, c, n, n, FORCED)
            assert rc == 0, "u2_conv_dgrad_tail declined " + name

        served_by_default = _hip.call_status("u2_conv_dgrad_tail", dy, wt, g2, y, bits, mean, invstd, dz, sums, 1, 1, m, c, c, n, n,
                                             0) == 0
        conv_kernel = None
        for fn in (two, fused):   # warm-up
            fn()
            if fn is two:
                conv()
                conv_kernel = _hip.call_nostream("u2_conv_last_kernel")
        torch.cuda.synchronize()
        t = {"two": [], "fused": [], "conv": [], "reduce": []}
        for _ in range(args.reps):
            t["two"].append(timed(two, args.launches))
            t["fused"].append(timed(fused, args.launches))
            t["conv"].append(timed(conv, args.launches))
            t["reduce"].append(timed(reduce, args.launches))
        med = {k: statistics.median(v) for k, v in t.items()}
        tb = m * n * 2
        row = {"M": m, "C": c, "N": n, "conv_kernel_code": conv_kernel,
               "two_launches_us": round(med["two"], 1), "fused_us": round(med["fused"], 1),
               "conv_alone_us": round(med["conv"], 1), "reduce_alone_us": round(med["reduce"], 1),
               "two_launches_us_range": [round(min(t["two"]), 1), round(max(t["two"]), 1)],
               "fused_us_range": [round(min(t["fused"]), 1), round(max(t["fused"]), 1)],
               "fused_tb_per_s": round((3 * tb + tb / 16 + m * c * 2) / med["fused"] / 1e6, 2),
               "fused_faster": bool(max(t["fused"]) < min(t["two"])),
               "launcher_takes_fused_form": bool(served_by_default)}
        result["shapes"][name] = row
        print(name, json.dumps(row))
        del y, g2, dy, g1, dz, bits
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
