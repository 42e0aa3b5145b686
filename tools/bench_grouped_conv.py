#!/usr/bin/env python
"""The grouped 3x3 kernels against the dense kernels at the same width.  GPU only: fails without a device.

The conv2 shapes of X-101-32x8d at 16 x 800 x 1333 (padded to 800 x 1344; STRIDE_IN_1X1 False, so the first block of res3-res5
carries the stride in conv2): res2 256 channels (cg = 8) on the stride-4 map, res3 512 (16), res4 1024 (32), res5 2048 (64), the
last three with their stride-2 twin.  Per shape and pass:

  grouped    u2_gconv3x3_fwd / _dgrad / _wgrad (conv_grouped.hip) on the fp32 parameter
  dense      the yardstick: u2_conv_igemm (forward, data gradient) and u2_conv_wgrad with variant 0 on the SAME activations and a
             dense filter of the same width in its kernel layouts (built outside the timed window)

Device-event time per call, median / min / max over the repetitions (each a window of at least --window-ms of back-to-back calls
between two events, grouped and dense alternating, every form warmed up first; the buffers are reused call after call, so at res4
and res5, whose maps fit the 256 MB last-level cache, the rate below is bytes delivered, not an HBM rate), the bytes the grouped pass has to move (activations read and written once, the
fp32 filter once) over its median time, that rate over the 8.0 TB/s HBM peak, and its MACs (useful: 9 cg per output, issued: 9 S
with S = max(cg, 32)).  condition: grouped median <= dense median, per shape and pass; "all_hold" says whether every one does.

--train N adds a short training run of configs/COCO-PanopticSegmentation/u2seg_X101_32x8d_800.yaml on synthetic 800 x 1333 batches
(the largest of --train-batches that fits): ms per step over N steps after 3 warm-up steps (host clock around a synchronise), and
the grouped kernels' share of the device's kernel time in one further step under torch.profiler (a run of its own).

    python tools/bench_grouped_conv.py [--window-ms 250] [--reps 7] [--batch 16] [--train 10] [--out profiles/grouped_conv.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
BF16 = torch.bfloat16
HBM_PEAK = 8.0e12
# (stage, channels, cg, input map (h, w) at batch 1, stride)
SHAPES = [("res2", 256, 8, (200, 336), 1),
          ("res3", 512, 16, (100, 168), 1), ("res3 stride 2", 512, 16, (200, 336), 2),
          ("res4", 1024, 32, (50, 84), 1), ("res4 stride 2", 1024, 32, (100, 168), 2),
          ("res5", 2048, 64, (25, 42), 1), ("res5 stride 2", 2048, 64, (50, 84), 2)]


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "each_ms": [round(x, 5) for x in v]}


def _window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / calls


def time_pair(forms, window_ms, reps):
    """Each form: 3 warm-up calls, 5 calls to size its window (at least `window_ms` of back-to-back calls), then `reps` windows,
    the forms alternating."""
    calls = {}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(20, int(window_ms / _window(fn, 5)) + 1)
    out = {k: [] for k in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            out[name].append(_window(fn, calls[name]))
    return {k: dict(summary(v), calls_per_window=calls[k]) for k, v in out.items()}


def bench_shape(stage, c, cg, hw, stride, batch, window_ms, reps):
    from u2seg_amd.layers import conv_launch
    from u2seg_amd.layers import functional as F

    groups = c // cg
    h, w = hw
    g = torch.Generator(device=DEV).manual_seed(c + stride)
    x = torch.relu(torch.randn((batch, h, w, c), generator=g, device=DEV)).to(BF16)
    gg = conv_launch.GroupedGeom.of(x.shape, (c, cg, 3, 3), groups, stride, 1)
    dz = (torch.randn((batch, gg.ho, gg.wo, c), generator=g, device=DEV) * 2.0 ** -10).to(BF16)
    wg = torch.randn((c, cg, 3, 3), generator=g, device=DEV) / (9 * cg) ** 0.5
    wdense = torch.randn((c, c, 3, 3), generator=g, device=DEV) / (9 * c) ** 0.5
    dg = conv_launch.ConvGeom.of(x.shape, wdense.shape, stride, 1)
    with torch.no_grad():
        wk = F.weight_fwd_layout(wdense, c)
        wd = F.weight_dgrad_layout(wdense, c, c)
    del wdense
    out, dx = torch.empty_like(dz), torch.empty_like(x)
    stats = torch.zeros((2, c), dtype=torch.float32, device=DEV)
    dw = torch.zeros((c, cg, 3, 3), dtype=torch.float32, device=DEV)
    dwk = torch.zeros((c, 9, c), dtype=torch.float32, device=DEV)
    act_in, act_out = x.numel() * 2, dz.numel() * 2
    wbytes = wg.numel() * 4
    s = max(cg, 32)
    passes = {
        "forward": ({"grouped": lambda: conv_launch.grouped_forward(gg, x, wg, None, None, out, stats, False),
                     "dense": lambda: conv_launch.forward(dg, x, wk, out, None, stats, False, 0, 0)}, act_in + act_out + wbytes),
        "dgrad": ({"grouped": lambda: conv_launch.grouped_dgrad(gg, dz, wg, None, dx),
                   "dense": lambda: conv_launch.dgrad(dg, dz, wd, dx, 0)}, act_in + act_out + wbytes),
        "wgrad": ({"grouped": lambda: conv_launch.grouped_wgrad(gg, x, dz, None, dw),
                   "dense": lambda: conv_launch.wgrad_scratch(dg, x, dz, dwk)}, act_in + act_out + wbytes),
    }
    rec = {"stage": stage, "channels": c, "cg": cg, "groups": groups, "batch": batch, "in_hw": [h, w], "out_hw": [gg.ho, gg.wo],
           "stride": stride, "useful_macs": gg.m_out * c * 9 * cg, "issued_macs": gg.m_out * c * 9 * s, "dense_macs": gg.m_out * c * 9 * c,
           "passes": {}}
    for name, (forms, nbytes) in passes.items():
        t = time_pair(forms, window_ms, reps)
        med = t["grouped"]["median_ms"] * 1e-3
        rec["passes"][name] = {"grouped": t["grouped"], "dense": t["dense"], "bytes": nbytes, "grouped_bytes_per_s": nbytes / med,
                               "grouped_share_of_hbm_peak": nbytes / med / HBM_PEAK,
                               "condition_holds": t["grouped"]["median_ms"] <= t["dense"]["median_ms"]}
        print("%-14s %-8s grouped %8.3f ms  dense %8.3f ms  %6.2f TB/s  %s" % (
            stage, name, t["grouped"]["median_ms"], t["dense"]["median_ms"], nbytes / med / 1e12,
            "ok" if rec["passes"][name]["condition_holds"] else "SLOWER THAN DENSE"), flush=True)
    return rec


def bench_training(steps, batches):
    import time

    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.engine import SimpleTrainer
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_optimizer

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_X101_32x8d_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV])
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    trainer = SimpleTrainer(model, build_optimizer(cfg, model))
    tried = []
    for b in batches:
        try:
            batch = make_synthetic_batch(b, height=800, width=1333, device=DEV)
            for _ in range(3):
                trainer.run_step(batch)
            torch.cuda.synchronize()
        except torch.OutOfMemoryError:
            tried.append(b)
            torch.cuda.empty_cache()
            continue
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.run_step(batch)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        trainer.check_finite()
        rec = {"config": "u2seg_X101_32x8d_800.yaml", "batch": b, "batches_that_did_not_fit": tried, "steps": steps,
               "ms_per_step": ms, "img_per_s": b / ms * 1e3, "peak_memory_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
               "grouped_kernel_share": None}
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                trainer.run_step(batch)
                torch.cuda.synchronize()
            dev = [e for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA]
            total = sum(e.device_time for e in dev)
            grouped = sum(e.device_time for e in dev if "gconv_kernel" in e.name or "gwgrad_kernel" in e.name)
            rec.update(grouped_kernel_share=grouped / total, grouped_kernel_ms=grouped * 1e-3, kernel_ms=total * 1e-3)
        except Exception as e:  # the share is an extra
            print("kernel share not available: %s" % e, file=sys.stderr)
        print("training: %s" % rec, flush=True)
        return rec
    raise RuntimeError("no batch of %s fits" % (batches,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=250.0, help="least length of one timed window of back-to-back calls")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--train", type=int, default=0, help="steps of the X-101-32x8d training run (0: none)")
    ap.add_argument("--train-batches", type=int, nargs="+", default=[16, 8, 4, 2])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_conv.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from u2seg_amd import _hip

    _hip.load()
    shapes = [bench_shape(*sh, a.batch, a.window_ms, a.reps) for sh in SHAPES]
    res = {"device": torch.cuda.get_device_name(0), "window_ms": a.window_ms, "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around windows of at least window_ms of back-to-back launches, grouped and dense alternating, "
                     "3 warm-up calls each",
           "note": "the same buffers are reused call after call: where input + output stay below the 256 MB of the last-level cache "
                   "(res4, res5) the bytes per second are a rate of bytes delivered, not an HBM rate",
           "shapes": shapes, "all_hold": all(p["condition_holds"] for sh in shapes for p in sh["passes"].values())}
    if a.train:
        res["training"] = bench_training(a.train, a.train_batches)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("all_hold: %s -> %s" % (res["all_hold"], a.out))


if __name__ == "__main__":
    main()
