#!/usr/bin/env python
"""Time of USL's regularised selection (u2seg_amd/cluster/select.py, usl.hip) at the stage-1 size on cuda:0: N = 1 000 000
clustered unit rows of D = 768, S representatives (one per cluster, S clusters), H = 32.

For each S (default 300 and 800), one JSON line:
  reg_ms               selection_regularizer alone (select + refine kernels and the wrapper), median of --runs device-event
                       timings after --warmup
  reg_tflops           2 N S D / reg_ms, and its share of the 157.3 TF fp32 matrix peak
  selection_ms         get_selection_with_reg_imagenet(iters 2, K = S, w 0.05, momentum 0, exclude True), median of 3
  torch_reg_ms         the same regularizer in plain fp32 torch (cdist in GEMM form + topk + the same mask / sum / blend)
  torch_loop_ms        the reference's per-cluster selection loop (one torch.where / argmax / item per cluster) in torch
usage: python tools/bench_usl_select.py [--sizes 300,800] [--runs 10] [--warmup 2] [--no-torch]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from u2seg_amd import _hip  # noqa: E402
from u2seg_amd.cluster.select import get_selection_with_reg_imagenet, selection_regularizer  # noqa: E402

PEAK_TFLOPS = 157.3
N, D, H, W = 1_000_000, 768, 32, 0.05


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    return statistics.median(event_ms(fn) for _ in range(runs))


def make_data(s, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    centers = torch.randn(s, D, device="cuda", generator=g)
    x = torch.empty(N, D, device="cuda")
    labels = torch.empty(N, dtype=torch.long, device="cuda")
    for i0 in range(0, N, 131072):
        n = min(131072, N - i0)
        lab = torch.randint(0, s, (n,), device="cuda", generator=g)
        if i0 == 0:
            lab[:s] = torch.arange(s, device="cuda")  # every cluster has a member
        x[i0:i0 + n] = torch.nn.functional.normalize(centers[lab] + 0.6 * torch.randn(n, D, device="cuda", generator=g), dim=1)
        labels[i0:i0 + n] = lab
    nd = 0.5 + torch.rand(N, device="cuda", generator=g)
    return x, labels, nd


def torch_regularizer(x, y, labels, reg, h, momentum=0.0, chunk=65536):
    """fp32 torch: cdist (GEMM form) + topk + the reference's same-cluster mask, power sum and blend."""
    out = torch.empty_like(reg)
    for i0 in range(0, x.shape[0], chunk):
        d = torch.cdist(x[i0:i0 + chunk], y, compute_mode="use_mm_for_euclid_dist") ** 2
        v, j = torch.topk(d, h, dim=1, largest=False, sorted=True)
        m = (j == labels[i0:i0 + chunk].view(-1, 1)).float()
        v = (1 - m) * v + m * 1e10
        out[i0:i0 + chunk] = reg[i0:i0 + chunk] * momentum + (1 / v).sum(1) * (1 - momentum)
    return out


def torch_loop(nd, reg, labels, k):
    picks = []
    for c in range(k):
        match = torch.where(labels == c)[0]
        if len(match) == 0:
            continue
        picks.append(match[(1 / nd[match] - W * reg[match]).argmax()].item())
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,800")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    _hip.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    for s in [int(v) for v in args.sizes.split(",")]:
        x, labels, nd = make_data(s)
        sel = torch.from_numpy(get_selection_with_reg_imagenet(x, nd, labels, s, iters=1, final_sample_num=s, w=W,
                                                               horizon_num=H, exclude_same_cluster=True)).cuda()
        y = x[sel]
        reg0 = torch.zeros(N, device="cuda")
        reg_ms = median_ms(lambda: selection_regularizer(x, y, labels, reg0, H, momentum=0.0, exclude_same_cluster=True),
                           args.runs, args.warmup)
        sel_ms = median_ms(lambda: get_selection_with_reg_imagenet(x, nd, labels, s, iters=2, final_sample_num=s, w=W,
                                                                   momentum=0.0, horizon_num=H, alpha=1.0,
                                                                   exclude_same_cluster=True), 3, 1)
        tflops = 2.0 * N * s * D / (reg_ms * 1e-3) / 1e12
        res = {"N": N, "S": s, "D": D, "H": H, "runs": args.runs, "reg_ms": round(reg_ms, 3), "reg_tflops": round(tflops, 1),
               "reg_peak_frac": round(tflops / PEAK_TFLOPS, 3), "selection_ms": round(sel_ms, 2)}
        if not args.no_torch:
            res["torch_reg_ms"] = round(median_ms(lambda: torch_regularizer(x, y, labels, reg0, H), 3, 1), 2)
            res["torch_loop_ms"] = round(median_ms(lambda: torch_loop(nd, reg0, labels, s), 3, 1), 2)
        print(json.dumps(res), flush=True)
        del x, labels, nd, y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
