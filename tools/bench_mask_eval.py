#!/usr/bin/env python
"""Mask evaluation per image: the device path (csrc/maskeval.hip through evaluation/mask_ops.mask_batch: run-length strings
+ pair counts of a batch in two synchronisations) against the host path it replaces (pred_masks.cpu(), data/rle.py's encode
per mask, numpy intersections), alternated in the same run.  GPU only: fails without a device.

Input: masks written by the paste kernel from seeded probabilities and boxes, 100 instances per image, a batch of 8 images,
8 ground-truth blob masks per image, at 480 x 640 and 800 x 1333.  One JSON line per size:
  device_ms     per image, device events around the whole call (both synchronisations and the host work between them included),
                median / min / max over the repetitions after warm-up
  call_wall_ms  per image, host clock around the same call (adds the decoding of the fetched buffer into Python strings)
  bytes         what the algorithm has to move per batch: the canvases read once + the planes written once
  hbm_share     bytes / device time over the 8 TB/s HBM peak DESIGN.md section 5 uses
  host_ms       per image, the host path, on `--host-images` images of the batch per round
  host_syncs, d2h_transfers  per device call, counted by mask_ops where they happen
    python tools/bench_mask_eval.py [--rounds 5] [--out profiles/mask_eval.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.data import rle  # noqa: E402
from u2seg_amd.evaluation import mask_ops  # noqa: E402
from u2seg_amd.modeling.inference import paste_masks_in_images  # noqa: E402

HBM_PEAK = 8.0e12
DEV = "cuda:0"


def seeded_batch(h, w, images, n, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    probs, boxes = [], []
    for _ in range(images):
        c = torch.rand(n, 2, 2, generator=g) * 20 + 4
        s = torch.rand(n, 2, generator=g) * 6 + 3
        p = torch.zeros(n, 28, 28)
        for b in range(2):
            p = torch.maximum(p, torch.exp(-((xx[None] - c[:, b, 0, None, None]) ** 2 + (yy[None] - c[:, b, 1, None, None]) ** 2)
                                           / (2 * s[:, b, None, None] ** 2)))
        p = (p + 0.15 * torch.rand(n, 28, 28, generator=g)).clamp(0, 1)
        bw, bh = torch.rand(n, generator=g) * w * 0.5 + 8, torch.rand(n, generator=g) * h * 0.5 + 8
        x0, y0 = torch.rand(n, generator=g) * (w - 4) - 2, torch.rand(n, generator=g) * (h - 4) - 2
        probs.append(p.to(DEV))
        boxes.append(torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1).to(DEV))
    return paste_masks_in_images(probs, boxes, [(h, w)] * images, 0.5)


def gt_blobs(rs, n, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), dtype=bool)
    for k in range(n):
        for _ in range(rs.randint(1, 4)):
            cx, cy, rx, ry = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(8, w / 3), rs.uniform(8, h / 3)
            out[k] |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1
    return out


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (2 device calls, 1 host pass); >= 5")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--instances", type=int, default=100)
    ap.add_argument("--gt", type=int, default=8)
    ap.add_argument("--host-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_eval.py needs a GPU: there is nothing to measure without one")
    assert args.rounds >= 5, "at least 10 device samples"
    lines = []
    for h, w in ((480, 640), (800, 1333)):
        masks = seeded_batch(h, w, args.images, args.instances, seed=h)
        rs = np.random.RandomState(w)
        counts = [[rle.counts_of(rle.encode(m)) for m in gt_blobs(rs, args.gt, h, w)] for _ in range(args.images)]
        torch.cuda.synchronize()
        for _ in range(2):  # warm-up: code objects, the allocator's blocks
            dev_out = mask_ops.mask_batch(masks, counts)
        dev_ms, wall_ms, host_ms, syncs = [], [], [], []
        host_out = {}
        for r in range(args.rounds):
            for _ in range(2):
                before = dict(mask_ops.counters)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                dev_out = mask_ops.mask_batch(masks, counts)
                e1.record()
                torch.cuda.synchronize()
                wall_ms.append((time.perf_counter() - t0) * 1e3 / args.images)
                dev_ms.append(e0.elapsed_time(e1) / args.images)
                syncs.append((mask_ops.counters["host_syncs"] - before["host_syncs"],
                              mask_ops.counters["d2h_transfers"] - before["d2h_transfers"]))
            for k in range(args.host_images):  # the parent's path, image by image
                i = (r * args.host_images + k) % args.images
                t0 = time.perf_counter()
                m = masks[i].cpu().numpy()
                host_out[i] = mask_ops._host_image(m, counts[i], h, w)
                host_ms.append((time.perf_counter() - t0) * 1e3)
        for i, ho in host_out.items():  # same answers, at the size that is timed
            assert ho["rles"] == dev_out[i]["rles"] and np.array_equal(ho["inter"], dev_out[i]["inter"]), i
        n = args.images * args.instances
        nbytes = n * h * w + n * w * mask_ops.words_per_column(h) * 8
        d = spread(dev_ms)
        runs = float(np.mean([len(rle.counts_of(x)) for o in dev_out for x in o["rles"]]))
        lines.append({"size": [h, w], "images": args.images, "instances": args.instances, "gt_per_image": args.gt,
                      "mean_runs_per_mask": runs, "device_ms": d, "call_wall_ms": spread(wall_ms), "host_ms": spread(host_ms),
                      "bytes": nbytes, "hbm_share": nbytes / (d["median"] * args.images * 1e-3) / HBM_PEAK,
                      "speedup_median": spread(host_ms)["median"] / d["median"],
                      "host_syncs": sorted(set(s[0] for s in syncs)), "d2h_transfers": sorted(set(s[1] for s in syncs)),
                      "results_equal_host": True})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
