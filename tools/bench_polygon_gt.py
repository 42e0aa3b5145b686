#!/usr/bin/env python
"""Polygon ground truth per image: the device route (csrc/polygon.hip through evaluation/mask_ops.planes_from_annotations:
the annotations of a batch become bit planes on the device) against the host definition (data/polygon.py, what the host route
of the evaluator runs per annotation), alternated in the same run.  GPU only: fails without a device.

Input: seeded star-shaped blobs of 20-200 vertices, 1-3 polygons per annotation, plus one crowd region as uncompressed RLE per
image; a batch of 8 images with 8 annotations at 480 x 640 and with 20 at 800 x 1333.  One JSON line per size:
  device_wall_ms  per image, host clock around planes_from_annotations + a synchronisation: parsing and checking the
                  annotations, the uploads, the launches and the kernels; median / min / max of 10 samples after 2 warm-ups
  device_ms       per image, device events around the same call
  host_ms         per image, the host definition (mask_ops.gt_mask of every annotation of an image)
  host_syncs, d2h_transfers  of one mask_batch call with this ground truth (8 detections per image) next to the same call with
                  the ground truth given as RLE counts
    python tools/bench_polygon_gt.py [--out profiles/polygon_gt.json]"""
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

DEV = "cuda:0"


def blob(rs, h, w, vertices):
    cx, cy = rs.uniform(0.1 * w, 0.9 * w), rs.uniform(0.1 * h, 0.9 * h)
    rx, ry = rs.uniform(0.05 * w, 0.4 * w), rs.uniform(0.05 * h, 0.4 * h)
    ang = np.sort(rs.uniform(0, 2 * np.pi, vertices))
    rad = rs.uniform(0.6, 1.0, vertices)
    return np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], axis=1).reshape(-1).tolist()


def annotations(rs, h, w, n):
    anns = [{"id": k, "iscrowd": 0, "segmentation": [blob(rs, h, w, rs.randint(20, 201)) for _ in range(rs.randint(1, 4))]}
            for k in range(n)]
    yy, xx = np.mgrid[0:h, 0:w]
    crowd = ((xx - 0.5 * w) / (0.3 * w)) ** 2 + ((yy - 0.6 * h) / (0.2 * h)) ** 2 <= 1
    anns.insert(n // 2, {"id": n, "iscrowd": 1, "segmentation": {"size": [h, w], "counts": rle.counts_of(rle.encode(crowd))}})
    return anns


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def budget(fn):
    before = dict(mask_ops.counters)
    out = fn()
    return out, {k: mask_ops.counters[k] - before[k] for k in before}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polygon_gt.py needs a GPU: there is nothing to measure without one")
    dev = torch.device(DEV)
    lines = []
    for (h, w), n in (((480, 640), 8), ((800, 1333), 20)):
        rs = np.random.RandomState(h)
        batch = [annotations(rs, h, w, n) for _ in range(args.images)]
        sizes = [(h, w)] * args.images
        wall_ms, dev_ms, host_ms = [], [], []
        host_masks = {}
        for s in range(-2, args.samples):  # two warm-ups, then the routes alternate
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            planes, descs, info = mask_ops.planes_from_annotations(batch, sizes, dev)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            i = s % args.images
            host_masks[i] = [mask_ops.gt_mask(a, h, w) for a in batch[i]]
            t2 = time.perf_counter()
            if s >= 0:
                wall_ms.append((t1 - t0) * 1e3 / args.images)
                dev_ms.append(e0.elapsed_time(e1) / args.images)
                host_ms.append((t2 - t1) * 1e3)
        host_planes = planes.cpu().numpy()
        nw = w * mask_ops.words_per_column(h)
        for i, masks in host_masks.items():  # same answers, at the size that is timed
            d = descs[i]
            got, padding = mask_ops.unpack_planes(host_planes[d.plane_offset : d.plane_offset + d.n * nw], d.n, h, w)
            assert not padding.any()
            for j, k in enumerate(info["order"][i]):
                assert np.array_equal(got[j], masks[k]), (i, k)
        dets = [torch.from_numpy(np.random.RandomState(i).rand(8, h, w) < 0.5).to(dev) for i in range(args.images)]
        out, used = budget(lambda: mask_ops.mask_batch(dets, gt=batch))
        counts = [[rle.counts_of(rle.encode(mask_ops.gt_mask(a, h, w))) for a in anns] for anns in batch]
        ref, used_rle = budget(lambda: mask_ops.mask_batch(dets, counts))
        assert all(np.array_equal(a["inter"], b["inter"]) for a, b in zip(out, ref))
        polys = [p for anns in batch for a in anns if isinstance(a["segmentation"], list) for p in a["segmentation"]]
        lines.append({"size": [h, w], "images": args.images, "annotations_per_image": n + 1, "polygons_per_image": len(polys) / args.images,
                      "mean_vertices": float(np.mean([len(p) // 2 for p in polys])),
                      "device_wall_ms": spread(wall_ms), "device_ms": spread(dev_ms), "host_ms": spread(host_ms),
                      "host_over_device_wall_median": spread(host_ms)["median"] / spread(wall_ms)["median"],
                      "mask_batch_budget": used, "mask_batch_budget_rle_only": used_rle, "results_equal_host": True})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
