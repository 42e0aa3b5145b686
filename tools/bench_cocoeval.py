#!/usr/bin/env python
"""COCO AP matching + accumulation: the device engine (csrc/cocoeval.hip through evaluation/cocoeval_ops.py) against the host
engine it stands in for (evaluation/cocoeval.py's Python loops), alternated in the same run.  GPU only: fails without one.

The problem is seeded, synthetic and val-like: 80 categories, 100 detections and 7 annotations per image, 5 % crowd regions,
the detections of an image concentrated on three categories, scores in thousandths (ties).  One JSON line per size:
  device_ms      one `evaluate_bbox(engine="device")` call, host clock around it with a synchronise at the end: prepare, pack,
                 upload, kernels, fetch, summary; median / min / max over the repetitions after warm-up
  split_ms       medians of the parts of that call: prepare (the host's grouping, shared with the host engine), pack, upload
                 (staging + copy), kernel (device events around the launches), fetch
  host_ms        one `evaluate_bbox(engine="host")` call (the engine of the parent commit, unchanged)
  host_syncs, d2h_transfers, h2d_transfers   per device call, counted by cocoeval_ops where they happen
  workspace_bytes, upload_bytes              device memory of the call
    python tools/bench_cocoeval.py [--rounds 5] [--out profiles/cocoeval.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.evaluation import cocoeval as CE  # noqa: E402
from u2seg_amd.evaluation import cocoeval_ops as OPS  # noqa: E402

INFERENCE_S_5000 = 6.0  # 5 000 images at the README's 784-807 img/s


def val_like(images, seed=0, cats=80, dets=100, anns_per_image=7, crowd=0.05):
    rs = np.random.RandomState(seed)
    annotations, results = [], []
    for img in range(1, images + 1):
        own = rs.choice(cats, size=3, replace=False) + 1
        first = len(annotations)
        for _ in range(anns_per_image):
            w, h = rs.uniform(8, 300, size=2)
            x, y = rs.uniform(0, 640 - 8), rs.uniform(0, 480 - 8)
            cat = int(own[rs.randint(3)]) if rs.rand() < 0.7 else int(rs.randint(cats)) + 1
            annotations.append({"id": len(annotations) + 1, "image_id": img, "category_id": cat, "iscrowd": int(rs.rand() < crowd),
                                "bbox": [float(x), float(y), float(w), float(h)], "area": float(w * h)})
        for _ in range(dets):
            if rs.rand() < 0.5:  # near an annotation of the image
                a = annotations[int(rs.randint(first, len(annotations)))]
                box = (np.asarray(a["bbox"]) + rs.normal(0, 4, size=4)).clip(1, None)
                cat = a["category_id"] if a["category_id"] in own else int(own[rs.randint(3)])
            else:
                box = np.r_[rs.uniform(0, 600), rs.uniform(0, 440), rs.uniform(8, 300, size=2)]
                cat = int(own[rs.randint(3)])
            results.append({"image_id": img, "category_id": cat, "bbox": [float(v) for v in box],
                            "score": float(np.round(rs.rand(), 3))})
    dataset = {"images": [{"id": i} for i in range(1, images + 1)], "categories": [{"id": c} for c in range(1, cats + 1)],
               "annotations": annotations}
    return dataset, results


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def device_call(dataset, results):
    """One call of the device engine, timed in its parts (the same steps as evaluate_bbox(engine="device"))."""
    torch.cuda.synchronize()
    before = dict(OPS.counters)
    t0 = time.perf_counter()
    imgs = sorted(im["id"] for im in dataset["images"])
    cats = sorted(c["id"] for c in dataset["categories"])
    params = CE.Params(imgs, cats)
    gts, dts = CE.prepare(dataset["annotations"], results, params)
    t1 = time.perf_counter()
    packed = OPS.pack(gts, dts, params)
    t2 = time.perf_counter()
    acc = OPS.run(packed, timing=True)
    stats = dict(zip(CE.STAT_NAMES, CE.summarize(acc, params)))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    lt = dict(OPS.last_timing)
    parts = {"prepare": (t1 - t0) * 1e3, "pack": (t2 - t1) * 1e3, "upload": lt["upload_ms"], "kernel": lt["kernel_ms"],
             "fetch": lt["fetch_ms"], "total": (t3 - t0) * 1e3}
    counts = {k: OPS.counters[k] - before[k] for k in before}
    return acc, stats, parts, counts, lt, packed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed repetitions per size after one warm-up")
    ap.add_argument("--small", type=int, default=500, help="images of the size both engines are timed (and compared) at")
    ap.add_argument("--large", type=int, default=5000, help="images of the validation-set size")
    ap.add_argument("--host-large", type=int, default=1, help="host calls at the large size (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cocoeval.py needs a GPU: there is nothing to measure without one")
    lines = []
    for images in (args.small, args.large):
        dataset, results = val_like(images, seed=images)
        small = images == args.small
        device_call(dataset, results)  # warm-up: code objects, the allocator's blocks, pinned memory
        dev_ms, host_ms, parts, counts = [], [], [], []
        host = None
        host_rounds = args.rounds if small else args.host_large
        for r in range(args.rounds):  # alternating: device, host, device, ...
            acc, stats, pt, cn, lt, packed = device_call(dataset, results)
            t0 = time.perf_counter()
            full = CE.evaluate_bbox(dataset, results, engine="device")
            torch.cuda.synchronize()
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            parts.append(pt)
            counts.append(cn)
            if r < host_rounds:
                t0 = time.perf_counter()
                host = CE.evaluate_bbox(dataset, results)
                host_ms.append((time.perf_counter() - t0) * 1e3)
                print("# %d images: host call %d %.1f s, device call %.3f s" % (images, r, host_ms[-1] / 1e3, dev_ms[-1] / 1e3),
                      file=sys.stderr, flush=True)
        line = {"images": images, "categories": 80, "detections": len(results), "annotations": len(dataset["annotations"]),
                "cells": packed.n_cells, "iou_entries": packed.iou_entries, "device_ms": spread(dev_ms),
                "split_ms": {k: float(np.median([p[k] for p in parts])) for k in parts[0]},
                "host_syncs": sorted(set(c["host_syncs"] for c in counts)),
                "d2h_transfers": sorted(set(c["d2h_transfers"] for c in counts)),
                "h2d_transfers": sorted(set(c["h2d_transfers"] for c in counts)),
                "workspace_bytes": lt["workspace_bytes"], "upload_bytes": lt["upload_bytes"], "AP": stats["AP"]}
        if host is not None:
            equal = all(np.array_equal(host[k], full[k]) for k in ("precision", "recall", "scores")) and host["stats"] == full["stats"]
            assert equal, "the device engine's tables differ from the host engine's at %d images" % images
            line.update(host_ms=spread(host_ms), results_equal_host=True,
                        speedup_median=spread(host_ms)["median"] / spread(dev_ms)["median"])
        if not small:
            line["device_s_per_task"] = spread(dev_ms)["median"] / 1e3
            line["inference_s_same_images"] = INFERENCE_S_5000 * images / 5000
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
