#!/usr/bin/env python
"""Panoptic quality per image: the device path (csrc/panopticeval.hip through evaluation/panoptic_ops.pair_counts_batch, then
pq.accumulate_counts on the fetched table) against the path it stands in for (pq.accumulate_image on the two id maps: three
np.unique sorts per image), alternated in the same run.  GPU only: fails without a device.

Input: id maps produced by the real merge (combine_semantic_and_instance_outputs_batch) on seeded pasted masks and a blocky
semantic map; ground truth of seeded blobs with 24-bit ids, one of them not in segments_info; batches of 8 and 32 images at
480 x 640 and 800 x 1333.  One JSON line per (size, batch):
  device_ms      per image, device events around the whole pair_counts_batch call (staging, upload, launch, fetch and the
                 host work between them included), median / min / max over the repetitions after warm-up
  call_wall_ms   per image, host clock around the same call
  kernel_ms      per image, device events around the launcher alone (clear + count kernels) on a batch already uploaded
  finish_ms      per image, pq.accumulate_counts on the fetched table
  device_total_ms  device_ms + finish_ms (medians): what stands against image_ms
  image_ms       per image, pq.accumulate_image on the same arrays (already on the host, ids already formed)
  png_ms         per image, what the file route adds: PNG-encoding the predicted map and decoding it and the ground truth
  bytes          what the kernel has to read per batch: 7 bytes per pixel
  kernel_hbm_share  bytes / kernel time over the 8 TB/s HBM peak DESIGN.md section 5 uses
  host_syncs, d2h_transfers, h2d_transfers  per device call, counted by panoptic_ops where they happen
    python tools/bench_panoptic_pq.py [--rounds 5] [--out profiles/panoptic_pq.json]"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.data.pseudo_panoptic import id2rgb, rgb2id  # noqa: E402
from u2seg_amd.evaluation import panoptic_ops, pq  # noqa: E402
from u2seg_amd.modeling.inference import combine_semantic_and_instance_outputs_batch, paste_masks_in_images  # noqa: E402
from u2seg_amd.structures import Boxes, Instances  # noqa: E402

HBM_PEAK = 8.0e12
DEV = "cuda:0"


def seeded_maps(h, w, images, n, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    probs, boxes = [], []
    for _ in range(images):
        c = torch.rand(n, 2, generator=g) * 12 + 8
        s = torch.rand(n, generator=g) * 6 + 4
        p = torch.exp(-((xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2) / (2 * s[:, None, None] ** 2))
        bw, bh = torch.rand(n, generator=g) * w * 0.4 + 16, torch.rand(n, generator=g) * h * 0.4 + 16
        x0, y0 = torch.rand(n, generator=g) * (w - 16), torch.rand(n, generator=g) * (h - 16)
        probs.append(p.clamp(0, 1).to(DEV))
        boxes.append(torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1).to(DEV))
    masks = paste_masks_in_images(probs, boxes, [(h, w)] * images, 0.5)
    insts, sems = [], []
    for m, b in zip(masks, boxes):
        inst = Instances((h, w))
        inst.pred_masks, inst.pred_boxes = m, Boxes(b)
        inst.scores = (torch.rand(n, generator=g) * 0.5 + 0.5).to(DEV)
        inst.pred_classes = torch.randint(0, 8, (n,), generator=g).to(DEV)
        sem = torch.randint(0, 28, (h // 50 + 1, w // 50 + 1), generator=g).repeat_interleave(50, 0).repeat_interleave(50, 1)
        insts.append(inst)
        sems.append(sem[:h, :w].contiguous().to(DEV))
    return combine_semantic_and_instance_outputs_batch(insts, sems, 0.5, 4096, 0.5, 28)


def gt_blobs(rs, k, h, w):
    """[h, w] ground-truth ids: k elliptic blobs with 24-bit ids over void, the last one not in segments_info."""
    yy, xx = np.mgrid[0:h, 0:w]
    ids = np.sort(rs.choice(np.arange(65536, 1 << 24), size=k, replace=False))
    gt = np.zeros((h, w), dtype=np.int64)
    for i in ids:
        cx, cy, rx, ry = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(w / 10, w / 3), rs.uniform(h / 10, h / 3)
        gt[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1] = i
    segs = [{"id": int(i), "category_id": int(rs.randint(0, 28)), "iscrowd": int(rs.rand() < 0.1)} for i in ids[:-1]]
    return gt, segs


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (2 device calls, 2 kernel-only launches, host passes); >= 5")
    ap.add_argument("--instances", type=int, default=40)
    ap.add_argument("--gt", type=int, default=24)
    ap.add_argument("--host-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_panoptic_pq.py needs a GPU: there is nothing to measure without one")
    assert args.rounds >= 5, "at least 10 device samples"
    cats = {c: {"isthing": int(c < 8)} for c in range(28)}
    lines = []
    for h, w in ((480, 640), (800, 1333)):
        for images in (8, 32):
            merged = seeded_maps(h, w, images, args.instances, seed=h + images)
            rs = np.random.RandomState(w + images)
            truth = [gt_blobs(rs, args.gt, h, w) for _ in range(images)]
            preds = [pan for pan, _ in merged]
            pred_segs = [[{"id": s["id"], "category_id": s["category_id"] if s["isthing"] else s["category_id"] % 20 + 8}
                          for s in info] for _, info in merged]
            gts = [id2rgb(gt) for gt, _ in truth]
            tables = [sorted(s["id"] for s in segs) for _, segs in truth]
            cols = [max([s["id"] for s in info] + [0]) + 1 for _, info in merged]
            torch.cuda.synchronize()
            for _ in range(2):  # warm-up: code objects, the allocators' blocks (device and pinned)
                tabs = panoptic_ops.pair_counts_batch(preds, gts, tables, cols)
            prepared = panoptic_ops._Prepared(preds, gts, tables, cols)
            prepared.upload()
            prepared.launch()
            dev_ms, wall_ms, kern_ms, fin_ms, img_ms, png_ms, syncs = [], [], [], [], [], [], []
            for r in range(args.rounds):
                for _ in range(2):
                    before = dict(panoptic_ops.counters)
                    tabs, ms, wall = timed(lambda: panoptic_ops.pair_counts_batch(preds, gts, tables, cols))
                    dev_ms.append(ms / images)
                    wall_ms.append(wall / images)
                    syncs.append(tuple(panoptic_ops.counters[k] - before[k] for k in ("host_syncs", "d2h_transfers", "h2d_transfers")))
                    _, ms, _ = timed(prepared.launch)
                    kern_ms.append(ms / images)
                for k in range(args.host_images):  # the parent's path and the finishing of the new one, image by image
                    i = (r * args.host_images + k) % images
                    pred_h = preds[i].cpu().numpy()
                    gt_ids, gt_segs = truth[i]
                    a, b = pq.PQStat(), pq.PQStat()
                    t0 = time.perf_counter()
                    pq.accumulate_image(a, gt_ids, gt_segs, pred_h, pred_segs[i], cats)
                    t1 = time.perf_counter()
                    pq.accumulate_counts(b, tabs[i], tables[i], gt_segs, pred_segs[i], cats)
                    t2 = time.perf_counter()
                    img_ms.append((t1 - t0) * 1e3)
                    fin_ms.append((t2 - t1) * 1e3)
                    assert (a.iou, a.tp, a.fp, a.fn) == (b.iou, b.tp, b.fp, b.fn), i  # same answers, at the size that is timed
                    with io.BytesIO() as buf:  # the ground-truth png exists on disk already: not timed
                        Image.fromarray(gts[i]).save(buf, format="PNG")
                        gt_png = buf.getvalue()
                    t0 = time.perf_counter()
                    with io.BytesIO() as buf:
                        Image.fromarray(id2rgb(pred_h)).save(buf, format="PNG")
                        back = rgb2id(np.asarray(Image.open(io.BytesIO(buf.getvalue()))))
                    rgb2id(np.asarray(Image.open(io.BytesIO(gt_png))))
                    png_ms.append((time.perf_counter() - t0) * 1e3)
                    assert np.array_equal(back, pred_h)
            assert all(np.array_equal(t, panoptic_ops.host_pair_counts(p, g, tb, c))
                       for t, p, g, tb, c in list(zip(tabs, preds, gts, tables, cols))[:2])
            nbytes = images * h * w * 7
            d, kk, f, im = spread(dev_ms), spread(kern_ms), spread(fin_ms), spread(img_ms)
            total = d["median"] + f["median"]
            lines.append({"size": [h, w], "images": images, "instances": args.instances, "gt_segments": args.gt,
                          "mean_pred_segments": float(np.mean([len(s) for s in pred_segs])),
                          "mean_table_entries": float(np.mean([t.size for t in tabs])),
                          "device_ms": d, "call_wall_ms": spread(wall_ms), "kernel_ms": kk, "finish_ms": f,
                          "device_total_ms": total, "image_ms": im, "png_ms": spread(png_ms),
                          "speedup_median": im["median"] / total, "bytes": nbytes,
                          "kernel_hbm_share": nbytes / (kk["median"] * images * 1e-3) / HBM_PEAK,
                          "host_syncs": sorted(set(s[0] for s in syncs)), "d2h_transfers": sorted(set(s[1] for s in syncs)),
                          "h2d_transfers": sorted(set(s[2] for s in syncs)), "results_equal_host": True})
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
