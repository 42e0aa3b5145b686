#!/usr/bin/env python
"""Boundary IoU's pixel work per image: the device call (csrc/semeval.hip through evaluation/semseg_ops.boundary_confusion, one
launch that adds to the plain and the boundary confusion matrix) against the host definition on the CPU
(semseg_ops.boundary_confusion_host) and against what the semantic evaluator's process() costs with the option off (LUT
gather + bincount on the device).  GPU only: fails without a device.

Input: blob-like label maps with 17 labels (seeded ellipses over label 0), prediction clusters 0 .. 27 behind a chained table,
at 480 x 640 / d = 16 and 800 x 1333 / d = 31.  One JSON line per size:
  device_ms        per image, device events around `launches` back-to-back calls, median / min / max over the repetitions
                   after warm-up
  device_wall_ms   per image, host clock around the same calls including the final synchronisation
  host_ms          per image, boundary_confusion_host on CPU tensors (host clock)
  process_off_ms   per image, device events around SemSegEvaluator.process with boundary_iou=False on device logits (argmax,
                   ground-truth upload, LUT gather, bincount)
  process_on_ms    the same with boundary_iou=True
  bytes            what the kernel has to read per image: 2 bytes per pixel
    python tools/bench_boundary_iou.py [--reps 20] [--launches 50] [--out profiles/semseg_boundary.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.evaluation import semseg_ops  # noqa: E402
from u2seg_amd.evaluation.sem_seg_evaluation import STUFF_TO_SUPERCATEGORY, SemSegEvaluator  # noqa: E402

DEV = "cuda:0"
N = 17


def blob_map(rs, h, w, labels, k=24):
    """[h, w] uint8: k ellipses with labels drawn from `labels` over label 0."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=np.uint8)
    for _ in range(k):
        cx, cy, rx, ry = rs.uniform(0, w), rs.uniform(0, h), rs.uniform(w / 10, w / 3), rs.uniform(h / 10, h / 3)
        m[((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1] = rs.choice(labels)
    return m


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def timed(fn, times):
    """`times` calls of fn between two device events: (device ms, wall ms) per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(times):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / times, (time.perf_counter() - t0) * 1e3 / times


class _Evaluator(SemSegEvaluator):
    """SemSegEvaluator.process on arrays in memory: no dataset catalog, no mapping file, no png decoding in the timing."""

    def __init__(self, gt, lut, boundary_iou):
        self._ignore_label, self._num_classes, self.mode, self._boundary_iou = 255, 16, "eval", boundary_iou
        self.input_file_to_gt_file = {"image": "gt"}
        self.sem_seg_loading_fn = lambda name, dtype: gt.astype(dtype)
        self._lut, self._lut8 = torch.from_numpy(lut.astype(np.int64)), None
        self.reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions after warm-up; >= 10")
    ap.add_argument("--launches", type=int, default=50, help="device calls between the two events of a repetition")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary_iou.py needs a GPU: there is nothing to measure without one")
    assert args.reps >= 10, "at least 10 device samples"
    lut = np.zeros(256, dtype=np.uint8)
    lut[:28] = np.concatenate([[0], np.arange(1, 28) % 16 + 1])  # clusters onto 1 .. 16 (16 = ignore), 0 kept
    lines = []
    for h, w in ((480, 640), (800, 1333)):
        rs = np.random.RandomState(h + w)
        d = semseg_ops.boundary_dilation(h, w)
        pred, gt = blob_map(rs, h, w, np.arange(1, 28)), blob_map(rs, h, w, np.arange(1, 17))
        pred_t, gt_t, lut_t = torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(lut)
        pred_d, gt_d, lut_d = pred_t.to(DEV), gt_t.to(DEV), lut_t.to(DEV)
        conf = torch.zeros((N, N), dtype=torch.int64, device=DEV)
        bconf = torch.zeros((N, N), dtype=torch.int64, device=DEV)
        call = lambda: semseg_ops.boundary_confusion(pred_d, gt_d, lut_d, d, N, conf, bconf)  # noqa: E731
        call()
        want_c, want_b = semseg_ops.boundary_confusion_host(pred_t, gt_t, lut_t, d, N)
        assert torch.equal(conf.cpu(), want_c) and torch.equal(bconf.cpu(), want_b)  # same answers, at the size that is timed
        logits = torch.zeros((28, h, w), dtype=torch.float32)
        logits.scatter_(0, pred_t.long()[None], 1.0)
        logits_d = logits.to(DEV)
        to_file = np.array([0] + [STUFF_TO_SUPERCATEGORY.index(c) + 1 for c in range(1, 16)] + [255], dtype=np.uint8)
        gt_file = to_file[gt]  # as the evaluator reads it: a stuff id of the supercategory, ignore = 255
        evs = {on: _Evaluator(gt_file, lut, on) for on in (False, True)}
        inputs, outputs = [{"file_name": "image"}], [{"sem_seg": logits_d}]
        for _ in range(3):  # warm-up: code objects, the allocator's blocks
            timed(call, args.launches)
            for ev in evs.values():
                ev.process(inputs, outputs)
        assert torch.equal(evs[True]._conf_matrix, evs[False]._conf_matrix) and torch.equal(evs[True]._conf_matrix.cpu(), 3 * want_c)
        assert torch.equal(evs[True]._b_conf_matrix.cpu(), 3 * want_b)
        dev_ms, wall_ms, off_ms, on_ms, host_ms = [], [], [], [], []
        for _ in range(args.reps):
            ms, wall = timed(call, args.launches)
            dev_ms.append(ms)
            wall_ms.append(wall)
            off_ms.append(timed(lambda: evs[False].process(inputs, outputs), 5)[0])
            on_ms.append(timed(lambda: evs[True].process(inputs, outputs), 5)[0])
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            semseg_ops.boundary_confusion_host(pred_t, gt_t, lut_t, d, N)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        dm, hm = spread(dev_ms), spread(host_ms)
        lines.append({"size": [h, w], "d": d, "labels": N, "launches": args.launches, "device_ms": dm,
                      "device_wall_ms": spread(wall_ms), "host_ms": hm, "process_off_ms": spread(off_ms),
                      "process_on_ms": spread(on_ms), "host_over_device_median": hm["median"] / dm["median"],
                      "bytes": 2 * h * w, "host_threads": torch.get_num_threads(), "results_equal_host": True})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
