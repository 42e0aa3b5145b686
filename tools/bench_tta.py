#!/usr/bin/env python
"""Test-time augmentation per image: GeneralizedRCNNWithTTA(impl="device") against impl="host" (the reference's procedure restated:
PIL views, a device <-> host round trip per view for the boxes, a dense score matrix, one image at a time) in one run, alternately,
after warm-up.  GPU only: fails without a device.

Model and input: u2seg_eval_800 with det_fill weights (tests/golden/make_fixtures.py) and the score thresholds lowered until
detections come through, one synthetic 800 x 1333 image, the default TEST.AUG (9 sizes x flip = 18 views), batch_size 3.
One JSON object:
  device_ms / host_ms           per image, device events around one call, median / min / max over the repetitions
  device_wall_ms / host_wall_ms the host clock around the same call, ending in a synchronise
  recompute_ms / _wall_ms       impl="device" with keep_features=False (the backbone runs twice over every view, as in the reference)
  stages_*_ms                   wall clock per stage with a synchronise at every boundary (separate repetitions: the boundaries
                                cost overlap): views, detect, merge (boxes to the original + NMS), masks, reduce (mean + paste)
  syncs_*                       host synchronisations per image: calls of tolist / item / cpu / nonzero / bool() on device tensors
  kept_feature_bytes            the FPN maps of all view batches together: what keep_features holds between the two passes
  peak_bytes_*                  torch.cuda.max_memory_allocated over one call
    python tools/bench_tta.py [--reps 10] [--out profiles/tta.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.golden.make_fixtures import det_fill  # noqa: E402
from u2seg_amd.config import get_cfg  # noqa: E402
from u2seg_amd.data import make_synthetic_batch  # noqa: E402
from u2seg_amd.modeling import GeneralizedRCNN, GeneralizedRCNNWithTTA, build_model  # noqa: E402
from u2seg_amd.modeling import test_time_augmentation as tta  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
STAGES = ("views", "detect", "merge", "masks", "reduce")


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def timed(fn):
    """One call between two device events: (device ms, wall ms including the final synchronisation)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


class SyncCounter:
    """Counts the calls that make the host wait for the device, on device tensors."""

    NAMES = ("tolist", "item", "cpu", "nonzero", "__bool__", "numpy")

    def __enter__(self):
        self.count, self.saved = 0, {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def wrapped(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.count += 1
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


def device_stages(wrapper, batch):
    """Wall ms per stage of the device path, a synchronise at every boundary."""
    marks = []

    def hook(name):
        torch.cuda.synchronize()
        marks.append((name, time.perf_counter()))

    wrapper.stage_hook = hook
    try:
        wrapper(batch)
    finally:
        wrapper.stage_hook = None
    return {a: (t1 - t0) * 1e3 for (a, t0), (_, t1) in zip(marks, marks[1:])}


def host_stages(wrapper, batch):
    """The same split of the host path: its methods timed with a synchronise on both sides."""
    acc = dict.fromkeys(STAGES, 0.0)

    def wrap(owner, name, stage, minus=None):
        orig = getattr(owner, name)

        def timed_call(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = orig(*a, **k)
            torch.cuda.synchronize()
            acc[stage] += (time.perf_counter() - t0) * 1e3
            return out

        setattr(owner, name, timed_call)
        return orig

    saved = {"tta_mapper": wrap(wrapper, "tta_mapper", "views")}
    for name, stage in (("_get_augmented_boxes", "detect"), ("_merge_detections", "merge"), ("_rescale_detected_boxes", "masks"),
                        ("_reduce_pred_masks", "reduce")):
        wrap(wrapper, name, stage)
        saved[name] = None
    import u2seg_amd.modeling.test_time_augmentation as mod

    post = mod.detector_postprocess
    total_masks = [0.0]
    batch_inf = wrapper._batch_inference

    def mask_pass(inputs, instances=None):
        if instances is None:
            return batch_inf(inputs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = batch_inf(inputs, instances)
        torch.cuda.synchronize()
        total_masks[0] += (time.perf_counter() - t0) * 1e3
        return out

    def post_timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = post(*a, **k)
        torch.cuda.synchronize()
        acc["reduce"] += (time.perf_counter() - t0) * 1e3
        return out

    wrapper._batch_inference = mask_pass
    mod.detector_postprocess = post_timed
    try:
        wrapper(batch)
    finally:
        mod.detector_postprocess = post
        del wrapper._batch_inference
        wrapper.tta_mapper = saved["tta_mapper"]
        for name in saved:
            if name != "tta_mapper":
                delattr(wrapper, name)
    acc["masks"] += total_masks[0]
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed repetitions per path after warm-up")
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py needs a GPU: there is nothing to measure without one")
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_eval_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0015,
                         "MODEL.PANOPTIC_FPN.COMBINE.INSTANCES_CONFIDENCE_THRESH", 0.0016])
    model = build_model(cfg)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(det_fill(k, v.cpu()).to(DEV))
    model.eval()
    x = make_synthetic_batch(1, start_index=0, height=800, width=1333, device=DEV)[0]
    batch = [{"image": x["image"], "height": 800, "width": 1333}]
    paths = {"device": GeneralizedRCNNWithTTA(cfg, model, impl="device"),
             "recompute": GeneralizedRCNNWithTTA(cfg, model, impl="device", keep_features=False),
             "host": GeneralizedRCNNWithTTA(cfg, model, impl="host")}
    outs = {}
    for name, w in paths.items():  # warm-up: code objects, the allocator's blocks, the pinned ring
        for _ in range(2):
            outs[name] = w(batch)[0]["instances"]
    equal = all(torch.equal(outs[n].pred_boxes.tensor, outs["host"].pred_boxes.tensor) and torch.equal(outs[n].scores, outs["host"].scores)
                and torch.equal(outs[n].pred_classes, outs["host"].pred_classes) and torch.equal(outs[n].pred_masks, outs["host"].pred_masks)
                for n in ("device", "recompute"))
    ms = {n: [] for n in paths}
    wall = {n: [] for n in paths}
    for _ in range(args.reps):
        for name, w in paths.items():  # alternately: drift of the machine hits every path alike
            d, t = timed(lambda: w(batch))
            ms[name].append(d)
            wall[name].append(t)
    syncs, peak = {}, {}
    for name, w in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        with SyncCounter() as c:
            w(batch)
        torch.cuda.synchronize()
        syncs[name], peak[name] = c.count, torch.cuda.max_memory_allocated()
    stage_ms = {"device": [], "host": []}
    for _ in range(args.stage_reps):
        stage_ms["device"].append(device_stages(paths["device"], batch))
        stage_ms["host"].append(host_stages(paths["host"], batch))
    stages = {n: {s: float(np.median([r[s] for r in runs])) for s in STAGES} for n, runs in stage_ms.items()}
    # what keep_features holds: the FPN maps of every view batch
    kept, shapes = 0, []
    with torch.no_grad():
        tfms = paths["device"].tta_mapper.view_transforms((800, 1333), (800, 1333))
        geometry = [(t.transforms[0].new_h, t.transforms[0].new_w, len(t.transforms) > 1) for t in tfms]  # [resize] or [resize, flip]
        views = tta.device_views(batch[0]["image"], geometry)
        for b0 in range(0, len(views), 3):
            feats, _, _ = GeneralizedRCNN._backbone_features(model, [{"image": v} for v in views[b0:b0 + 3]])
            kept += sum(f.numel() * f.element_size() for f in feats.values())
            shapes.append({k: [list(f.shape), str(f.dtype)] for k, f in feats.items()})
            del feats
    line = {"input": [800, 1333], "views": len(tfms), "view_sizes": [[g[0], g[1]] for g in geometry[::2]], "batch_size": 3,
            "instances": len(outs["host"]), "results_equal_host": bool(equal),
            "device_ms": spread(ms["device"]), "device_wall_ms": spread(wall["device"]),
            "recompute_ms": spread(ms["recompute"]), "recompute_wall_ms": spread(wall["recompute"]),
            "host_ms": spread(ms["host"]), "host_wall_ms": spread(wall["host"]),
            "host_over_device_wall_median": float(np.median(wall["host"]) / np.median(wall["device"])),
            "stages_device_ms": stages["device"], "stages_host_ms": stages["host"],
            "syncs_device": syncs["device"], "syncs_recompute": syncs["recompute"], "syncs_host": syncs["host"],
            "kept_feature_bytes": kept, "kept_feature_maps_first_batch": shapes[0],
            "peak_bytes_device": peak["device"], "peak_bytes_recompute": peak["recompute"], "peak_bytes_host": peak["host"],
            "host_threads": torch.get_num_threads()}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
