#!/usr/bin/env python
"""What the semantic and panoptic outputs cost on top of instance test-time augmentation, per image, in one run: (a)
GeneralizedRCNNWithTTA(impl="device"), (b) PanopticFPNWithTTA(impl="device"), (c) PanopticFPNWithTTA(impl="host"), alternately,
after warm-up; and the accumulate kernel alone against the same reduction from existing pieces.  GPU only: fails without a device.

Model and input as tools/bench_tta.py: u2seg_eval_800 with det_fill weights and lowered score thresholds, one synthetic
800 x 1333 image, the default TEST.AUG (9 sizes x flip = 18 views), batch_size 3.  One JSON object:
  instances_device_ms / panoptic_device_ms / panoptic_host_ms   device events around one call, median / min / max
  *_wall_ms                     the host clock around the same call, ending in a synchronise
  extra_device_ms               median(b) - median(a): the semantic head on 18 views, the accumulate calls and the merge
  stages_panoptic_device_ms     wall clock per stage of (b) with a synchronise at every boundary (separate repetitions)
  peak_bytes_*                  torch.cuda.max_memory_allocated over one call
  kernel                        the reduction of the 18 views' logits (random, in padded blocks as the head leaves them) alone:
    fused_ms                    u2_tta_accumulate_sem_seg, six calls of three views, device events, per image
    pieces_ms                   u2_bilinear_resize_f32 per view (none for the identity views, as sem_seg_postprocess), flip, add
                                in view order, one division - what impl="host" launches for the reduction
    fused_bytes                 bytes the fused calls have to move: every view's window once, the accumulator read and written
                                once per call (not read by the first), the arg-max map
    fused_GBps, share_of_hbm    fused_bytes over fused_ms, and over the 6.3 TB/s a float4 copy reaches on this chip
    python tools/bench_tta_panoptic.py [--reps 10] [--out profiles/tta_panoptic.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_tta import device_stages, spread, timed  # noqa: E402
from tests.golden.make_fixtures import det_fill  # noqa: E402
from u2seg_amd.config import get_cfg  # noqa: E402
from u2seg_amd.data import make_synthetic_batch  # noqa: E402
from u2seg_amd.modeling import GeneralizedRCNNWithTTA, PanopticFPNWithTTA, build_model  # noqa: E402
from u2seg_amd.modeling import tta_panoptic as tta  # noqa: E402
from u2seg_amd.modeling.test_time_augmentation import mean_in_view_order  # noqa: E402
from u2seg_amd.modeling.inference import sem_seg_postprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HBM_GBPS = 6300.0  # achievable HBM rate of the MI355X (float4 copy)
STAGES = ("views", "detect", "merge", "masks", "reduce", "panoptic")


def kernel_alone(geometry, classes, size, batch_size, reps, divisibility=32):
    """The reduction of one image's view logits: fused calls against resize + flip + add.  geometry: ((h, w, flip), ...)."""
    H, W = size
    gen = torch.Generator(device=DEV).manual_seed(0)
    blocks, windows, flips = [], [], []
    for h, w, f in geometry:
        hp, wp = -(-h // divisibility) * divisibility, -(-w // divisibility) * divisibility
        blocks.append(torch.empty((classes, hp, wp), dtype=torch.float32, device=DEV).uniform_(-8, 8, generator=gen))
        windows.append((h, w))
        flips.append(bool(f))
    acc = torch.empty((classes, H, W), dtype=torch.float32, device=DEV)
    amax = torch.empty((H, W), dtype=torch.int64, device=DEV)
    n = len(blocks)

    def fused():
        for v in range(0, n, batch_size):
            last = v + batch_size >= n
            tta.tta_accumulate_sem_seg(blocks[v:v + batch_size], windows[v:v + batch_size], flips[v:v + batch_size], acc, v == 0,
                                       n if last else 0, amax if last else None)
        return acc

    def pieces():
        terms = []
        for b, win, f in zip(blocks, windows, flips):
            t = sem_seg_postprocess(b, win, H, W)
            terms.append(t.flip(dims=[2]) if f else t)
        return mean_in_view_order(terms)

    for _ in range(2):
        equal = bool(torch.equal(fused(), pieces()))
    ms = {"fused": [], "pieces": []}
    for _ in range(reps):
        ms["fused"].append(timed(fused)[0])
        ms["pieces"].append(timed(pieces)[0])
    calls = -(-n // batch_size)
    nbytes = sum(4 * classes * h * w for h, w in windows) + 4 * classes * H * W * (2 * calls - 1) + 8 * H * W
    med = float(np.median(ms["fused"]))
    return {"views": n, "classes": classes, "calls": calls, "results_equal_pieces": equal, "fused_ms": spread(ms["fused"]),
            "pieces_ms": spread(ms["pieces"]), "fused_bytes": nbytes, "fused_GBps": nbytes / med / 1e6,
            "share_of_hbm": nbytes / med / 1e6 / HBM_GBPS, "hbm_GBps_assumed": HBM_GBPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="timed repetitions per path after warm-up")
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta_panoptic.py needs a GPU: there is nothing to measure without one")
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
    paths = {"instances_device": GeneralizedRCNNWithTTA(cfg, model, impl="device"),
             "panoptic_device": PanopticFPNWithTTA(cfg, model, impl="device"),
             "panoptic_host": PanopticFPNWithTTA(cfg, model, impl="host")}
    outs = {}
    for name, w in paths.items():  # warm-up: code objects, the allocator's blocks, the pinned ring
        for _ in range(2):
            outs[name] = w(batch)[0]
    d, h = outs["panoptic_device"], outs["panoptic_host"]
    equal = bool(torch.equal(d["sem_seg"], h["sem_seg"]) and torch.equal(d["panoptic_seg"][0], h["panoptic_seg"][0])
                 and d["panoptic_seg"][1] == h["panoptic_seg"][1]
                 and torch.equal(d["instances"].pred_masks, outs["instances_device"]["instances"].pred_masks))
    segments = len(d["panoptic_seg"][1])
    del outs, d, h
    ms = {n: [] for n in paths}
    wall = {n: [] for n in paths}
    for _ in range(args.reps):
        for name, w in paths.items():  # alternately: drift of the machine hits every path alike
            dev_ms, wall_ms = timed(lambda: w(batch))
            ms[name].append(dev_ms)
            wall[name].append(wall_ms)
    peak = {}
    for name, w in paths.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        w(batch)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
    runs = [device_stages(paths["panoptic_device"], batch) for _ in range(args.stage_reps)]
    stages = {s: float(np.median([r[s] for r in runs])) for s in STAGES}
    tfms = paths["panoptic_device"].tta_mapper.view_transforms((800, 1333), (800, 1333))
    geometry = [(t.transforms[0].new_h, t.transforms[0].new_w, len(t.transforms) > 1) for t in tfms]  # [resize] or [resize, flip]
    with torch.no_grad():
        kernel = kernel_alone(geometry, model.sem_seg_head.num_classes, (800, 1333), 3, args.reps)
    line = {"input": [800, 1333], "views": len(tfms), "view_sizes": [[g[0], g[1]] for g in geometry[::2]], "batch_size": 3,
            "classes": model.sem_seg_head.num_classes, "panoptic_segments": segments, "results_equal_host": equal}
    for name in paths:
        line[name + "_ms"], line[name + "_wall_ms"] = spread(ms[name]), spread(wall[name])
        line["peak_bytes_" + name] = peak[name]
    line["extra_device_ms"] = float(np.median(ms["panoptic_device"]) - np.median(ms["instances_device"]))
    line["extra_device_wall_ms"] = float(np.median(wall["panoptic_device"]) - np.median(wall["instances_device"]))
    line["host_over_device_wall_median"] = float(np.median(wall["panoptic_host"]) / np.median(wall["panoptic_device"]))
    line["stages_panoptic_device_ms"] = stages
    line["kernel"] = kernel
    line["host_threads"] = torch.get_num_threads()
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
