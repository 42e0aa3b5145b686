#!/usr/bin/env python
"""Cost of a precise-BN pass (u2seg_amd/engine/precise_bn.py) at the training shape, batch 16 x 800 x 1333 synthetic images (canvas
800 x 1344), on cuda:0, in one process, device events around each timed region:
  * pass_iter_ms: one statistics iteration - the backbone (ResNet-50 + FPN) training forward under no_grad at momentum 1.0 and one
    u2_bn_precise_update launch (update_bn_stats over `--iters` batches, finalize included, divided by the batch count);
  * update_us / finalize_us: the two kernels alone, `--reps` back-to-back launches each over the 61 layers (28 608 channels);
  * step_ms: one training step (SimpleTrainer.run_step) of the same batch, for comparison.
usage: python tools/bench_precise_bn.py [--iters 10] [--warmup 2] [--reps 200]   (prints one JSON line)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from u2seg_amd import _hip  # noqa: E402
from u2seg_amd.config import get_cfg  # noqa: E402
from u2seg_amd.data import make_synthetic_batch  # noqa: E402
from u2seg_amd.engine import SimpleTrainer, get_bn_modules, update_bn_stats  # noqa: E402
from u2seg_amd.engine.precise_bn import _LayerTable, _backbone_strides  # noqa: E402
from u2seg_amd.modeling import build_model  # noqa: E402
from u2seg_amd.solver import build_optimizer  # noqa: E402


def timed(fn, n):
    """ms per call of fn over n calls, device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--batch", type=int, default=16)
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_precise_bn needs cuda:0"
    _hip.load()
    dev = "cuda:0"
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", dev])
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    trainer = SimpleTrainer(model, build_optimizer(cfg, model))
    batch = make_synthetic_batch(args.batch, start_index=0, device=dev)

    for _ in range(args.warmup):
        trainer.run_step(batch)
    step_ms = timed(lambda: trainer.run_step(batch), args.iters)

    update_bn_stats(model, iter([batch] * args.warmup), args.warmup)
    pass_ms = timed(lambda: update_bn_stats(model, iter([batch] * args.iters), args.iters), 1)

    layers = get_bn_modules(model)
    strides = _backbone_strides(model.backbone)
    table = _LayerTable(layers, [strides[id(bn)] for bn in layers], torch.device(dev))
    h, w = 800, 1344
    update_us = 1e3 * timed(lambda: table.update(args.batch, h, w), args.reps)
    finalize_us = 1e3 * timed(table.finalize, args.reps)
    channels = table.channels
    print(json.dumps({
        "batch": args.batch, "canvas": [h, w], "layers": len(layers), "channels": channels,
        "pass_iter_ms": round(pass_ms / args.iters, 3), "step_ms": round(step_ms, 3),
        "pass_200_s": round(200 * pass_ms / args.iters / 1e3, 2),
        "update_us": round(update_us, 2), "finalize_us": round(finalize_us, 2),
        # bytes each launch moves: update reads mean, var (fp32) and reads + writes A, Q (fp64) per channel; finalize reads A, Q
        # and writes mean, var (the table and T are a few KB)
        "update_bytes": channels * (4 + 4 + 2 * 8 + 2 * 8), "finalize_bytes": channels * (2 * 8 + 2 * 4),
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()
