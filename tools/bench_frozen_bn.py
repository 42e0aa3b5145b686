#!/usr/bin/env python
"""What FrozenBN and a frozen backbone prefix cost per training step.  GPU only: fails without a device.

One configuration per invocation (one process each), at the benchmark's shape (16 images of 3 x 800 x 1333, bf16, synthetic
COCO-panoptic batches, random initial weights, the solver of the config):

  default      configs/COCO-PanopticSegmentation/u2seg_R50_800.yaml: SyncBN everywhere, nothing frozen
  frozenbn     u2seg_R50_800_finetune.yaml with BACKBONE.FREEZE_AT 0: FrozenBN in the bottom-up network, every layer trains
  finetune     u2seg_R50_800_finetune.yaml: FrozenBN, stem and res2 frozen

Per configuration: device-event time per step over --steps steps after --warmup (median / min / max of the single steps), and
from ONE further step under torch.profiler the number of kernel launches, the launches and device time of the normalisation /
element-wise family (the kernels of csrc/norm.hip that touch activations, the stem's fused tail, ATen's element-wise kernels)
and of the two kernels of csrc/frozen.hip (fold, scaled gradient accumulate).  The result is merged into --out under the
configuration's name.  No pass / fail threshold: the file records what was measured.

Each invocation under its own time limit, the next one only after the last has ended well:

    timeout -k 10 300 python tools/bench_frozen_bn.py --config default && \\
    timeout -k 10 300 python tools/bench_frozen_bn.py --config frozenbn && \\
    timeout -k 10 300 python tools/bench_frozen_bn.py --config finetune"""
import argparse
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG_DIR = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation")
CONFIGS = {
    "default": ("u2seg_R50_800.yaml", []),
    "frozenbn": ("u2seg_R50_800_finetune.yaml", ["MODEL.BACKBONE.FREEZE_AT", 0]),
    "finetune": ("u2seg_R50_800_finetune.yaml", []),
}
# activation-sized passes that are neither a convolution nor a head: norm.hip's apply / reduce / ReLU kernels, the fused stem
# tail and the pool of pool_resize.hip, ATen's element-wise kernels
NORM_FAMILY = re.compile(r"affine_act|affine_upadd|affine_relu_maxpool|bn_finalize|gn_finalize|colreduce|colstats|norm_bwd_apply|"
                         r"relu_bwd|add_n_kernel|maxpool_(fwd|bwd)|bn_act_fused|bn_bwd_apply|elementwise")
FROZEN = {"fold": re.compile(r"frozen_fold_kernel"), "scale_add": re.compile(r"frozen_wgrad_scale_add_kernel")}


def census(step):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith("Memcpy")
               and not e.name.startswith("Memset")]

    def total(pred):
        sel = [e for e in kernels if pred(e.name)]
        return {"launches": len(sel), "ms": round(sum(e.device_time for e in sel) / 1e3, 4)}

    out = {"kernel_launches": len(kernels), "kernel_ms": round(sum(e.device_time for e in kernels) / 1e3, 3),
           "norm_elementwise": total(lambda n: bool(NORM_FAMILY.search(n))),
           "conv": total(lambda n: ("conv" in n or "wgrad" in n) and "frozen" not in n)}
    for key, rx in FROZEN.items():
        out["frozen_" + key] = total(lambda n, rx=rx: bool(rx.search(n)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool needs the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.engine import SimpleTrainer
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer

    _hip.load()
    dev = "cuda:0"
    name, opts = CONFIGS[args.config]
    torch.manual_seed(1234)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CFG_DIR, name))
    cfg.merge_from_list(["MODEL.DEVICE", dev, "SOLVER.IMS_PER_BATCH", args.batch] + opts)
    model = build_model(cfg)
    model.train()
    opt = build_optimizer(cfg, model)
    trainer = SimpleTrainer(model, opt, build_lr_scheduler(cfg, opt))
    batches = [make_synthetic_batch(args.batch, start_index=i * args.batch, height=args.height, width=args.width, device=dev)
               for i in range(2)]
    torch.manual_seed(1000)
    for i in range(args.warmup):
        trainer.run_step(batches[i % 2])
    torch.cuda.synchronize()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    events[0].record()
    for i in range(args.steps):
        trainer.run_step(batches[i % 2])
        events[i + 1].record()
    torch.cuda.synchronize()
    total_loss = trainer.check_finite()
    each = [events[i].elapsed_time(events[i + 1]) for i in range(args.steps)]
    row = {"config": name, "opts": opts, "batch": args.batch, "height": args.height, "width": args.width, "steps": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "trainable_tensors": sum(p.requires_grad for p in model.parameters()),
           "trainable_elements": int(opt.total),
           "step_ms": {"median": statistics.median(each), "min": min(each), "max": max(each),
                       "mean": events[0].elapsed_time(events[-1]) / args.steps, "each": [round(v, 3) for v in each]},
           "final_total_loss": total_loss}

    def write():
        data = {}
        if os.path.exists(args.out):
            data = json.load(open(args.out))
        data[args.config] = row
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:   # one line per configuration
            f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(data[k], sort_keys=True)) for k in sorted(data)) + "\n}\n")

    write()   # the timing is on disk before the profiled step
    if not args.no_census:
        row["census_one_step"] = census(lambda: trainer.run_step(batches[0]))
        write()
    print(json.dumps({args.config: row}))


if __name__ == "__main__":
    main()
