#!/usr/bin/env python
"""What the box heads' loss options cost.  GPU only: fails without a device.

One cascade stage's losses at the training shape (R = 8192 rows = 16 images x 512 proposals, K = 800 classes, logits 832 wide,
deltas 32 wide, 25 % foreground), forward plus backward, each on its own:

  classification   softmax (u2_softmax_ce, the default), sigmoid and sigmoid with a federated mask of 50 classes, through the
                   HIP path (layers/functional.py) and through the torch definition (modeling/box_losses.py) on the device;
                   and the mask itself (fed_loss_classes_mask: ATen on either path)
  box regression   L1 (u2_box_reg_l1, the default), smooth-L1 with beta = 0.5, GIoU, DIoU, CIoU, HIP and torch definition

Per form: device-event time per call, median / min / max over the repetitions (each a run of back-to-back calls between two
events, the forms alternating), and the number of kernels one call launches, counted by torch.profiler in a pass of its own
(null where the profiler is not available).

    python tools/bench_box_losses.py [--calls 400] [--reps 7] [--out profiles/box_losses.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
BF16 = torch.bfloat16
R, K, LP_CLS, LP_BOX = 8192, 800, 832, 32
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
BETA = 0.5


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "each": [round(x, 5) for x in v]}


def launches_of(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception as e:  # a count is an extra: the times do not depend on it
        print("launch count not available: %s" % e, file=sys.stderr)
        return None


def time_forms(forms, calls, reps):
    for fn in forms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(calls):
                fn()
            e.record()
            e.synchronize()
            out[name].append(s.elapsed_time(e) / calls)
    return {k: dict(summary(v), launches=launches_of(forms[k])) for k, v in out.items()}


def inputs():
    g = torch.Generator(device=DEV).manual_seed(0)
    z = (torch.randn((R, LP_CLS), generator=g, device=DEV) * 3).to(BF16)
    lab = torch.where(torch.rand(R, generator=g, device=DEV) < 0.25, torch.randint(0, K, (R,), generator=g, device=DEV),
                      torch.full((R,), K, device=DEV))
    xy = torch.rand((R, 2), generator=g, device=DEV) * torch.tensor([1300.0, 780.0], device=DEV)
    wh = 2 + torch.rand((R, 2), generator=g, device=DEV) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((R, 4), generator=g, device=DEV) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    pred = torch.randn((R, LP_BOX), generator=g, device=DEV).to(BF16)
    freq = torch.rand(K, generator=g, device=DEV) + 0.1
    return z, lab, prop, gt, pred, freq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_losses.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_box_losses.py measures on the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional as F
    from u2seg_amd.modeling import box_losses as BL

    _hip.load()
    z, lab, prop, gt, pred, freq = inputs()
    mask = BL.fed_loss_classes_mask(lab[:512], 50, K, freq)   # (one image's labels: about 50 classes present or drawn)

    def fb(loss_of, x):
        def run():
            leaf = x.detach().requires_grad_(True)
            loss_of(leaf).backward()
        return run

    cls = {
        "softmax  hip (default)": fb(lambda t: F.softmax_cross_entropy(t, lab, K + 1), z),
        "sigmoid  hip": fb(lambda t: F.sigmoid_cross_entropy(t, lab, K + 1), z),
        "sigmoid  torch": fb(lambda t: BL.sigmoid_cross_entropy(t, lab, K), z),
        "sigmoid + federated mask  hip": fb(lambda t: F.sigmoid_cross_entropy(t, lab, K + 1, mask), z),
        "sigmoid + federated mask  torch": fb(lambda t: BL.sigmoid_cross_entropy(t, lab, K, mask), z),
        "fed_loss_classes_mask (ATen, both paths)": lambda: BL.fed_loss_classes_mask(lab, 50, K, freq),
    }
    box = {"L1  hip (default)": fb(lambda t: F.box_reg_l1_loss(t, prop, gt, lab, K, WEIGHTS, R), pred)}
    for kind, beta in (("smooth_l1", BETA), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0)):
        box["%s  hip" % kind] = fb(lambda t, kind=kind, beta=beta: F.box_reg_loss(kind, t, prop, gt, lab, K, WEIGHTS, R, beta), pred)
        box["%s  torch" % kind] = fb(
            lambda t, kind=kind, beta=beta: BL.box_reg_loss(kind, t, prop, gt, lab, K, WEIGHTS, beta) / R, pred)
    out = {"device": torch.cuda.get_device_name(0),
           "shape": "R = %d, K = %d, logits %d wide, deltas %d wide, 25 %% foreground; forward + backward per call" % (
               R, K, LP_CLS, LP_BOX),
           "unit": "ms per call", "classification": time_forms(cls, args.calls, args.reps),
           "box_regression": time_forms(box, args.calls, args.reps)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
