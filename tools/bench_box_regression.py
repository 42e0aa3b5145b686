#!/usr/bin/env python
"""What the RPN's localisation loss options and class-specific box regression cost.  GPU only: fails without a device.

Two training shapes, forward plus backward per call, each form on its own:

  rpn     16 images' anchors over the five FPN levels of an 800 x 1216 batch (strides 4 .. 64, A = 3: 243 k anchors per
          image), the fused 32-wide maps, 256 sampled anchors per image of which 64 positive, G = 8.  The default
          pair (L1, unit weights: u2_rpn_loss_level), the same options through u2_rpn_loss_level_opt, smooth-L1 with beta = 0.5,
          GIoU, DIoU and CIoU with the weights (1, 1, 1, 1), and the torch definitions (modeling/box_losses.py: objectness +
          rpn_box_reg_loss on the maps' columns).
  heads   R = 8192 rows (16 images x 512 proposals), K = 800, 25 % foreground.  The default pair (class agnostic, deltas 32
          wide: u2_box_reg_l1 and u2_apply_deltas), the class-specific loss on the 3200-wide map (u2_box_reg_loss_cls) for L1,
          smooth-L1, GIoU, DIoU, CIoU with its torch definitions, and the class-specific decode (u2_apply_deltas_cls) with its.

Per form: device-event time per call, median / min / max over the repetitions (each a run of back-to-back calls between two
events, the forms alternating), and the number of kernels one call launches, counted by torch.profiler in a pass of its own
(null where the profiler is not available).

    python tools/bench_box_regression.py [--calls 200] [--reps 7] [--out profiles/box_regression.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_box_losses import time_forms  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
B, A, G, LP_RPN = 16, 3, 8, 32
LEVELS = [(200, 304, 4, 32.0), (100, 152, 8, 64.0), (50, 76, 16, 128.0), (25, 38, 32, 256.0), (13, 19, 64, 512.0)]
R, K, LP_CLS, LP_AGN = 8192, 800, 3200, 32
HEAD_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
UNIT = (1.0, 1.0, 1.0, 1.0)
BETA = 0.5
FORMS = (("smooth_l1", BETA), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0))


def level_anchors(h, w, stride, size):
    ys, xs = torch.meshgrid(torch.arange(h, device=DEV) * float(stride), torch.arange(w, device=DEV) * float(stride), indexing="ij")
    ratios = torch.tensor([0.5, 1.0, 2.0], device=DEV)
    aw, ah = size / ratios.sqrt(), size * ratios.sqrt()
    cx, cy = xs.reshape(-1, 1), ys.reshape(-1, 1)
    return torch.stack((cx - aw / 2, cy - ah / 2, cx + aw / 2, cy + ah / 2), -1).reshape(-1, 4).contiguous()


def rpn_inputs():
    g = torch.Generator(device=DEV).manual_seed(0)
    anchors = [level_anchors(*lv) for lv in LEVELS]
    cat = torch.cat(anchors)
    atot = cat.shape[0]
    labels = torch.full((B, atot), -1, dtype=torch.int8, device=DEV)
    match = torch.zeros((B, atot), dtype=torch.int32, device=DEV)
    gt = torch.zeros((B, G, 4), device=DEV)
    for b in range(B):
        pick = torch.randperm(atot, generator=g, device=DEV)[:256]
        labels[b, pick[64:]] = 0
        labels[b, pick[:64]] = 1
        # each image's boxes: eight of its positives' anchors, moved and resized a little; every positive is matched to one of them
        src = cat[pick[:G]]
        wh = (src[:, 2:] - src[:, :2]).repeat(1, 2)
        gt[b] = src + torch.randn((G, 4), generator=g, device=DEV) * wh * 0.1
        match[b, pick[:64]] = torch.randint(0, G, (64,), generator=g, device=DEV).to(torch.int32)
    maps = []
    for h, w, _, _ in LEVELS:
        m = (torch.randn((B, h, w, LP_RPN), generator=g, device=DEV) * 0.5).to(BF16)
        m._u2_rpn_fused = True
        maps.append(m)
    return anchors, cat, labels, match, gt, maps


def head_inputs():
    g = torch.Generator(device=DEV).manual_seed(1)
    lab = torch.where(torch.rand(R, generator=g, device=DEV) < 0.25, torch.randint(0, K, (R,), generator=g, device=DEV),
                      torch.full((R,), K, device=DEV))
    xy = torch.rand((R, 2), generator=g, device=DEV) * torch.tensor([1300.0, 780.0], device=DEV)
    wh = 2 + torch.rand((R, 2), generator=g, device=DEV) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((R, 4), generator=g, device=DEV) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    pred = torch.randn((R, LP_CLS), generator=g, device=DEV).to(BF16)
    return lab, prop, gt, pred, pred[:, :LP_AGN].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_regression.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_box_regression.py measures on the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional as F
    from u2seg_amd.modeling import box_losses as BL

    _hip.load()
    clamp = math.log(1000.0 / 16)
    anchors, cat, labels, match, gt, maps = rpn_inputs()
    norm = 256.0 * B

    def rpn_hip(**opts):
        def run():
            leaves = []
            for m in maps:
                leaf = m.detach().requires_grad_(True)
                leaf._u2_rpn_fused = True
                leaves.append(leaf)
            cls, loc = F.rpn_losses(labels, match, gt, anchors, A, norm, leaves, leaves, **opts)
            (cls + loc).backward()
        return run

    def rpn_torch(kind, beta):
        def run():
            leaves = [m.detach().requires_grad_(True) for m in maps]
            obj = torch.cat([m[..., :A].reshape(B, -1) for m in leaves], 1)
            dlt = torch.cat([m[..., A:5 * A].reshape(B, -1, 4) for m in leaves], 1)
            loss = (BL.rpn_objectness_loss(labels, obj) + BL.rpn_box_reg_loss(kind, labels, match, gt, cat, dlt, UNIT, beta, clamp)) / norm
            loss.backward()
        return run

    rpn = {"L1  hip (default: u2_rpn_loss_level)": rpn_hip(),
           "L1  hip (u2_rpn_loss_level_opt, weights 10 10 5 5)": rpn_hip(weights=HEAD_WEIGHTS),
           "L1  torch": rpn_torch("smooth_l1", 0.0)}
    for kind, beta in FORMS:
        rpn["%s  hip" % kind] = rpn_hip(box_reg_loss_type=kind, smooth_l1_beta=beta)
        rpn["%s  torch" % kind] = rpn_torch(kind, beta)

    lab, prop, gtb, pred, pred_agn = head_inputs()

    def fb(loss_of, x):
        def run():
            leaf = x.detach().requires_grad_(True)
            loss_of(leaf).backward()
        return run

    heads = {"L1  class agnostic, hip (default: u2_box_reg_l1)": fb(lambda t: F.box_reg_l1_loss(t, prop, gtb, lab, K, HEAD_WEIGHTS, R),
                                                                      pred_agn)}
    for kind, beta in (("smooth_l1", 0.0),) + FORMS:
        name = "L1" if (kind, beta) == ("smooth_l1", 0.0) else kind
        heads["%s  class specific, hip" % name] = fb(
            lambda t, kind=kind, beta=beta: F.box_reg_loss_cls(kind, t, prop, gtb, lab, K, HEAD_WEIGHTS, R, beta), pred)
        heads["%s  class specific, torch" % name] = fb(
            lambda t, kind=kind, beta=beta: BL.box_reg_loss(kind, t, prop, gtb, lab, K, HEAD_WEIGHTS, beta, clamp, False) / R, pred)
    decode = {
        "decode  class agnostic, hip (default: u2_apply_deltas)":
            lambda: F.apply_deltas(prop, pred_agn[:, :4].float().contiguous(), HEAD_WEIGHTS, None, None, clamp),
        "decode  class specific, hip (u2_apply_deltas_cls)": lambda: F.apply_deltas_cls(prop, pred, K, HEAD_WEIGHTS, clamp),
        "decode  class specific, torch": lambda: BL.predict_boxes_cls(pred, prop, K, HEAD_WEIGHTS, clamp),
    }
    atot = cat.shape[0]
    out = {"device": torch.cuda.get_device_name(0), "unit": "ms per call",
           "rpn_shape": "%d images, levels %s, A = %d: %d anchors per image, fused %d-wide maps, 256 sampled (64 positive) per image, "
                        "G = %d; forward + backward per call" % (B, [lv[:2] for lv in LEVELS], A, atot, LP_RPN, G),
           "rpn": time_forms(rpn, args.calls, args.reps),
           "heads_shape": "R = %d, K = %d, deltas %d wide (class agnostic: %d), 25 %% foreground; forward + backward per call, "
                          "decode: forward only" % (R, K, LP_CLS, LP_AGN),
           "heads": time_forms(heads, args.calls, args.reps),
           "decode": time_forms(decode, args.calls, args.reps)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
