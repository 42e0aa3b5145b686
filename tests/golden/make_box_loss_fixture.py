"""Generates tests/golden/box_loss_golden.npz / .json: what the reference computes for the box heads' loss options on small
fixed inputs.  Runs only where the reference is checked out; the output is committed and the tests read nothing else.

    python tests/golden/make_box_loss_fixture.py

  * diou_loss / ciou_loss (layers/losses.py) on 64 box pairs, per-row values and the gradient with respect to the first box.
    Planted pairs: disjoint, one inside the other (both ways), a ground truth 1 px wide.
  * FastRCNNOutputLayers (roi_heads/fast_rcnn.py) on 64 rows, K = 12:
      - sigmoid_cross_entropy_loss with use_sigmoid_ce, value and logit gradient;
      - the same with use_fed_loss and a fixed class set: torch.multinomial is replaced for the call by a function that hands
        out the leading entries of a stored list, so the mask of fast_rcnn.py:414-416 is a known one;
      - box_reg_loss for diou, ciou and smooth_l1 at beta = 0.5 (smooth_l1_loss is the stand-in of make_fixtures.py), value and
        delta gradient, with the first cascade stage's weights.  One row's dw lies above the scale clamp.

Stored: the inputs and every result, fp32."""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

K, R, NUM_FED, BETA = 12, 64, 9, 0.5
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def boxes(rs, n):
    xy = rs.rand(n, 2).astype(np.float32) * np.array([300.0, 200.0], dtype=np.float32)
    wh = (4 + rs.rand(n, 2) ** 2 * 150).astype(np.float32)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def main():
    from make_fixtures import import_reference

    import_reference()
    from detectron2.layers import ShapeSpec
    from detectron2.layers.losses import ciou_loss, diou_loss
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.modeling.roi_heads.fast_rcnn import FastRCNNOutputLayers

    rs = np.random.RandomState(7)
    arrays = {}

    # ---- the two losses of layers/losses.py ---------------------------------------------------------
    b2 = boxes(rs, R)
    wh = np.tile(b2[:, 2:] - b2[:, :2], (1, 2))
    b1 = (b2 + rs.randn(R, 4).astype(np.float32) * wh * 0.15).astype(np.float32)
    b1[:, 2:] = np.maximum(b1[:, 2:], b1[:, :2] + 1)
    b1[0] = b2[0] + np.array([1000, 0, 1000, 0], dtype=np.float32)              # disjoint
    b1[1] = b2[1] + np.array([1, 1, -1, -1], dtype=np.float32)                  # the first inside the second
    b1[2] = b2[2] + np.array([-3, -2, 2, 5], dtype=np.float32)                  # the second inside the first
    b2[3, 2] = b2[3, 0] + 1                                                     # a ground truth 1 px wide
    arrays["b1"], arrays["b2"] = b1, b2
    for name, fn in (("diou", diou_loss), ("ciou", ciou_loss)):
        x = torch.from_numpy(b1).requires_grad_(True)
        v = fn(x, torch.from_numpy(b2))
        v.sum().backward()
        arrays[name + "_rows"], arrays[name + "_rows_grad"] = v.detach().numpy(), x.grad.numpy()

    # ---- FastRCNNOutputLayers -----------------------------------------------------------------------
    logits = (rs.randn(R, K + 1) * 3).astype(np.float32)
    gt = np.array([0, 1, 3, 4, 8], dtype=np.int64)[rs.randint(0, 5, size=R)]   # five of the twelve classes occur
    gt[::3] = K                                   # background rows
    fed_w = (rs.rand(K) + 0.5).astype(np.float32)
    fed_w[9] = 0                                  # class 9 does not occur and cannot be drawn
    prop = boxes(rs, R)
    pwh = np.tile(prop[:, 2:] - prop[:, :2], (1, 2))
    gtb = (prop + rs.randn(R, 4).astype(np.float32) * pwh * 0.1).astype(np.float32)
    gtb[:, 2:] = np.maximum(gtb[:, 2:], gtb[:, :2] + 1)
    deltas = (rs.randn(R, 4) * np.array([1.0, 1.0, 0.5, 0.5])).astype(np.float32)
    fg_rows = np.nonzero(gt < K)[0]
    deltas[fg_rows[0], 2] = 25.0                  # dw = 5 > log(1000 / 16): clamped
    arrays.update(logits=logits, gt_classes=gt, fed_weight=fed_w, prop=prop, gtb=gtb, deltas=deltas)

    def layers(**kw):
        return FastRCNNOutputLayers(ShapeSpec(channels=8), box2box_transform=Box2BoxTransform(weights=WEIGHTS), num_classes=K,
                                    cls_agnostic_bbox_reg=True, **kw)

    def cls_loss(layer, prefix):
        z = torch.from_numpy(logits).requires_grad_(True)
        loss = layer.sigmoid_cross_entropy_loss(z, torch.from_numpy(gt))
        loss.backward()
        arrays[prefix + "_loss"], arrays[prefix + "_grad"] = loss.detach().numpy(), z.grad.numpy()

    cls_loss(layers(use_sigmoid_ce=True), "sigmoid")

    present = np.unique(gt)
    candidates = [c for c in range(K) if c not in present and fed_w[c] > 0]
    extra = np.array(rs.permutation(candidates), dtype=np.int64)
    assert len(present) < NUM_FED <= len(present) + len(extra), (present, extra)   # (the reference counts the background in)
    fed_layer = layers(use_sigmoid_ce=True, use_fed_loss=True, get_fed_loss_cls_weights=lambda: torch.from_numpy(fed_w),
                       fed_loss_num_classes=NUM_FED)
    real_multinomial = torch.multinomial
    asked = []

    def given(prob, n, replacement=False):
        assert not replacement and bool((prob[torch.from_numpy(extra[:n])] > 0).all())
        asked.append(int(n))
        return torch.from_numpy(extra[:n])

    torch.multinomial = given
    try:
        cls_loss(fed_layer, "fed")
        classes = fed_layer.get_fed_loss_classes(torch.from_numpy(gt), NUM_FED, K, fed_layer.fed_loss_cls_weights)
    finally:
        torch.multinomial = real_multinomial
    mask = torch.zeros(K + 1)
    mask[classes] = 1                             # fast_rcnn.py:414-416
    arrays["fed_extra"], arrays["fed_mask"] = extra, mask[:K].numpy()

    for kind, beta in (("diou", 0.0), ("ciou", 0.0), ("smooth_l1", BETA)):
        layer = layers(box_reg_loss_type=kind, smooth_l1_beta=beta)
        d = torch.from_numpy(deltas).requires_grad_(True)
        loss = layer.box_reg_loss(torch.from_numpy(prop), torch.from_numpy(gtb), d, torch.from_numpy(gt))
        loss.backward()
        arrays["box_%s_loss" % kind], arrays["box_%s_grad" % kind] = loss.detach().numpy(), d.grad.numpy()

    meta = {"num_classes": K, "rows": R, "fed_loss_num_classes": NUM_FED, "smooth_l1_beta": BETA, "weights": list(WEIGHTS),
            "scale_clamp": math.log(1000.0 / 16), "multinomial_asked_for": asked,
            "losses": {k: float(v) for k, v in arrays.items() if k.endswith("_loss")}}
    np.savez_compressed(os.path.join(HERE, "box_loss_golden.npz"), **{k: np.asarray(v) for k, v in arrays.items()})
    with open(os.path.join(HERE, "box_loss_golden.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
