"""Generates tests/golden/box_regression_golden.npz: what the reference computes for the RPN's localisation loss options and for
class-specific box regression on small fixed inputs.  Runs only where the reference is checked out; the output is committed
(arrays only) and the tests read nothing else.

    python tests/golden/make_box_regression_fixture.py

  * RPN.losses (proposal_generator/rpn.py:366-429) on B = 2 images, two levels of 5 x 7 and 2 x 3 positions, A = 3 anchors,
    G = 3 ground-truth boxes; the second image has no ground truth (labels 0 / -1 only, matched boxes all zero, as
    label_and_sample_anchors hands them over).  For diou, ciou, smooth_l1 at beta = 0.5 and at beta = 0, each with the anchor
    weights (1, 1, 1, 1) and (10, 10, 5, 5): loss_rpn_cls, loss_rpn_loc and the gradients with respect to the objectness logits
    and the anchor deltas.  One positive's dw lies above the scale clamp.
  * FastRCNNOutputLayers (roi_heads/fast_rcnn.py) with cls_agnostic_bbox_reg=False on R = 64 rows, K = 12: box_reg_loss for the
    same four forms (value and delta gradient) and predict_boxes ([R, 4 K]).

GIoU is not here: the reference takes it from fvcore, which make_fixtures.py stands in for without a giou_loss of its own.
Stored: the inputs and every result, fp32 (labels int8 / int64, match int32); scalars as 0-d arrays."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

B, A, G = 2, 3, 3
LEVELS = ((5, 7, 8, 32.0), (2, 3, 16, 64.0))      # (h, w, stride, anchor size)
BATCH_PER_IMAGE = 16
K, R, BETA = 12, 64, 0.5
RPN_WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))
HEAD_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
FORMS = (("diou", 0.0, "diou"), ("ciou", 0.0, "ciou"), ("smooth_l1", BETA, "smooth_l1"), ("smooth_l1", 0.0, "l1"))


def level_anchors(h, w, stride, size):
    """Position-major, the three aspect ratios 0.5 / 1 / 2 innermost (the order of the maps' columns)."""
    out = []
    for y in range(h):
        for x in range(w):
            for ratio in (0.5, 1.0, 2.0):
                aw, ah = size / math.sqrt(ratio), size * math.sqrt(ratio)
                cx, cy = x * stride, y * stride
                out.append([cx - aw / 2, cy - ah / 2, cx + aw / 2, cy + ah / 2])
    return np.array(out, dtype=np.float32)


def boxes(rs, n):
    xy = rs.rand(n, 2).astype(np.float32) * np.array([300.0, 200.0], dtype=np.float32)
    wh = (4 + rs.rand(n, 2) ** 2 * 150).astype(np.float32)
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def main():
    from make_fixtures import import_reference

    import_reference()
    from detectron2.layers import ShapeSpec
    from detectron2.modeling.box_regression import Box2BoxTransform
    from detectron2.modeling.matcher import Matcher
    from detectron2.modeling.proposal_generator.rpn import RPN
    from detectron2.modeling.roi_heads.fast_rcnn import FastRCNNOutputLayers
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage

    rs = np.random.RandomState(22)
    arrays = {}

    # ---- RPN.losses ----------------------------------------------------------------------------------------
    per_level = [level_anchors(*lv) for lv in LEVELS]
    anchors = np.concatenate(per_level)
    atot = anchors.shape[0]
    gt = np.zeros((B, G, 4), dtype=np.float32)
    gt[0] = np.array([[2, 1, 40, 30], [20, 10, 52, 38], [0, 0, 70, 90]], dtype=np.float32)
    labels = rs.choice(np.array([-1, 0], dtype=np.int8), size=(B, atot), p=[0.6, 0.4])
    match = np.zeros((B, atot), dtype=np.int32)
    pos = rs.permutation(atot)[:14]                      # positives in both levels of the first image only
    pos = np.concatenate([pos, [atot - 2]])
    labels[0, pos] = 1
    match[0, pos] = rs.randint(0, G, size=len(pos))
    match[0, labels[0] != 1] = rs.randint(0, G, size=int((labels[0] != 1).sum()))   # matches of non-positives take no part
    obj = (rs.randn(B, atot) * 2).astype(np.float32)
    deltas = (rs.randn(B, atot, 4) * np.array([0.5, 0.5, 0.3, 0.3])).astype(np.float32)
    deltas[0, pos[0], 2] = 25.0                          # dw = 5 (weights 5) or 25 (weights 1): above log(1000 / 16)
    arrays.update(rpn_anchors=anchors, rpn_level_hw=np.array([lv[:2] for lv in LEVELS], dtype=np.int64), rpn_gt=gt,
                  rpn_labels=labels, rpn_match=match, rpn_obj=obj, rpn_deltas=deltas,
                  rpn_batch_per_image=np.array(BATCH_PER_IMAGE, dtype=np.int64))
    matched = np.stack([gt[b][match[b]] for b in range(B)])
    matched[1] = 0                                       # no ground truth: label_and_sample_anchors hands over zeros
    splits = np.cumsum([a.shape[0] for a in per_level])[:-1]
    for wi, weights in enumerate(RPN_WEIGHTS):
        for kind, beta, name in FORMS:
            rpn = RPN(in_features=["p"], head=torch.nn.Identity(), anchor_generator=torch.nn.Identity(),
                      anchor_matcher=Matcher([0.3, 0.7], [0, -1, 1], allow_low_quality_matches=True),
                      box2box_transform=Box2BoxTransform(weights=weights), batch_size_per_image=BATCH_PER_IMAGE,
                      positive_fraction=0.5, pre_nms_topk=(10, 10), post_nms_topk=(10, 10), box_reg_loss_type=kind,
                      smooth_l1_beta=beta)
            o = torch.from_numpy(obj).requires_grad_(True)
            d = torch.from_numpy(deltas).requires_grad_(True)
            with EventStorage(0):
                out = rpn.losses([Boxes(torch.from_numpy(a)) for a in per_level],
                                 list(torch.tensor_split(o, list(splits), dim=1)), [torch.from_numpy(l) for l in labels],
                                 list(torch.tensor_split(d, list(splits), dim=1)), [torch.from_numpy(m) for m in matched])
            (go,) = torch.autograd.grad(out["loss_rpn_cls"], o, retain_graph=True)
            (gd,) = torch.autograd.grad(out["loss_rpn_loc"], d)
            key = "rpn_w%d_%s" % (wi, name)
            arrays[key + "_cls"], arrays[key + "_loc"] = out["loss_rpn_cls"].detach().numpy(), out["loss_rpn_loc"].detach().numpy()
            arrays[key + "_dobj"], arrays[key + "_ddeltas"] = go.numpy(), gd.numpy()
    arrays["rpn_weights"] = np.array(RPN_WEIGHTS, dtype=np.float32)

    # ---- FastRCNNOutputLayers, class specific ----------------------------------------------------------------
    cls = np.array([0, 1, 3, 4, 8, 11], dtype=np.int64)[rs.randint(0, 6, size=R)]
    cls[::3] = K                                         # background rows
    prop = boxes(rs, R)
    pwh = np.tile(prop[:, 2:] - prop[:, :2], (1, 2))
    gtb = (prop + rs.randn(R, 4).astype(np.float32) * pwh * 0.1).astype(np.float32)
    gtb[:, 2:] = np.maximum(gtb[:, 2:], gtb[:, :2] + 1)
    hd = (rs.randn(R, 4 * K) * np.tile([1.0, 1.0, 0.5, 0.5], K)).astype(np.float32)
    fg_rows = np.nonzero(cls < K)[0]
    hd[fg_rows[0], 4 * cls[fg_rows[0]] + 2] = 25.0       # the labelled class's dw = 5 > log(1000 / 16): clamped
    arrays.update(head_classes=cls, head_prop=prop, head_gtb=gtb, head_deltas=hd, head_weights=np.array(HEAD_WEIGHTS, np.float32),
                  head_num_classes=np.array(K, dtype=np.int64), beta=np.array(BETA, dtype=np.float32),
                  scale_clamp=np.array(math.log(1000.0 / 16), dtype=np.float32))
    for kind, beta, name in FORMS:
        layer = FastRCNNOutputLayers(ShapeSpec(channels=8), box2box_transform=Box2BoxTransform(weights=HEAD_WEIGHTS),
                                     num_classes=K, cls_agnostic_bbox_reg=False, box_reg_loss_type=kind, smooth_l1_beta=beta)
        d = torch.from_numpy(hd).requires_grad_(True)
        loss = layer.box_reg_loss(torch.from_numpy(prop), torch.from_numpy(gtb), d, torch.from_numpy(cls))
        loss.backward()
        arrays["head_%s_loss" % name], arrays["head_%s_grad" % name] = loss.detach().numpy(), d.grad.numpy()
    inst = Instances((400, 500))
    inst.proposal_boxes = Boxes(torch.from_numpy(prop))
    with torch.no_grad():
        (pred,) = layer.predict_boxes((torch.zeros(R, K + 1), torch.from_numpy(hd)), [inst])
    assert pred.shape == (R, 4 * K)
    arrays["head_pred_boxes"] = pred.numpy()

    np.savez_compressed(os.path.join(HERE, "box_regression_golden.npz"), **{k: np.asarray(v) for k, v in arrays.items()})
    for k in sorted(arrays):
        if np.asarray(arrays[k]).ndim == 0:
            print(k, float(arrays[k]))


if __name__ == "__main__":
    main()
