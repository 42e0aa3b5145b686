"""float64 restatements of the box heads' loss options (roi_heads/fast_rcnn.py:386-463, modeling/box_regression.py:43-116 and
310-369, layers/losses.py:5-133; GIoU as DESIGN 21 pins it), written with torch.where instead of masked assignment so that
autograd can be taken twice (the GPU tests propagate rounding errors through first and second derivatives), and the
stand-in for u2seg_amd.layers.functional the CPU tests put under the ROI heads."""
import math

import torch
import torch.nn.functional as TF

F64 = torch.float64
EPS = 1e-7


def sigmoid_ce_terms(z, labels, num_classes, weight=None):
    """z float64 [R, >= K + 1]: per-element loss terms [R, K] and the sigmoid-minus-target gradient [R, K], both times the
    class weight."""
    k = num_classes
    x = z[:, :k]
    t = TF.one_hot(labels.clamp(0, k), k + 1)[:, :k].to(F64) * ((labels >= 0) & (labels < k))[:, None]
    w = torch.ones(k, dtype=F64, device=z.device) if weight is None else weight.to(F64)
    terms = (x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))) * w
    return terms, (torch.sigmoid(x) - t) * w


def get_deltas(src, tgt, weights):
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcx, tcy = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), 1)


def decode(deltas, boxes, weights, scale_clamp):
    """apply_deltas; also returns which of dw / dh were clamped."""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    wx, wy, ww, wh = weights
    dw, dh = deltas[:, 2] / ww, deltas[:, 3] / wh
    clamped = torch.stack((dw > scale_clamp, dh > scale_clamp), 1)
    dw, dh = dw.clamp(max=scale_clamp), dh.clamp(max=scale_clamp)
    pcx, pcy = deltas[:, 0] / wx * w + cx, deltas[:, 1] / wy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), 1), clamped


def iou_loss_rows(kind, b, g, eps=EPS):
    """Per-row GIoU / DIoU / CIoU loss of boxes b against g."""
    x1, y1, x2, y2 = b.unbind(1)
    x1g, y1g, x2g, y2g = g.unbind(1)
    iw = torch.minimum(x2, x2g) - torch.maximum(x1, x1g)
    ih = torch.minimum(y2, y2g) - torch.maximum(y1, y1g)
    inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
    area = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g)
    cw = torch.maximum(x2, x2g) - torch.minimum(x1, x1g)
    ch = torch.maximum(y2, y2g) - torch.minimum(y1, y1g)
    if kind == "giou":
        union, c = area - inter, cw * ch
        return 1 - inter / (union + eps) + (c - union) / (c + eps)
    iou = inter / (area - inter + eps)
    dist = ((x2 + x1) / 2 - (x1g + x2g) / 2) ** 2 + ((y2 + y1) / 2 - (y1g + y2g) / 2) ** 2
    loss = 1 - iou + dist / (cw ** 2 + ch ** 2 + eps)
    if kind == "ciou":
        v = (4 / math.pi ** 2) * (torch.atan((x2g - x1g) / (y2g - y1g)) - torch.atan((x2 - x1) / (y2 - y1))) ** 2
        alpha = (v / (1 - iou + v + eps)).detach()
        loss = loss + alpha * v
    return loss


def smooth_l1_rows(pred, target, beta):
    n = (pred - target).abs()
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum(1)


def branch_margin(b, g):
    """The smallest distance [rows] of a max / min pair or an overlap test of iou_loss_rows from its switching point: where it
    lies within the error of the decoded coordinates, the branch the fp32 arithmetic takes is not determined."""
    pairs = torch.stack([(b[:, q] - g[:, q]).abs() for q in range(4)], 1).amin(1)
    iw = torch.minimum(b[:, 2], g[:, 2]) - torch.maximum(b[:, 0], g[:, 0])
    ih = torch.minimum(b[:, 3], g[:, 3]) - torch.maximum(b[:, 1], g[:, 1])
    return torch.minimum(pairs, torch.minimum(iw.abs(), ih.abs()))


class TorchLossFunctional:
    """What u2seg_amd/modeling/roi_heads.py asks of layers/functional.py for its losses, served by torch on any device:
    the definitions of u2seg_amd/modeling/box_losses.py and torch's own cross entropy.  Every call is recorded by name."""

    def __init__(self):
        self.calls = []

    def softmax_cross_entropy(self, logits, labels, num_classes, counters=None):
        self.calls.append("softmax_cross_entropy")
        return TF.cross_entropy(logits[:, :num_classes].float(), labels, reduction="mean")

    def sigmoid_cross_entropy(self, logits, labels, num_classes, class_weight=None, counters=None):
        from u2seg_amd.modeling.box_losses import sigmoid_cross_entropy

        self.calls.append("sigmoid_cross_entropy")
        return sigmoid_cross_entropy(logits, labels, num_classes - 1, class_weight)

    def box_reg_l1_loss(self, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer):
        from u2seg_amd.modeling.box_losses import box_reg_loss

        self.calls.append("box_reg_l1_loss")
        return box_reg_loss("smooth_l1", pred, proposals, gt_boxes, labels, bg_label, weights, 0.0) / normalizer

    def box_reg_loss(self, kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0,
                     scale_clamp=math.log(1000.0 / 16)):
        from u2seg_amd.modeling.box_losses import box_reg_loss

        self.calls.append("box_reg_loss:" + kind)
        return box_reg_loss(kind, pred, proposals, gt_boxes, labels, bg_label, weights, beta, scale_clamp) / normalizer
