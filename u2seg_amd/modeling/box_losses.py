"""The box heads' loss options written out in plain torch: fp32 ops under autograd, on any device.  These are the definitions
the HIP kernels of csrc/losses.hip (u2_sigmoid_ce, u2_box_reg_loss, u2_box_reg_loss_cls, u2_rpn_loss_level_opt) are measured
against, as impl="host" is for the test-time augmentation.

  sigmoid_cross_entropy    roi_heads/fast_rcnn.py:386-422
  fed_loss_classes_mask    roi_heads/fast_rcnn.py:356-382, 414-416
  box_reg_loss             roi_heads/fast_rcnn.py:424-463 over modeling/box_regression.py:310-369, layers/losses.py:5-133 and
                           Box2BoxTransform (box_regression.py:43-116); class specific with cls_agnostic=False
  rpn_box_reg_loss         proposal_generator/rpn.py:405-413 over box_regression.py:310-369 (_dense_box_regression_loss)
  rpn_objectness_loss      proposal_generator/rpn.py:415-420
  predict_boxes_cls        roi_heads/fast_rcnn.py:494-524 with 4 K deltas per row

GIoU: the reference takes giou_loss from fvcore.  Here it is pinned as
    loss = 1 - I / (U + eps) + (C - U) / (C + eps),   eps = 1e-7,
with I the intersection (zero unless both overlaps are strictly positive), U = A1 + A2 - I and C the area of the smallest
enclosing box.  No fvcore run stands behind this: parity unpinned."""
import math

import torch
import torch.nn.functional as TF

BOX_REG_LOSS_TYPES = ("smooth_l1", "giou", "diou", "ciou")
EPS = 1e-7


def sigmoid_cross_entropy(logits, gt_classes, num_classes, class_weight=None):
    """logits [N, >= K + 1] (columns past K + 1 are padding), gt_classes int64 [N] in [0, K] with K the background.
    sum over the K foreground columns of BCE-with-logits against the one-hot target, times class_weight [K] where given,
    divided by N; 0 for an empty input."""
    k = num_classes
    logits = logits[:, : k + 1].float()
    n = logits.shape[0]
    if logits.numel() == 0:
        return logits.new_zeros([1])[0]
    target = logits.new_zeros(n, k + 1)
    target[torch.arange(n, device=logits.device), gt_classes] = 1
    target = target[:, :k]
    cls_loss = TF.binary_cross_entropy_with_logits(logits[:, :-1], target, reduction="none")
    if class_weight is not None:
        cls_loss = cls_loss * class_weight.view(1, k).expand(n, k).float()
    return torch.sum(cls_loss) / n


def fed_loss_classes_mask(gt_classes, num_fed, num_classes, weight, extra_classes=None):
    """The federated loss's class set as a float mask [K]: 1 for every class present in gt_classes and for as many more as are
    needed to reach num_fed, drawn without replacement with probability proportional to `weight` [K]; classes already present
    and the background have probability 0.  As in the reference, whose torch.unique sees it, a background label among
    gt_classes counts as one of the num_fed (its column is then dropped: num_fed - 1 foreground classes stay).

    No host synchronisation: presence is a scatter, the draw has a fixed length min(num_fed, K), and its leading
    num_fed - present entries are kept by a comparison on the device.  A prefix of a draw without replacement has the
    distribution of the shorter draw, so this is the reference's distribution (its torch.unique sizes a tensor on the host).

    Two cases in which the reference's torch.multinomial raises are served instead: with fewer candidates of non-zero weight
    than are wanted, those that exist are taken (draws of zero-weight classes are discarded), and with num_fed > K the same.

    extra_classes (int64 [M], tests): stands in for the draw; its leading num_fed - present entries are used as they are."""
    k = num_classes
    dev = gt_classes.device
    present = torch.zeros(k + 1, dtype=torch.float32, device=dev)
    present[gt_classes] = 1                                       # scatter; the background lands in column K
    want = num_fed - present.sum()                                # <= 0: nothing is added
    present = present[:k]
    prob = weight.float() * (1 - present)
    if extra_classes is None:
        # (multinomial wants a positive total: a uniform floor over rows it can never be asked to use - see `keep` below)
        draw = torch.multinomial(prob + (prob.sum() <= 0).float(), min(num_fed, k), replacement=False)
    else:
        draw = extra_classes.to(dev)
    keep = (torch.arange(draw.numel(), device=dev) < want) & (prob[draw] > 0)
    mask = present.clone()
    mask[draw] = torch.maximum(mask[draw], keep.float())
    return mask


def get_deltas(src, tgt, weights):
    """Box2BoxTransform.get_deltas (box_regression.py:43-76)."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcx, tcy = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), dim=1)


def apply_deltas(deltas, boxes, weights, scale_clamp):
    """Box2BoxTransform.apply_deltas (box_regression.py:78-116) for [N, 4] deltas."""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    wx, wy, ww, wh = weights
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw = torch.clamp(deltas[:, 2] / ww, max=scale_clamp)
    dh = torch.clamp(deltas[:, 3] / wh, max=scale_clamp)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1)


def _overlap(b1, b2):
    x1, y1, x2, y2 = b1.unbind(dim=-1)
    x1g, y1g, x2g, y2g = b2.unbind(dim=-1)
    xk1, yk1 = torch.max(x1, x1g), torch.max(y1, y1g)
    xk2, yk2 = torch.min(x2, x2g), torch.min(y2, y2g)
    inter = torch.zeros_like(x1)
    mask = (yk2 > yk1) & (xk2 > xk1)
    inter[mask] = (xk2[mask] - xk1[mask]) * (yk2[mask] - yk1[mask])
    return (x1, y1, x2, y2), (x1g, y1g, x2g, y2g), inter


def giou_loss(b1, b2, eps=EPS):
    """The pinned GIoU (module docstring), per row."""
    (x1, y1, x2, y2), (x1g, y1g, x2g, y2g), inter = _overlap(b1, b2)
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    area_c = (torch.max(x2, x2g) - torch.min(x1, x1g)) * (torch.max(y2, y2g) - torch.min(y1, y1g))
    return 1 - inter / (union + eps) + (area_c - union) / (area_c + eps)


def _diou_terms(b1, b2, eps):
    (x1, y1, x2, y2), (x1g, y1g, x2g, y2g), inter = _overlap(b1, b2)
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter + eps
    iou = inter / union
    xc1, yc1 = torch.min(x1, x1g), torch.min(y1, y1g)
    xc2, yc2 = torch.max(x2, x2g), torch.max(y2, y2g)
    diag = ((xc2 - xc1) ** 2) + ((yc2 - yc1) ** 2) + eps
    x_p, y_p = (x2 + x1) / 2, (y2 + y1) / 2
    x_g, y_g = (x1g + x2g) / 2, (y1g + y2g) / 2
    dist = ((x_p - x_g) ** 2) + ((y_p - y_g) ** 2)
    return iou, dist / diag


def diou_loss(b1, b2, eps=EPS):
    """layers/losses.py:5-63, per row."""
    iou, term = _diou_terms(b1, b2, eps)
    return 1 - iou + term


def ciou_loss(b1, b2, eps=EPS):
    """layers/losses.py:66-133, per row; alpha carries no gradient."""
    iou, term = _diou_terms(b1, b2, eps)
    w_pred, h_pred = b1[..., 2] - b1[..., 0], b1[..., 3] - b1[..., 1]
    w_gt, h_gt = b2[..., 2] - b2[..., 0], b2[..., 3] - b2[..., 1]
    v = (4 / (math.pi ** 2)) * torch.pow((torch.atan(w_gt / h_gt) - torch.atan(w_pred / h_pred)), 2)
    with torch.no_grad():
        alpha = v / (1 - iou + v + eps)
    return 1 - iou + term + alpha * v


_IOU_LOSSES = {"giou": giou_loss, "diou": diou_loss, "ciou": ciou_loss}


def _box_rows_loss(kind, pred, src, gt, weights, beta, scale_clamp):
    """The summed loss of rows of four deltas `pred` against their source boxes and ground truth (all [n, 4], fp32)."""
    if kind not in BOX_REG_LOSS_TYPES:
        raise ValueError("Invalid box regression loss type '%s' (one of %s)" % (kind, ", ".join(BOX_REG_LOSS_TYPES)))
    if kind == "smooth_l1":
        n = torch.abs(pred - get_deltas(src, gt, weights))
        if beta < 1e-5:
            return n.sum()
        return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum()
    return _IOU_LOSSES[kind](apply_deltas(pred, src, weights, scale_clamp), gt).sum()


def box_reg_loss(kind, deltas, proposals, gt_boxes, gt_classes, num_classes, weights, beta=0.0,
                 scale_clamp=math.log(1000.0 / 16), cls_agnostic=True):
    """The box regression loss over the foreground rows 0 <= gt_classes < K, summed (the caller divides by max(R, 1)).
    deltas [R, >= 4] (class agnostic: the first four columns) or, with cls_agnostic=False, [R, >= 4 K]: a row of class c is
    scored on columns 4c .. 4c + 3 (fast_rcnn.py:445-450).  proposals / gt_boxes fp32 [R, 4]."""
    if kind not in BOX_REG_LOSS_TYPES:
        raise ValueError("Invalid box regression loss type '%s' (one of %s)" % (kind, ", ".join(BOX_REG_LOSS_TYPES)))
    fg = (gt_classes >= 0) & (gt_classes < num_classes)
    if cls_agnostic:
        pred = deltas[:, :4].float()[fg]
    else:
        cols = 4 * gt_classes[fg][:, None] + torch.arange(4, device=deltas.device)
        pred = deltas.float()[fg].gather(1, cols)
    return _box_rows_loss(kind, pred, proposals.float()[fg], gt_boxes.float()[fg], weights, beta, scale_clamp)


def predict_boxes_cls(deltas, proposals, num_classes, weights, scale_clamp=math.log(1000.0 / 16)):
    """deltas [R, >= 4 K], proposals [R, 4] -> [R, 4 K]: every class's deltas applied to the row's proposal."""
    r, k = deltas.shape[0], num_classes
    d = deltas[:, : 4 * k].float().reshape(r * k, 4)
    src = proposals.float()[:, None, :].expand(r, k, 4).reshape(r * k, 4)
    return apply_deltas(d, src, weights, scale_clamp).reshape(r, 4 * k)


def rpn_box_reg_loss(kind, labels, match, gt_boxes, anchors, deltas, weights=(1.0, 1.0, 1.0, 1.0), beta=0.0,
                     scale_clamp=math.log(1000.0 / 16)):
    """The RPN's localisation loss, summed over the positives (the caller divides by batch_size_per_image * B).
    labels [B, A] (1 = positive; 0 and -1 take no part), match [B, A] the matched ground truth's index, gt_boxes fp32
    [B, G, 4], anchors fp32 [A, 4] (all levels concatenated), deltas [B, A, 4]."""
    b_idx, a_idx = torch.nonzero(labels == 1, as_tuple=True)
    pred = deltas.float()[b_idx, a_idx]
    gt = gt_boxes.float()[b_idx, match[b_idx, a_idx].long()]
    return _box_rows_loss(kind, pred, anchors.float()[a_idx], gt, weights, beta, scale_clamp)


def rpn_objectness_loss(labels, logits):
    """BCE-with-logits over the anchors with label >= 0, summed.  labels / logits [B, A]."""
    valid = labels >= 0
    return TF.binary_cross_entropy_with_logits(logits.float()[valid], labels[valid].float(), reduction="sum")
