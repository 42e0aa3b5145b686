"""The head losses: semantic, box classification and regression, mask, RPN - and the device counters some of them feed."""
import math

import torch
from torch.autograd import Function

from .. import _hip
from .weights import BF16, _check_act, zeros_f32


class _SemSegLossFn(Function):
    """bilinear x4 + cross_entropy(mean, ignore) fused (meta_arch/semantic_seg.py:255-267)."""

    @staticmethod
    def forward(ctx, logits, target_u8, num_classes, ignore):
        _check_act(logits)
        b, h, w, lp = logits.shape
        assert target_u8.dtype == torch.uint8 and target_u8.shape == (b, 4 * h, 4 * w)
        acc = torch.empty((b, h, w, lp), dtype=torch.float32, device=logits.device)  # every element is written
        sc = zeros_f32((2,), logits.device)
        _hip.call("u2_semseg_upsample_ce", logits, target_u8.contiguous(), acc, sc[0:1], sc[1:2], b, h, w, lp,
                  num_classes, ignore)
        ctx.save_for_backward(acc, sc)
        return sc[0] / sc[1]

    @staticmethod
    def backward(ctx, g):
        acc, sc = ctx.saved_tensors
        d = torch.empty(acc.shape, dtype=BF16, device=acc.device)
        gg = g.detach().float().reshape(1).contiguous()
        _hip.call("u2_scale_to_bf16", acc, gg, sc[1:2], 1.0, d, acc.numel())
        return d, None, None, None


def sem_seg_loss(logits, target_u8, num_classes, ignore=255):
    return _SemSegLossFn.apply(logits, target_u8, num_classes, ignore)


class _ScaledGradLossFn(Function):
    """A loss over the rows of `pred` whose kernel writes, beside the loss sum, the gradient d already multiplied by
    1 / divisor: launch(pred, d, loss) runs it, backward is d * g.  The division of the sum stays in here - outside the node
    autograd would scale g by 1 / divisor a second time."""

    @staticmethod
    def forward(ctx, pred, launch, divisor):
        d = torch.empty_like(pred)
        loss = zeros_f32((1,), pred.device)
        launch(pred, d, loss)
        ctx.save_for_backward(d)
        return loss[0] / divisor

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return d * g, None, None   # g: 0-dim fp32, the product keeps d's dtype (one launch)


def _check_counters(counters, n, device):
    assert counters.dtype == torch.int32 and counters.is_contiguous() and counters.numel() >= n and counters.device == device, (
        "expected >= %d contiguous int32 counters on %s" % (n, device))


def softmax_cross_entropy(logits, labels, num_classes, counters=None):
    """cross_entropy(scores, labels, reduction='mean') (roi_heads/fast_rcnn.py:344).
    counters (int32 [>= 5], optional): rows, pred == gt, fg, fg and pred == gt, fg and pred == background are ADDED to it
    (u2_softmax_ce_stats); the loss and its gradient do not depend on it."""
    r, lp = logits.shape

    def launch(x, d, loss):
        if counters is None:
            _hip.call("u2_softmax_ce", x.contiguous(), labels.contiguous(), d, loss, r, num_classes, lp, 1.0 / max(r, 1))
        else:  # the same kernel body, which also counts fast_rcnn.py:88-115 into counters[0..4] (background = the last class)
            _check_counters(counters, 5, x.device)
            _hip.call("u2_softmax_ce_stats", x.contiguous(), labels.contiguous(), d, loss, r, num_classes, lp,
                      1.0 / max(r, 1), counters, num_classes - 1)

    return _ScaledGradLossFn.apply(logits, launch, max(r, 1))


def sigmoid_cross_entropy(logits, labels, num_classes, class_weight=None, counters=None):
    """FastRCNNOutputLayers.sigmoid_cross_entropy_loss (roi_heads/fast_rcnn.py:386-422): BCE-with-logits over the K foreground
    columns, times the federated class mask where given, summed, / rows.
    num_classes counts the background (K + 1 valid columns, as softmax_cross_entropy takes it); class_weight fp32 [K] or None;
    counters as softmax_cross_entropy's."""
    r, lp = logits.shape

    def launch(x, d, loss):
        cw = class_weight
        if cw is not None:
            assert cw.dtype == torch.float32 and cw.numel() >= num_classes - 1
            cw = cw.contiguous()
        if counters is not None:
            _check_counters(counters, 5, x.device)
        _hip.call("u2_sigmoid_ce", x.contiguous(), labels.contiguous(), cw, d, loss, r, num_classes, lp, 1.0 / max(r, 1),
                  counters, num_classes - 1)

    return _ScaledGradLossFn.apply(logits, launch, max(r, 1))


def box_reg_l1_loss(pred, proposals, gt_boxes, labels, bg_label, weights, normalizer):
    """smooth_l1(beta=0) = L1 over foreground rows, summed, / normalizer (roi_heads/fast_rcnn.py:424-463)."""
    r, lp = pred.shape
    normalizer = float(normalizer)

    def launch(x, d, loss):
        _hip.call("u2_box_reg_l1", x.contiguous(), proposals.contiguous(), gt_boxes.contiguous(), labels.contiguous(), d, loss,
                  r, lp, bg_label, weights[0], weights[1], weights[2], weights[3], 1.0 / normalizer)

    return _ScaledGradLossFn.apply(pred, launch, normalizer)


BOX_REG_LOSS_KINDS = {"smooth_l1": _hip.K.BOXLOSS_SMOOTH_L1, "giou": _hip.K.BOXLOSS_GIOU, "diou": _hip.K.BOXLOSS_DIOU,
                      "ciou": _hip.K.BOXLOSS_CIOU}


def box_reg_loss(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0,
                 scale_clamp=math.log(1000.0 / 16)):
    """smooth-L1 with beta > 0 and the IoU-family losses on the decoded box (modeling/box_regression.py:310-369) over foreground
    rows, summed, / normalizer.  kind: smooth_l1 (beta > 0; beta == 0 is box_reg_l1_loss), giou, diou or ciou."""
    if kind not in BOX_REG_LOSS_KINDS:
        raise ValueError("Invalid box regression loss type '%s' (one of %s)" % (kind, ", ".join(BOX_REG_LOSS_KINDS)))
    r, lp = pred.shape
    normalizer, beta, scale_clamp = float(normalizer), float(beta), float(scale_clamp)

    def launch(x, d, loss):
        _hip.call("u2_box_reg_loss", BOX_REG_LOSS_KINDS[kind], x.contiguous(), proposals.contiguous(), gt_boxes.contiguous(),
                  labels.contiguous(), d, loss, r, lp, bg_label, weights[0], weights[1], weights[2], weights[3], beta,
                  scale_clamp, 1.0 / normalizer)

    return _ScaledGradLossFn.apply(pred, launch, normalizer)


def box_reg_loss_cls(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0,
                     scale_clamp=math.log(1000.0 / 16)):
    """box_reg_l1_loss / box_reg_loss for class-specific regression (cls_agnostic_bbox_reg=False): pred [R, LP] holds
    4 * bg_label valid columns and a foreground row of label c is scored on columns 4c .. 4c + 3 (fast_rcnn.py:445-450).  All
    four kinds; smooth_l1 takes any beta >= 0.  The kernel writes the whole [R, LP] gradient, zeros included."""
    if kind not in BOX_REG_LOSS_KINDS:
        raise ValueError("Invalid box regression loss type '%s' (one of %s)" % (kind, ", ".join(BOX_REG_LOSS_KINDS)))
    r, lp = pred.shape
    normalizer, beta, scale_clamp = float(normalizer), float(beta), float(scale_clamp)

    def launch(x, d, loss):
        _hip.call("u2_box_reg_loss_cls", BOX_REG_LOSS_KINDS[kind], x.contiguous(), proposals.contiguous(), gt_boxes.contiguous(),
                  labels.contiguous(), d, loss, r, lp, bg_label, weights[0], weights[1], weights[2], weights[3], beta,
                  scale_clamp, 1.0 / normalizer)

    return _ScaledGradLossFn.apply(pred, launch, normalizer)


class _MaskPredictBCEFn(Function):
    """1x1 predictor restricted to the gt-class channel + BCE-with-logits(mean)
    (roi_heads/mask_head.py:258 + :33-112)."""

    @staticmethod
    def forward(ctx, x, weight, bias, classes, target_u8, phased=False, counters=None):
        n, ph, pw, c = x.shape
        if phased:  # x = the deconvolution's unshuffled phases [n, P, P, 4 C]: the kernel reads (and writes dx) in place
            ph, pw, c = 2 * ph, 2 * pw, c // 4
        p = ph * pw
        k = weight.shape[0]
        w2 = weight.detach().reshape(k, c).float().contiguous()
        b2 = bias.detach().float().contiguous()
        x, classes, target_u8 = x.contiguous(), classes.contiguous(), target_u8.contiguous()
        loss = zeros_f32((1,), x.device)
        denom = float(max(n * p, 1))
        # the loss alone here; the gradients come from a second launch in backward, scaled by the loss's upstream gradient inside
        # the kernel (forming dx here and multiplying it by that scalar in backward was a 0.2 ms pass over dx per step)
        if counters is None:
            _hip.call("u2_mask_predict_bce", x, w2, b2, classes, target_u8, None, None, None, loss, None, n, p, c, 1.0 / denom,
                      ph if phased else 0, None)
        else:  # the same loss, and mask_head.py:90-102's counts into counters[0..3]
            _check_counters(counters, 4, x.device)
            _hip.call("u2_mask_predict_bce_stats", x, w2, b2, classes, target_u8, loss, counters, n, p, c, ph if phased else 0)
        ctx.save_for_backward(x, w2, b2, classes, target_u8)
        ctx.cfg = (n, p, c, k, denom, ph if phased else 0, weight.shape)
        return loss[0] / denom

    @staticmethod
    def backward(ctx, g):
        x, w2, b2, classes, target_u8 = ctx.saved_tensors
        n, p, c, k, denom, phased_side, wshape = ctx.cfg
        dx = torch.empty_like(x)
        dw, db = zeros_f32((k, c), x.device), zeros_f32((k,), x.device)
        _hip.call("u2_mask_predict_bce", x, w2, b2, classes, target_u8, dx, dw, db, None, None, n, p, c, 1.0 / denom, phased_side,
                  g.detach().float().reshape(1).contiguous())
        return dx, dw.view(wshape), db, None, None, None, None


def mask_predict_bce_loss(x, weight, bias, classes, target_u8, phased=False, counters=None):
    """counters (int32 [>= 4], optional): false positives, false negatives, positives and positions are ADDED to it
    (u2_mask_predict_bce_stats)."""
    return _MaskPredictBCEFn.apply(x, weight, bias, classes, target_u8, phased, counters)


def count_labels_i8(labels, counters):
    """counters[0] += #(labels == 1), counters[1] += #(labels == 0) over an int8 tensor (the RPN's subsampled anchor labels)."""
    assert labels.dtype == torch.int8 and labels.is_contiguous()
    _check_counters(counters, 2, labels.device)
    _hip.call("u2_count_labels_i8", labels, labels.numel(), counters)


def mask_predict_prob(x, weight, bias, classes, phased=False):
    """mask_rcnn_inference (roi_heads/mask_head.py:115-158) with the 1x1 predictor folded in: fp32 [n, 1, 2P, 2P] probabilities of
    each detection's predicted class.  x: [n, 2P, 2P, 256] trunk output, or with `phased` the deconvolution's unshuffled GEMM
    output [n, P, P, 4 * 256] (ConvTranspose2d(..., shuffle=False)).  No autograd."""
    _check_act(x)
    n = x.shape[0]
    side = x.shape[1] * 2 if phased else x.shape[1]
    c = x.shape[3] // 4 if phased else x.shape[3]
    out = torch.empty((n, 1, side, side), dtype=torch.float32, device=x.device)
    if n:
        _hip.call("u2_mask_predict_prob", x.contiguous(), weight.detach().reshape(weight.shape[0], -1).contiguous(),
                  bias.detach().contiguous(), classes.to(torch.int64).contiguous(), out, n, side, c, int(phased))
    return out


class _RPNLossFn(Function):
    """RPN objectness BCE(sum) + localisation loss(sum) over all levels, both / normalizer
    (proposal_generator/rpn.py:366-429).  `fused`: each level is ONE map holding objectness (columns 0-2) and deltas (3-14).
    `options`: None = L1 with unit weights (u2_rpn_loss_level), else (kind code, beta, weights, scale_clamp) for
    u2_rpn_loss_level_opt."""

    @staticmethod
    def forward(ctx, labels, match, gt_boxes, anchors_per_level, num_anchors, normalizer, fused, options, *obj_and_deltas):
        nl = len(anchors_per_level)
        objs, dlts = obj_and_deltas[:nl], obj_and_deltas[nl:]
        b, atot = labels.shape
        g = gt_boxes.shape[1]
        loss = zeros_f32((2,), labels.device)
        grads = []
        off = 0
        for lvl in range(nl):
            o = objs[lvl]
            hw = o.shape[1] * o.shape[2]
            if fused:
                go, d, gd = torch.empty_like(o), None, None
            else:
                d = dlts[lvl]
                go, gd = torch.empty_like(o), torch.empty_like(d)
            args = (o, d, labels, match, gt_boxes, anchors_per_level[lvl], go, gd, loss, b, hw, num_anchors, o.shape[3],
                    d.shape[3] if d is not None else 0, atot, off, g, 1.0 / normalizer)
            if options is None:
                _hip.call("u2_rpn_loss_level", *args)
            else:
                kind, beta, weights, scale_clamp = options
                _hip.call("u2_rpn_loss_level_opt", kind, *args, weights[0], weights[1], weights[2], weights[3], beta, scale_clamp)
            grads.append((go, gd))
            off += hw * num_anchors
        assert off == atot
        ctx.grads = grads
        ctx.fused = fused
        ctx.num_anchors = num_anchors
        return loss[0] / normalizer, loss[1] / normalizer

    @staticmethod
    def backward(ctx, g_cls, g_loc):
        if ctx.fused:
            a = ctx.num_anchors
            go0 = ctx.grads[0][0]
            scale = torch.zeros(go0.shape[-1], dtype=torch.float32, device=go0.device)
            scale[:a] = g_cls
            scale[a : 5 * a] = g_loc
            scale = scale.to(go0.dtype)
            return (None, None, None, None, None, None, None, None, *[go * scale for go, _ in ctx.grads])
        gos = [go * g_cls for go, _ in ctx.grads]   # 0-dim fp32 factors: the products keep the maps' dtype
        gds = [gd * g_loc for _, gd in ctx.grads]
        return (None, None, None, None, None, None, None, None, *gos, *gds)


def rpn_losses(labels, match, gt_boxes, anchors_per_level, num_anchors, normalizer, objs, deltas, box_reg_loss_type="smooth_l1",
               smooth_l1_beta=0.0, weights=(1.0, 1.0, 1.0, 1.0), scale_clamp=math.log(1000.0 / 16)):
    """objs / deltas: per level [B, H, W, LP] maps - or, when the head ran both predictors as one conv (the maps carry
    `_u2_rpn_fused`), the fused maps in `objs` (deltas are then views of them and are not used).
    The localisation loss: box_reg_loss_type smooth_l1 (beta >= 0), giou, diou or ciou with the anchors' Box2BoxTransform
    `weights`; smooth_l1 with beta 0 and unit weights is the launch it has always been (u2_rpn_loss_level)."""
    if box_reg_loss_type not in BOX_REG_LOSS_KINDS:
        raise ValueError("Invalid dense box regression loss type '%s' (one of %s)" % (box_reg_loss_type, ", ".join(BOX_REG_LOSS_KINDS)))
    weights = tuple(float(w) for w in weights)
    beta = float(smooth_l1_beta)
    if len(weights) != 4 or min(weights) <= 0 or beta < 0:
        raise ValueError("rpn_losses: four positive weights and beta >= 0 expected, got %r, %r" % (weights, beta))
    options = None
    if (box_reg_loss_type, beta, weights) != ("smooth_l1", 0.0, (1.0, 1.0, 1.0, 1.0)):
        options = (BOX_REG_LOSS_KINDS[box_reg_loss_type], beta, weights, float(scale_clamp))
    if all(getattr(o, "_u2_rpn_fused", False) for o in objs):
        return _RPNLossFn.apply(labels, match, gt_boxes, anchors_per_level, num_anchors, float(normalizer), True, options, *objs)
    return _RPNLossFn.apply(labels, match, gt_boxes, anchors_per_level, num_anchors, float(normalizer), False, options, *objs,
                            *deltas)
