"""Boundary IoU's pixel work for the semantic evaluator (the reference's _mask_to_boundary and the two bincounts of its
process(), detectron2/evaluation/sem_seg_evaluation.py:264-276, 396-407).

boundary(m) = m - erode(m) in uint8, where erode(m) is the reference's zero ring + d passes of a 3 x 3 minimum: the minimum over
the (2 d + 1) x (2 d + 1) window centred on the pixel with everything outside the image counted as 0.  The boundary value is a
difference of label values, and that difference is what is counted:
    bconf[n * boundary(lut[pred]) + boundary(gt)] += 1        conf[n * lut[pred] + gt] += 1

Two paths with identical results.  Host: `boundary_confusion_host`, torch ops on any device (zero padding, then the square
minimum as two max-pools of the negated map, rows and columns), which is the definition and the route for maps that live on
the CPU.  Device (csrc/semeval.hip, taken when the maps live on a GPU): `boundary_confusion` makes one launch per image that
adds to both matrices where they are."""
import math

import torch
import torch.nn.functional as F

from .. import _hip

_scratch = {}  # device -> uint8 tensor of the general path (d above the fused cap); grows, never shrinks


def boundary_dilation(h, w, ratio=0.02):
    """d of an h x w map: max(1, round(0.02 * diagonal)), Python's round (half to even) like the reference's."""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def fused_cap():
    """Largest d the fused kernel serves; a larger one goes through the row / column passes and a scratch buffer."""
    return int(_hip.call_nostream("u2_semseg_boundary_fused_cap"))


def erode_host(m, d):
    """[h, w] uint8 -> the (2 d + 1)-square minimum with zeros outside the image."""
    h, w = m.shape
    if 2 * d + 1 > 2 * max(h, w) + 1:  # every window leaves the image; also keeps the padding within what F.pad allows
        return torch.zeros_like(m)
    x = F.pad(m.to(torch.float32)[None, None], (d, d, d, d), value=0.0)
    x = F.max_pool2d(-x, (1, 2 * d + 1), 1)  # the square minimum, along the rows and then along the columns
    return (-F.max_pool2d(x, (2 * d + 1, 1), 1))[0, 0].to(torch.uint8)


def _checked(pred, gt, lut, d, n):
    if pred.dim() != 2 or pred.shape != gt.shape or pred.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise ValueError("pred %s %s and gt %s %s: expected two [h, w] uint8 maps of one size"
                         % (tuple(pred.shape), pred.dtype, tuple(gt.shape), gt.dtype))
    if pred.numel() == 0:
        raise ValueError("empty label maps")
    if lut is not None and (lut.dtype != torch.uint8 or lut.numel() != 256):
        raise ValueError("lut: expected 256 uint8 entries")
    if d < 1 or not 1 <= n <= 32:
        raise ValueError("d = %d, n = %d: expected d >= 1 and 1 <= n <= 32" % (d, n))


def boundary_confusion_host(pred, gt, lut, d, n):
    """pred, gt: [h, w] uint8 on any device; lut: 256 uint8 entries applied to pred before the erosion, or None.
    Returns (conf, bconf), int64 [n, n] on that device.  Every mapped label must be < n."""
    _checked(pred, gt, lut, d, n)
    if lut is not None:
        pred = lut.to(pred.device).reshape(-1)[pred.long()]
    if int(pred.max()) >= n or int(gt.max()) >= n:
        raise ValueError("a label >= n = %d" % n)
    b_pred, b_gt = pred - erode_host(pred, d), gt - erode_host(gt, d)
    conf = torch.bincount(n * pred.reshape(-1).long() + gt.reshape(-1).long(), minlength=n * n).view(n, n)
    bconf = torch.bincount(n * b_pred.reshape(-1).long() + b_gt.reshape(-1).long(), minlength=n * n).view(n, n)
    return conf, bconf


def boundary_confusion_device(pred, gt, lut, d, n, conf, bconf):
    """The launch: conf (or None) and bconf, int64 [n, n] on the maps' GPU, are added to in place."""
    _checked(pred, gt, lut, d, n)
    dev = pred.device
    assert pred.is_cuda and gt.device == dev and bconf.device == dev and (conf is None or conf.device == dev)
    assert bconf.dtype == torch.int64 and bconf.is_contiguous() and bconf.numel() == n * n
    assert conf is None or (conf.dtype == torch.int64 and conf.is_contiguous() and conf.numel() == n * n)
    assert lut is None or lut.device == dev
    h, w = pred.shape
    pred, gt = pred.contiguous(), gt.contiguous()
    need = int(_hip.call_nostream("u2_semseg_boundary_scratch_bytes", h, w, d))
    scratch = None
    if need > 0:
        scratch = _scratch.get(dev)
        if scratch is None or scratch.numel() < need:
            scratch = _scratch[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    _hip.call("u2_semseg_boundary_confusion", pred, gt, lut, h, w, d, n, conf, bconf, scratch, need)


def boundary_confusion(pred, gt, lut, d, n, conf, bconf):
    """conf += the plain counts, bconf += the boundary counts of one image, in place; the matrices live on the maps' device.
    GPU maps go to the kernel, CPU maps to the host definition."""
    if pred.is_cuda:
        boundary_confusion_device(pred, gt, lut, d, n, conf, bconf)
        return
    c, b = boundary_confusion_host(pred, gt, lut, d, n)
    if conf is not None:
        conf += c
    bconf += b
