"""Precise BatchNorm statistics before a checkpoint: detectron2's PreciseBN hook (engine/hooks.py:567-636, built by
engine/defaults.py:428-452) over fvcore.nn.precise_bn.update_bn_stats.

PARITY UNPINNED: the reference pins fvcore>=0.1.5,<0.1.6 (setup.py:186) and no copy of its precise_bn.py was available when this
was written.  The estimator below is fvcore 0.1.5's population-variance form as documented for it: every training-mode BN layer
at momentum 1.0, per forward with b = N * H * W elements per channel of the layer's input,
    tot += b;  pop_mean += (mean - pop_mean) * b / tot;  pop_sq += (mean^2 + var * (b - 1) / b - pop_sq) * b / tot
and finally running_mean = pop_mean, running_var = pop_sq - pop_mean^2 (no Bessel factor).  Here it is accumulated in the
equivalent closed form, in fp64 on the device (u2_bn_precise_update / u2_bn_precise_finalize, csrc/norm.hip):
    A = sum b * mean,  Q = sum b * mean^2 + (b - 1) * var,  T = sum b;  mean = A / T,  var = Q / T - mean^2.
fvcore accumulates in the buffers' fp32; the fp64 sums are more precise, not bit-equal.

The statistics pass runs the backbone (ResNet + FPN) only: the RPN, ROI heads and semantic head hold no BatchNorm in any shipped
config and do not change what the backbone's layers see."""
import itertools

import torch

from .. import _hip
from ..layers.modules import BatchNorm2d


def get_bn_modules(model):
    """fvcore.nn.precise_bn.get_bn_modules for this project's layers: the BatchNorm2d instances in training mode (SyncBN and "BN";
    FrozenBN and GroupNorm hold no running statistics to update)."""
    return [m for m in model.modules() if isinstance(m, BatchNorm2d) and m.training]


def precise_bn_due(iteration, max_iter, period):
    """The PreciseBN hook's schedule (engine/hooks.py:608-613) for the 0-based `iteration` that has just finished: the last one,
    and with period > 0 every one where iteration + 1 is a multiple of it.  Nothing at or past max_iter (a resumed run that has
    already finished)."""
    if iteration >= max_iter:
        return False
    nxt = iteration + 1
    return nxt == max_iter or (period > 0 and nxt % period == 0)


def _stride(conv):
    s = conv.stride
    if not isinstance(s, int):
        assert s[0] == s[1], "square strides only"
        s = s[0]
    return s


def _resnet_strides(resnet, out):
    """Output stride of every norm layer of a ResNet (modeling/backbone.py), keyed by id(norm)."""
    stem = resnet.stem
    out[id(stem.conv1.norm)] = _stride(stem.conv1)
    s = stem.stride  # after the stem's max pool
    for stage in resnet.stages:
        for blk in stage:
            if blk.shortcut is not None:
                out[id(blk.shortcut.norm)] = s * _stride(blk.shortcut)
            for conv in (blk.conv1, blk.conv2, blk.conv3):
                s *= _stride(conv)
                out[id(conv.norm)] = s


def _backbone_strides(backbone):
    out = {}
    if hasattr(backbone, "top_down") and hasattr(backbone, "bottom_up"):  # FPN over a ResNet
        _resnet_strides(backbone.bottom_up, out)
        shapes = backbone.bottom_up.output_shape()
        for _level, feature, lateral, output in backbone.top_down:
            out[id(lateral.norm)] = out[id(output.norm)] = shapes[feature].stride
    elif hasattr(backbone, "stem") and hasattr(backbone, "stages"):
        _resnet_strides(backbone, out)
    return out


class _LayerTable:
    """The device table (include/u2seg_hip.h U2PreciseBnLayer: two pointers, offset, channels, stride, reserved - 32 bytes a row)
    and the fp64 accumulators of one pass."""

    def __init__(self, layers, strides, device):
        rows, off = [], 0
        for bn, s in zip(layers, strides):
            for t in (bn.running_mean, bn.running_var):
                assert t.dtype == torch.float32 and t.is_contiguous() and t.device == device and t.numel() == bn.num_features
            assert s >= 1
            rows.append([bn.running_mean.data_ptr(), bn.running_var.data_ptr(), off | (bn.num_features << 32), s])
            off += bn.num_features
        self.n_layers, self.channels = len(rows), off
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)  # once per pass
        self.acc = torch.zeros(2 * off, dtype=torch.float64, device=device)
        self.tot = torch.zeros(len(rows), dtype=torch.float64, device=device)

    def update(self, n, h, w):
        _hip.call("u2_bn_precise_update", self.table, self.n_layers, self.acc, self.tot, self.channels, n, h, w)

    def finalize(self):
        _hip.call("u2_bn_precise_finalize", self.table, self.n_layers, self.acc, self.tot, self.channels)


def update_bn_stats(model, batches, num_iters=200):
    """fvcore.nn.precise_bn.update_bn_stats: recompute the running statistics of every training-mode BatchNorm layer of `model` as
    the population statistics of `num_iters` batches drawn from `batches` (an iterable of batched inputs; an iterator is consumed
    where it stands, so a second call continues it).  Runs under no_grad with the layers' momentum at 1.0 (restored afterwards);
    one u2_bn_precise_update launch per batch and one u2_bn_precise_finalize at the end.  Parameters, gradients and optimizer
    state are not touched; each layer's num_batches_tracked rises by num_iters (one training forward each)."""
    bn_layers = get_bn_modules(model)
    if not bn_layers:
        return
    backbone = getattr(model, "backbone", None)
    if backbone is None or not hasattr(model, "_backbone_features"):
        raise NotImplementedError("precise BN runs the backbone of a PanopticFPN-style model (model._backbone_features)")
    strides = _backbone_strides(backbone)
    names = {id(m): n for n, m in model.named_modules()}
    for bn in bn_layers:
        if id(bn) not in strides:
            raise NotImplementedError("precise BN: training-mode BatchNorm %r lies outside the ResNet / FPN backbone; its statistics "
                                      "would need the full forward pass" % names.get(id(bn), "?"))
    device = bn_layers[0].running_mean.device
    table = _LayerTable(bn_layers, [strides[id(bn)] for bn in bn_layers], device)
    momenta = [bn.momentum for bn in bn_layers]
    out_strides = {name: spec.stride for name, spec in backbone.output_shape().items()}
    consumed = 0
    try:
        for bn in bn_layers:
            bn.momentum = 1.0  # running_mean / running_var hold the batch's mean and unbiased variance after each forward
        with torch.no_grad():
            for batch in itertools.islice(batches, num_iters):
                features, _sizes, (h, w) = model._backbone_features(batch)
                n = len(batch)
                for name, f in features.items():  # the canvas the strides are counted from (shapes only: no device work)
                    s = out_strides[name]
                    assert tuple(f.shape[:3]) == (n, -(-h // s), -(-w // s)), (name, tuple(f.shape), (n, h, w))
                del features
                table.update(n, h, w)
                consumed += 1
        assert consumed == num_iters, "Data loader only produced {} batches, but {} batches were expected.".format(
            consumed, num_iters)
        table.finalize()
    finally:
        for bn, m in zip(bn_layers, momenta):
            bn.momentum = m
    for bn in bn_layers:
        bn._updates += 1  # the raw-pointer writes do not bump `_version`: the eval fold cache (Conv2d._folded_eval) keys on this
