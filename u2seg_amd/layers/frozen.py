"""Training through a FrozenBatchNorm2d (layers/batch_norm.py:13-100 of the reference): conv -> fixed affine map (-> + residual)
(-> ReLU) with the arithmetic of the folded inference path.

  W' = bf16(fp32(w) * s[co])                                  one launch per step writes both kernel layouts of every such layer
  out = bf16(relu?(sum x W' + t))                             bias and clamp in the conv epilogue, one rounding
  out = bf16(relu?(bf16(sum x W' + t) + r))                   with a residual r: the accumulating epilogue's two roundings, as one
                                                              extra pass (u2_affine_act with scale 1, shift 0) so that r survives
  dz = g [out > 0],  dr = dz,  dx = dgrad(dz, W'),  dw[co] = s[co] * dW'[co]   (u2_frozen_wgrad_scale_add)

The norm's four buffers get no gradient and the shift t no bias-gradient work.

Cost against the unfrozen path, not parity: a 1x1 layer there adds its weight gradient straight into the arena slot
(conv_launch.wgrad_into); here every layer, 1x1 included, pays zeroed kernel-layout scratch, u2_conv_wgrad into it
(conv_launch.wgrad_scratch) and one more weight-sized pass for the scaled add (52 launches, about 1.3 ms per step on the side
stream for a ResNet-50)."""
import weakref

import numpy as np
import torch
from torch.autograd import Function

from .. import _hip
from . import conv_launch
from .streams import _conv_variant, _run_wgrad
from .weights import BF16, _check_act, ceil32, grad_slot, zeros_f32

# include/u2seg_hip.h U2FrozenFoldDesc: four pointers, N, Cin, T, Cp, Npad, block_begin, two reserved ints - 64 bytes a row
_DESC = np.dtype([("w", "<u8"), ("s", "<u8"), ("fwd", "<u8"), ("dgrad", "<u8"), ("N", "<i4"), ("Cin", "<i4"), ("T", "<i4"),
                  ("Cp", "<i4"), ("Npad", "<i4"), ("blk", "<i4"), ("r0", "<i4"), ("r1", "<i4")])
assert _DESC.itemsize == 64

_registry = []       # weakrefs of every live _FoldEntry, in the order the layers were first run
_table_cache = {}    # device -> (key, device table, blocks): rebuilt only when the set of layers to fold or a pointer changes
_unit = {}           # (device, c) -> (ones, zeros) fp32


def scale_shift(norm):
    """norm.eval_scale_shift() as contiguous fp32 vectors, kept until one of the norm's buffers changes (four small torch launches
    per layer and pass otherwise).  The buffers of a FrozenBatchNorm2d only change through torch: version counters see it."""
    bufs = (norm.weight, norm.bias, norm.running_mean, norm.running_var)
    key = tuple((t._version, t.data_ptr()) for t in bufs) + (norm.eps,)
    hit = norm.__dict__.get("_u2_scale_shift")
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        s, t = norm.eval_scale_shift()
        val = (s.float().contiguous(), t.float().contiguous())
    norm.__dict__["_u2_scale_shift"] = (key, val)
    return val


class _FoldEntry:
    """The two bf16 layouts of one layer's W' and what they were made from."""

    __slots__ = ("weight", "norm", "dims", "fwd", "dgrad", "ss", "key", "stream", "__weakref__")

    def current_key(self):
        w = self.weight
        st = getattr(w, "_u2_stamp", None)   # the optimizer writes through raw pointers: its step stamp is part of the key
        return (w._version, w.data_ptr(), st[0] if st is not None else 0)

    def stale(self):
        return self.key != self.current_key() or self.ss is not scale_shift(self.norm)


def _fold(entries, device):
    """One u2_frozen_fold launch for `entries`."""
    for e in entries:
        e.ss = scale_shift(e.norm)
    key = tuple((id(e), e.weight.data_ptr(), e.ss[0].data_ptr(), e.fwd.data_ptr(), e.dgrad.data_ptr()) for e in entries)
    hit = _table_cache.get(device)
    if hit is None or hit[0] != key:
        desc = np.zeros(len(entries), dtype=_DESC)
        blocks = 0
        for i, e in enumerate(entries):
            n, cin, t, cp, npad = e.dims
            desc[i] = (key[i][1], key[i][2], key[i][3], key[i][4], n, cin, t, cp, npad, blocks, 0, 0)
            blocks += ((npad + 63) // 64) * ((cin * t + 63) // 64)
        table = torch.from_numpy(desc.view(np.uint8).copy()).to(device)
        hit = _table_cache[device] = (key, table, blocks)
    _hip.call("u2_frozen_fold", hit[1], len(entries), hit[2])
    for e in entries:
        e.key = e.current_key()


def folded_layouts(conv, cp):
    """(forward layout [N][T][cp], data-gradient layout [cp][T][Npad], s, t) of conv + its FrozenBatchNorm2d for inputs of cp
    physical channels.  When this layer's layouts are out of date, every layer's that is (the optimizer has stepped: all of them)
    is rewritten by the same launch."""
    w = conv.weight
    n, cin, kh, kw = w.shape
    dims = (n, cin, kh * kw, cp, ceil32(n))
    stream = _hip.stream_ptr()
    e = conv.__dict__.get("_u2_frozen_fold")
    if e is None or e.dims != dims or e.weight is not w or e.norm is not conv.norm or e.fwd.device != w.device:
        assert cin <= cp and cp % 2 == 0 and w.dtype == torch.float32 and w.is_contiguous()
        e = _FoldEntry()
        e.weight, e.norm, e.dims, e.key, e.ss, e.stream = w, conv.norm, dims, None, None, stream
        # zeroed once: the fold never writes the rows of input channels cin..cp-1
        e.fwd = torch.zeros((n, dims[2], cp), dtype=BF16, device=w.device)
        e.dgrad = torch.zeros((cp, dims[2], dims[4]), dtype=BF16, device=w.device)
        conv.__dict__["_u2_frozen_fold"] = e
        _registry.append(weakref.ref(e))
    if e.stream != stream or e.stale():
        e.stream = stream
        # the layers folded along: alive, on this device, last run on this stream (a layout must not be rewritten under a
        # stream that may still read it)
        batch, alive = [], []
        for ref in _registry:
            o = ref()
            if o is None:
                continue
            alive.append(ref)
            if o is e or (o.stream == stream and o.fwd.device == w.device and o.stale()):
                batch.append(o)
        _registry[:] = alive
        _fold(batch, w.device)
    return e.fwd, e.dgrad, e.ss[0], e.ss[1]


def _unit_affine(c, device):
    hit = _unit.get((device, c))
    if hit is None:
        hit = _unit[(device, c)] = (torch.ones(c, dtype=torch.float32, device=device), torch.zeros(c, dtype=torch.float32, device=device))
    return hit


class _FrozenConvFn(Function):
    @staticmethod
    def forward(ctx, x, weight, residual, s, t, wk, wd, stride, pad, relu, slot_box):
        _check_act(x)
        g = ctx.geom = conv_launch.ConvGeom.of(x.shape, weight.shape, stride, pad)
        out = conv_launch.alloc_out(g, x.device)
        ctx.variant = _conv_variant()
        conv_launch.forward(g, x, wk, out, t, None, relu and residual is None, 0, ctx.variant)
        if residual is not None:
            _check_act(residual)
            assert tuple(residual.shape) == tuple(out.shape), (tuple(residual.shape), tuple(out.shape))
            one, zero = _unit_affine(g.npad, x.device)
            y, out = out, torch.empty_like(out)
            _hip.call("u2_affine_act", y, one, zero, residual, out, 1, g.m_out, g.npad, g.npad, int(relu), None)
        ctx.save_for_backward(x, out if relu else None)
        ctx.relu = relu
        # the layouts and the scale as this pass used them (rewritten in place only after the optimizer has stepped)
        ctx.wd, ctx.s = wd, s
        slot = slot_box[0]
        ok = slot is not None and slot.is_contiguous() and slot.dtype == torch.float32 and slot.numel() == weight.numel()
        ctx.slot = slot if ok else None
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * 11
        x, out = ctx.saved_tensors
        geom = ctx.geom
        need_dx, need_dw, need_dr = ctx.needs_input_grad[:3]
        g = g.contiguous()
        dz = g
        if ctx.relu:
            dz = torch.empty_like(g)
            _hip.call("u2_relu_bwd", g, out, dz, g.numel())
        dx = None
        if need_dx:
            dx = torch.empty_like(x)
            conv_launch.dgrad(geom, dz, ctx.wd, dx, ctx.variant)
        dw = None
        if need_dw:
            s = ctx.s

            def accumulate(dst):   # dst += s * dW', dW' in the kernel's layout in scratch zeroed by the pool of the stream this runs on
                dwk = zeros_f32((geom.npad, geom.taps, geom.cp), x.device)
                conv_launch.wgrad_scratch(geom, x, dz, dwk)
                _hip.call("u2_frozen_wgrad_scale_add", dwk, s, dst, geom.n, geom.cin, geom.taps, geom.cp)

            if ctx.slot is not None:
                slot = ctx.slot
                _run_wgrad(x.device, (x, dz), lambda: accumulate(slot))
            else:
                dw = torch.zeros((geom.n, geom.cin, geom.kh, geom.kw), dtype=torch.float32, device=x.device)
                accumulate(dw)
        return (dx, dw, dz if need_dr else None) + (None,) * 8


def frozen_conv2d(conv, x, residual=None, relu=False):
    """conv (a layers.modules.Conv2d whose norm is a FrozenBatchNorm2d) on x, under autograd."""
    stride, pad = conv.stride, conv.padding
    assert isinstance(stride, int) and isinstance(pad, int)
    if conv.groups != 1:
        # a grouped 3x3 layer: the u2_gconv3x3_* kernels apply s themselves (W' = bf16(w * s) as they stage it, dw = s * dW' as
        # they add it): no entry in the fold table, no scaled-add pass
        from .functional import grouped_conv2d   # (functional imports this module by name: the import cannot stand at the top)

        assert residual is None, "a grouped layer takes no residual"
        s, t = scale_shift(conv.norm)
        return grouped_conv2d(x, conv.weight, t, conv.groups, stride, pad, relu=bool(relu), scale=s, round_bias=False)[0]
    wk, wd, s, t = folded_layouts(conv, x.shape[3])
    return _FrozenConvFn.apply(x, conv.weight, residual, s, t, wk, wd, stride, pad, bool(relu), (grad_slot(conv.weight),))


class _AffineReluMaxPoolFn(Function):
    """The stem's tail behind a FrozenBatchNorm2d under autograd: max_pool_3x3_s2(relu(y * s + t)) in one pass each way.  The
    backward pass is the batch-norm form's apply step (dx = k1 dz + k2 y + k3, ReLU mask recomputed from y * s + t > 0) with
    k1 = s and k2 = k3 = 0: the gradient of a fixed affine map."""

    @staticmethod
    def forward(ctx, y, scale, shift):
        _check_act(y)
        b, h, w, c = y.shape
        ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        out = torch.empty((b, ho, wo, c), dtype=BF16, device=y.device)
        idx = torch.empty((b, ho, wo, c), dtype=torch.uint8, device=y.device)
        _hip.call("u2_affine_relu_maxpool_fwd", y, scale, shift, out, idx, b, h, w, c)
        ctx.save_for_backward(y, idx, scale, shift)
        return out

    @staticmethod
    def backward(ctx, dy):
        y, idx, scale, shift = ctx.saved_tensors
        b, h, w, c = y.shape
        zero = _unit_affine(c, y.device)[1]
        dx = torch.empty_like(y)
        _hip.call("u2_affine_relu_maxpool_bwd_apply", dy.contiguous(), idx, y, scale, zero, zero, scale, shift, dx, b, h, w, c)
        return dx, None, None


def affine_relu_max_pool_train(y, scale, shift):
    return _AffineReluMaxPoolFn.apply(y, scale.contiguous(), shift.contiguous())
