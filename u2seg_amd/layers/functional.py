"""torch.autograd.Function wrappers over the C-ABI HIP launchers (include/u2seg_hip.h).

Activations are NHWC bfloat16 tensors ``[B, H, W, C]`` whose physical channel count is a multiple
of 32 (logical channel counts such as 28 / 3 / 12 / 801 / 4 are zero padded on the right and the
consumer is told the logical width).  Parameters stay fp32 in the reference layout
(``[Cout, Cin, kh, kw]``, state-dict compatible with detectron2) and are re-laid-out to the kernel
layout (``[Cout][kh*kw][Cin]`` bf16) on the fly.

Every function here launches HIP kernels; none has a CPU or ATen compute fallback.

This module holds the differentiable layers whose backward passes talk to each other through layers/deferred.py (conv, stem,
norms, pooling, resampling, fan-out, ROIAlign) and is the one name the rest of the package calls the layers by: the zero pool and
the weight layouts (weights.py), the streams (streams.py), the head losses (losses.py), the selection wrappers (select.py) and
the FrozenBN training path (frozen.py) are imported here by name.  Functions are re-exported, mutable state never: a switch lives in exactly one module.
A convolution's shapes and the argument lists of its launches are written once, in conv_launch.py (used here and in frozen.py, not re-exported).
"""
import collections
import ctypes
import functools
import os

import torch
import torch.distributed as dist
from torch.autograd import Function

from .. import _hip
from . import conv_launch, deferred, streams
from .frozen import affine_relu_max_pool_train, frozen_conv2d  # noqa: F401
from .losses import (BOX_REG_LOSS_KINDS, box_reg_l1_loss, box_reg_loss, box_reg_loss_cls, count_labels_i8, mask_predict_bce_loss,  # noqa: F401
                     mask_predict_prob, rpn_losses, sem_seg_loss, sigmoid_cross_entropy, softmax_cross_entropy)
from .select import (_TOPK_MAX_K, _topk_rows_sorted, _topk_segments, apply_deltas, apply_deltas_cls, assign_levels, batched_nms,  # noqa: F401
                     iou_match, mask_crop, rpn_decode, sem_seg_upsample, topk_rows, topk_rows_multi)
from .streams import (_NO_STREAMK, _conv_variant, _run_wgrad, _world, aux_stream, clear_branch_pieces,  # noqa: F401
                      flush_branch_pieces, issue_branch_piece, join_all_streams, join_aux_stream, join_wgrad_stream,
                      producer_streams, queue_branch_pieces, set_stream_overlap, streamk_region)
from .weights import (BF16, _check_act, _conv_bias, _weight_layout, ceil32, grad_slot, release_library_scratch,  # noqa: F401
                      weight_dgrad_layout, weight_fc_dgrad_layout, weight_fwd_layout, zeros_f32)

# --------------------------------------------------------------------------------------------
# switches (tests and A/B runs assign them on this module; they are read at call time)
# --------------------------------------------------------------------------------------------
_DET_STATS = False   # set_deterministic_stats()
STEM_TAIL_FUSE = os.environ.get("U2_STEM_TAIL_FUSE", "1") != "0"   # the stem's norm -> ReLU -> max pool as one pass (stem_tail_ok)
STEM_DIRECT = os.environ.get("U2_STEM_DIRECT", "1") != "0"   # the stem conv and its weight gradient without the im2col matrix
FUSED_BWD_MIN_PIXELS = int(os.environ.get("U2_FUSED_BWD_MIN_PIXELS", "200000"))
# Three backward folds hand autograd a zero placeholder and leave the gradient to the node that receives it (layers/deferred.py):
# - the batch-norm backward apply step of an expanding 1x1 layer evaluated inside that layer's fused backward launch (0: separate)
LAZY_BN_APPLY = os.environ.get("U2_LAZY_BN_APPLY", "1") != "0"
# - the ROIAlign gather of a tapped FPN map deferred to the map's _FanOutFn.backward (round 6); U2_ROI_SUM_FOLD=0: the tap gathers
#   on the spot and u2_add_n sums afterwards
ROI_SUM_FOLD = os.environ.get("U2_ROI_SUM_FOLD", "1") != "0"
# - the backward reduce of a residual block's tail folded into the next block's conv1 data gradient (u2_conv_dgrad_tail;
#   U2_TAIL_BWD_FUSE=0: two launches).  The placeholder runs in the other direction here: the conv hands autograd a placeholder for
#   its input gradient, and the tail's backward, which receives it, finds (dz, sums) in its own state.
TAIL_BWD_FUSE = os.environ.get("U2_TAIL_BWD_FUSE", "1") != "0"
_TAIL_SHAPES = ((64, 256), (128, 512), (256, 1024))   # (conv1 output channels, block width) the kernel serves
ROI_ORDER_MIN = int(os.environ.get("U2_ROI_ORDER_MIN", "1000000000"))   # ROI count from which the ROIAlign forward sorts its rows
ROI_ALIGN_BWD_ATOMIC = False  # True selects the fp32-atomic scatter variant (kept for A/B tests)
_UP2_BWD_LAST = None   # (key, dout, dx) of the semantic head's shared upsample gradient (_BilinearUp2Fn.backward)


def set_deterministic_stats(on):
    """Test switch: the BN column statistics that the conv epilogue accumulates with fp32 atomics (their order varies from
    run to run, so the forward pass differs in the last bits between runs) are taken from the stored output by a fixed-order
    reduction instead.  Free-running comparisons (tests/test_gpu_parity.py) use it to be reproducible."""
    global _DET_STATS
    _DET_STATS = bool(on)


def set_tail_bwd_fuse(on):
    """Run-time form of U2_TAIL_BWD_FUSE (tests, A/B runs); applies to graphs built afterwards."""
    global TAIL_BWD_FUSE
    TAIL_BWD_FUSE = bool(on)


# --------------------------------------------------------------------------------------------
# convolution / linear
# --------------------------------------------------------------------------------------------
def _fixed_order_stats(out, n):
    o = out[..., :n].float().reshape(-1, n)
    packed = torch.cat([o.sum(0), (o * o).sum(0), o.new_zeros(1)])
    st = packed[: 2 * n].view(2, n)
    st._u2_packed = packed
    return st


def _stats_buffer(n, device):
    """[sum | sum of squares] of a conv output's channels as a view of a zeroed [2n + 1] buffer: under SyncBN the extra slot
    takes this rank's element count and the whole buffer is all-reduced as it stands (no concatenation, no host round trip).
    The buffer is CONSUMED by batch_norm_act under SyncBN: after it the `stats` a caller still holds are the sums over all ranks,
    not this rank's (the only consumer in this package is the norm that follows the conv; clone before the norm if both are needed)."""
    packed = zeros_f32((2 * n + 1,), device)
    st = packed[: 2 * n].view(2, n)
    st._u2_packed = packed
    return st


class _Conv2dFn(Function):
    """F.conv2d (+bias)(+ReLU) with optional per-channel sum / sum-of-squares of the output
    (reference: detectron2/layers/wrappers.py:127-134)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, relu, want_stats, param_ref=None, round_bias=True, tail=None):
        _check_act(x)
        ctx.tail = tail   # x is a residual block's output whose tail reduce this layer's data gradient may take over (_TailState)
        # boxed so that autograd does not treat them as inputs: the owning Parameter and its arena gradient slice (looked up by
        # conv2d() - Function.forward runs with autograd disabled, where grad_slot() answers None)
        param = param_ref[0] if param_ref is not None else None
        wgrad_dst = param_ref[1] if param_ref is not None and len(param_ref) > 1 else None
        g = conv_launch.ConvGeom.of(x.shape, weight.shape, stride, pad)
        n = g.n
        assert g.cin <= g.cp
        wk = weight_fwd_layout(weight, g.cp, param)
        out = conv_launch.alloc_out(g, x.device)
        stats = _stats_buffer(n, x.device) if want_stats else None
        # autocast casts every floating-point argument of a convolution, the bias included (pinned by the reference run under
        # bf16 autocast, tests/golden/bf16_units_golden.npz); a folded eval-mode norm shift is not a conv bias and stays fp32
        bias_f = None
        if bias is not None:
            bias_f = _conv_bias(bias, round_bias)
        ctx.variant = _conv_variant()
        conv_launch.forward(g, x, wk, out, bias_f, None if _DET_STATS else stats, relu, 0, ctx.variant)
        if want_stats and _DET_STATS:
            stats = _fixed_order_stats(out, n)
        ctx.save_for_backward(x, weight, out if relu else None)
        ctx.cfg = (stride, pad, relu, bias is not None)
        # 1x1 / linear weights: the gradient is accumulated straight into the optimizer's arena slice
        ctx.wgrad_dst = wgrad_dst if (g.taps == 1 and wgrad_dst is not None) else None
        # the arena slice in the parameter's own [N, Cin, KH, KW] shape (multi-tap filters accumulate into it with a torch add)
        # (a reshaped view of the parameter - the box head's fc1 as a 7x7 conv - gets the slice in the view's shape)
        ctx.arena = None
        if wgrad_dst is not None and wgrad_dst.numel() == weight.numel() and wgrad_dst.is_contiguous():
            ctx.arena = wgrad_dst if tuple(wgrad_dst.shape) == tuple(weight.shape) else wgrad_dst.view(weight.shape)
        ctx.param = param
        # the bias gradient goes straight into the bias' arena slice as well (u2_colsum_add), if the kernels can add into it
        bdst = param_ref[2] if param_ref is not None and len(param_ref) > 2 and bias is not None else None
        ctx.bias_dst = bdst if bdst is not None and bdst.is_contiguous() and bdst.dtype == torch.float32 and bdst.numel() == n else None
        ctx.set_materialize_grads(False)  # no zero tensor for the (non-differentiable) statistics output
        if want_stats:
            ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        if dout is None:
            return (None,) * 10
        x, weight, out = ctx.saved_tensors
        stride, pad, relu, has_bias = ctx.cfg
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        geom = conv_launch.ConvGeom.of(x.shape, weight.shape, stride, pad)   # the shapes, derived once for all helpers
        lazy = deferred.take(deferred.BN_APPLY, dout)
        if lazy is not None:   # the gradient is still (dz, y, coefficients) of the batch normalisation behind this layer
            dx, dout = _conv_bwd_lazy_bn(ctx, geom, x, weight, *lazy)
            if dx is not None:
                return (dx,) + (None,) * 9
        dout = dout.contiguous()
        dz, bias_done = _conv_bwd_relu(ctx, geom, dout, out) if relu else (dout, False)
        dx, fused = _conv_bwd_data(ctx, geom, x, weight, dz) if need_dx else (None, False)
        dw = _conv_bwd_weight(ctx, geom, x, weight, dz) if need_dw and not fused else None
        db = _conv_bwd_bias(ctx, geom, dz) if has_bias and need_db and not bias_done else None
        return (dx, dw, db) + (None,) * 7


def _conv_bwd_lazy_bn(ctx, g, x, weight, lz_dz, lz_y, lz_k):
    """The norm behind the layer left its apply step dout = k1 dz + k2 y + k3 (lz_k rows 2-4) to this backward: (dx, None) when one
    launch formed both gradients from the operands, else (None, dout) - the step as its own launch, then the usual paths."""
    m, cp, npad = g.m_in, g.cp, g.npad
    assert not ctx.cfg[2] and not ctx.cfg[3] and g.is_1x1_unit
    wd = weight_dgrad_layout(weight, cp, npad, ctx.param)
    dx = torch.empty_like(x)
    if ctx.wgrad_dst is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and _hip.call_status(
            "u2_conv1x1_bwd_fused_bn", x, lz_dz, lz_y, lz_k[2], lz_k[3], lz_k[4], wd, dx, ctx.wgrad_dst, m, cp, cp, npad, npad,
            npad, cp, g.n, g.cin, g.cin, 1, 0) == 0:
        return dx, None
    dout = torch.empty_like(lz_y)   # not served after all
    _hip.call("u2_norm_bwd_apply", lz_dz, None, lz_y, lz_k[2], lz_k[3], lz_k[4], dout, None, 1, m, npad, npad, 0, None, None)
    return None, dout


def _conv_bwd_relu(ctx, g, dout, out):
    """ReLU backward -> (dz, whether the bias gradient was added to its arena slice in the same pass over dout / out)"""
    dz = torch.empty_like(dout)
    if ctx.bias_dst is not None and ctx.needs_input_grad[2]:
        _hip.call("u2_relu_bwd_colsum", dout, out, dz, ctx.bias_dst, zeros_f32((g.npad,), dout.device), g.m_out, g.npad, g.npad, g.n)
        return dz, True
    _hip.call("u2_relu_bwd", dout, out, dz, g.m_out * g.npad)
    return dz, False


def _conv_bwd_data(ctx, g, x, weight, dz):
    """-> (dx, whether the launch that formed it accumulated the weight gradient as well)"""
    cp, npad = g.cp, g.npad
    dst = ctx.wgrad_dst
    if dst is not None and ctx.needs_input_grad[1] and g.is_1x1_unit and g.n > 128 and g.m_in >= FUSED_BWD_MIN_PIXELS:
        # both gradients of an expanding 1x1 layer in one pass over dz (u2_conv1x1_bwd_fused: dz is the large operand); the
        # launcher answers 1 for a shape it does not serve
        assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.numel() == g.n * g.cin
        wd = weight_dgrad_layout(weight, cp, npad, ctx.param)
        dx = torch.empty_like(x)
        if _hip.call_status("u2_conv1x1_bwd_fused", x, dz, wd, dx, dst, g.m_in, cp, cp, npad, npad, npad, cp, g.n, g.cin, g.cin, 1,
                            0) == 0:
            return dx, True
    # conv1 of a bottleneck behind an identity block: the data gradient g1 is formed, summed with the residual path's gradient,
    # masked and reduced in one launch (u2_conv_dgrad_tail); what autograd carries to the previous block's tail is a placeholder,
    # (dz, sums) wait in the tail's state
    dx = _tail_launch(ctx, g, dz, x, weight)
    if dx is not None:
        return dx, False
    dx = torch.empty_like(x)
    if g.is_fc:
        conv_launch.fc_dgrad(g, dz, weight_fc_dgrad_layout(weight, cp, npad, ctx.param), dx, ctx.variant)
    else:
        conv_launch.dgrad(g, dz, weight_dgrad_layout(weight, cp, npad, ctx.param), dx, ctx.variant)
    return dx, False


def _conv_bwd_weight(ctx, g, x, weight, dz):
    """The weight gradient: accumulated into the optimizer's arena on the side stream (-> None), or returned for autograd."""
    n, cin, kh, kw = g.n, g.cin, g.kh, g.kw
    dst, arena = ctx.wgrad_dst, ctx.arena

    def scratch():   # in the kernel's layout, zeroed by the pool of the stream this runs on
        dwk = zeros_f32((g.npad, g.taps, g.cp), x.device)
        conv_launch.wgrad_scratch(g, x, dz, dwk)
        return dwk

    if dst is not None:
        assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.numel() == n * cin

        def launch():
            conv_launch.wgrad_into(g, x, dz, dst)
    elif arena is not None and streams._WGRAD_SIDE:
        # multi-tap filters: kernel-layout scratch, then accumulated into the arena slice by one transposing kernel (the strided
        # torch add took 70-170 us per 3x3 layer, 1.3 ms per step) - all of it on the side stream
        def launch():
            dwk = scratch()
            if g.taps * (g.cp + 1) * 4 <= 64 * 1024 and arena.is_contiguous():
                _hip.call("u2_wgrad_permute_add", dwk, arena, n, cin, g.taps, g.cp)
            else:
                arena.add_(dwk[:n, :, :cin].view(n, kh, kw, cin).permute(0, 3, 1, 2))
    else:
        return scratch()[:n, :, :cin].view(n, kh, kw, cin).permute(0, 3, 1, 2)
    _run_wgrad(x.device, (x, dz), launch)
    return None


def _conv_bwd_bias(ctx, g, dz):
    """The bias gradient: added into the bias' arena slice (-> None), or returned for autograd."""
    if ctx.bias_dst is not None:
        _hip.call("u2_colsum_add", dz, ctx.bias_dst, g.m_out, g.npad, g.npad, g.n)
        return None
    sums = zeros_f32((1, 2, g.npad), dz.device)
    _hip.call("u2_colstats", dz, sums, 1, g.m_out, g.npad, g.npad)
    return sums[0, 0, :g.n]


def _tail_launch(ctx, g, dz, x, weight):
    """_conv_bwd_data: launch the fused data gradient + tail reduce if this layer was marked for it in the forward pass, the
    other consumer's gradient has been posted and the kernel serves the shape; returns the placeholder autograd carries instead of
    dx.  None: the caller takes the two launches."""
    tail = ctx.tail
    if tail is None or not TAIL_BWD_FUSE or tail.g2 is None or tail.result is not None:
        return None
    n, cp = g.n, g.cp
    if ctx.cfg[2] or not g.is_1x1_unit or tuple(tail.g2.shape) != tuple(x.shape) \
            or tuple(tail.y.shape) != tuple(x.shape) or not tail.g2.is_contiguous() or g.npad != n:
        return None
    wd = weight_dgrad_layout(weight, cp, n, ctx.param)
    dzt = torch.empty_like(tail.y)
    sums = zeros_f32((2, cp), x.device)
    if _hip.call_status("u2_conv_dgrad_tail", dz, wd, tail.g2, tail.y, tail.bits, tail.mean, tail.invstd, dzt, sums, g.b, g.h, g.w, n, n,
                        cp, cp, ctx.variant) != 0:
        return None   # declined (shape, fill rule, switched off by the variant bits): nothing was written
    ph = deferred.post(deferred.TAIL, x.device, x.shape, tail)
    tail.result = (dzt, sums)
    return ph


class _GroupedConv2dFn(Function):
    """F.conv2d(groups = G) of a 3x3 / pad-1 layer (+bias)(+ReLU)(+statistics), conv2 of a ResNeXt bottleneck
    (backbone/resnet.py:155-166), on the u2_gconv3x3_* kernels.  They read the fp32 parameter itself and round it while they
    stage it: no kernel layout is looked up, cached or rewritten on this path.  `scale` (fp32 [C], no gradient): the kernels
    compute with W' = bf16(w * scale[n]) and return dw = scale[n] * dW' - the FrozenBN fold (layers/frozen.py) without its table."""

    @staticmethod
    def forward(ctx, x, weight, bias, scale, groups, stride, pad, relu, want_stats, slot_box, round_bias):
        _check_act(x)
        g = ctx.geom = conv_launch.GroupedGeom.of(x.shape, weight.shape, groups, stride, pad)
        assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.device == x.device
        w = weight.detach()
        out = torch.empty((g.b, g.ho, g.wo, g.c), dtype=BF16, device=x.device)
        stats = _stats_buffer(g.c, x.device) if want_stats else None
        bias_f = _conv_bias(bias, round_bias) if bias is not None else None
        conv_launch.grouped_forward(g, x, w, scale, bias_f, out, None if _DET_STATS else stats, relu)
        if want_stats and _DET_STATS:
            stats = _fixed_order_stats(out, g.c)
        ctx.save_for_backward(x, weight, out if relu else None, scale)
        ctx.relu = relu
        slot = slot_box[0] if slot_box is not None else None
        ok = slot is not None and slot.is_contiguous() and slot.dtype == torch.float32 and tuple(slot.shape) == tuple(weight.shape)
        ctx.slot = slot if ok else None
        ctx.set_materialize_grads(False)
        if want_stats:
            ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        if dout is None:
            return (None,) * 11
        x, weight, out, scale = ctx.saved_tensors
        g = ctx.geom
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        # neither deferred-gradient protocol (layers/deferred.py) reaches a 3x3 layer: BN_APPLY is posted to expanding 1x1 layers,
        # TAIL by a 1x1 conv1 - a placeholder arriving here would be a gradient silently dropped
        assert not deferred.holds(deferred.BN_APPLY, dout) and not deferred.holds(deferred.TAIL, dout), \
            "a deferred gradient reached a grouped 3x3 layer"
        dz = dout.contiguous()
        if ctx.relu:
            dz = torch.empty_like(dz)
            _hip.call("u2_relu_bwd", dout.contiguous(), out, dz, dz.numel())
        dx = None
        if need_dx:
            dx = torch.empty_like(x)
            conv_launch.grouped_dgrad(g, dz, weight.detach(), scale, dx)
        dw = None
        if need_dw:
            if ctx.slot is not None:
                slot = ctx.slot
                _run_wgrad(x.device, (x, dz), lambda: conv_launch.grouped_wgrad(g, x, dz, scale, slot))
            else:
                dw = torch.zeros(weight.shape, dtype=torch.float32, device=x.device)
                conv_launch.grouped_wgrad(g, x, dz, scale, dw)
        db = None
        if need_db:
            sums = zeros_f32((1, 2, g.c), dz.device)
            _hip.call("u2_colstats", dz, sums, 1, g.m_out, g.c, g.c)
            db = sums[0, 0]
        return (dx, dw, db) + (None,) * 8


def grouped_conv2d(x, weight, bias, groups, stride, pad, relu=False, want_stats=False, scale=None, round_bias=True):
    """-> (out, stats or None).  `weight`: the fp32 [C, C // groups, 3, 3] tensor the kernels read (a Parameter, or a folded copy)."""
    slot = grad_slot(weight) if isinstance(weight, torch.nn.Parameter) else None
    return _GroupedConv2dFn.apply(x, weight, bias, scale, groups, stride, pad, relu, want_stats, (slot,), round_bias)


def conv2d(x, weight, bias=None, stride=1, pad=0, relu=False, want_stats=False, param=None, round_bias=True, groups=1):
    """`param`: the nn.Parameter that owns `weight`'s memory when `weight` is a reshaped view of it (defaults to `weight`
    itself when that is a Parameter); it carries the optimizer's gradient slot and the cached kernel layouts.
    groups > 1: a grouped 3x3 layer (_GroupedConv2dFn); `param` plays no part there, the kernels read `weight` as it stands."""
    if groups != 1:
        out, stats = grouped_conv2d(x, weight, bias, groups, stride, pad, relu, want_stats, None, round_bias)
        return (out, stats) if want_stats else out
    if param is None and isinstance(weight, torch.nn.Parameter):
        param = weight
    slot = grad_slot(param) if param is not None else None
    bslot = grad_slot(bias) if isinstance(bias, torch.nn.Parameter) else None
    tail = getattr(x, "_u2_tail", None) if TAIL_BWD_FUSE and torch.is_grad_enabled() else None
    if tail is not None and not (bias is None and not relu and stride == 1 and pad == 0 and tuple(weight.shape[2:]) == (1, 1)
                                 and (weight.shape[0], x.shape[3]) in _TAIL_SHAPES and weight.shape[1] == x.shape[3]
                                 and getattr(x, "_u2_twin", None) is not None):
        tail = None   # (a strided or biased consumer, a width the kernel does not serve, the second handle: two launches)
    out, stats = _Conv2dFn.apply(x, weight, bias, stride, pad, relu, want_stats,
                                 (param, slot, bslot) if param is not None else None, round_bias, tail)
    if LAZY_BN_APPLY and want_stats and slot is not None and bias is None and not relu and stride == 1 and pad == 0 \
            and x.requires_grad and tuple(weight.shape[2:]) == (1, 1) and 128 < weight.shape[0] <= 256 and x.shape[3] <= 64 \
            and x.shape[0] * x.shape[1] * x.shape[2] >= FUSED_BWD_MIN_PIXELS:
        # a batch normalisation on this output may leave its backward apply step to this layer's fused backward launch
        out._u2_lazy_ok = True
    return (out, stats) if want_stats else out


def conv2d_add_(x, weight, bias, out, stride=1, pad=0, relu=False, param=None):
    """Inference only, in place: out = act(bf16(conv(x, weight) + bias) + out) - a residual block's tail (conv3 with its
    fixed-statistics norm folded in, + shortcut, + ReLU: backbone/resnet.py:204-210) as ONE launch that reads the shortcut
    where it writes the result.  `out` is overwritten: the caller must own it."""
    assert not torch.is_grad_enabled()
    _check_act(x)
    _check_act(out)
    g = conv_launch.ConvGeom.of(x.shape, weight.shape, stride, pad)
    assert tuple(out.shape) == (g.b, g.ho, g.wo, g.npad) and g.npad == g.n, "the accumulating epilogue has no padded output channels"
    wk = weight_fwd_layout(weight, g.cp, param)
    bias_f = bias.detach().float().contiguous() if bias is not None else None
    conv_launch.forward(g, x, wk, out, bias_f, None, relu, 1, _conv_variant())
    return out


def linear(x2d, weight, bias=None, relu=False):
    """nn.Linear on a [R, K] bf16 matrix (K % 32 == 0); returns [R, ceil32(N)]."""
    r, k = x2d.shape
    n = weight.shape[0]
    param = weight if isinstance(weight, torch.nn.Parameter) else None
    out = conv2d(x2d.view(1, r, 1, k), weight.view(n, weight.shape[1], 1, 1), bias, 1, 0, relu, False, param)
    return out.view(r, -1)


class _StemConvFn(Function):
    """(x - mean)/std, zero pad to the batch canvas, 7x7 stride-2 pad-3 conv of 3 -> 64 channels
    (rcnn.py:223-234 + backbone/resnet.py:355-357). Images need no gradient.

    Production path (STEM_DIRECT): u2_stem_conv_fwd / u2_stem_conv_wgrad read the MFMA operands from the normalised image window in
    LDS; what is kept for the backward pass is the image list.  The im2col GEMM (u2_stem_im2col_batch + u2_conv_igemm, the matrix
    saved for u2_conv_wgrad) serves the calls the direct launcher declines, U2_STEM_DIRECT=0 and the deterministic-statistics mode,
    whose fixed-order pass wants the stem among the recorded u2_conv_igemm launches."""

    KP = 160

    @staticmethod
    def forward(ctx, weight, images, pixel_mean, pixel_std, hpad, wpad):
        n = weight.shape[0]
        b = len(images)
        ho, wo = (hpad + 6 - 7) // 2 + 1, (wpad + 6 - 7) // 2 + 1
        kp = _StemConvFn.KP
        is_u8 = images[0].dtype == torch.uint8
        for img in images:
            assert img.is_cuda and img.is_contiguous() and img.shape[0] == 3
            assert img.dtype == (torch.uint8 if is_u8 else torch.float32), "one pixel type per batch"
        ptrs = (ctypes.c_void_p * b)(*[img.data_ptr() for img in images])
        hs = (ctypes.c_int * b)(*[img.shape[1] for img in images])
        ws = (ctypes.c_int * b)(*[img.shape[2] for img in images])
        # [64, 3, 7, 7] -> K order (kh, kw, c), zero padded to kp: the forward layout of a 49-tap, 3-channel conv flattened
        wk = torch.zeros((n, 1, kp), dtype=BF16, device=weight.device)
        wk[:, 0, :147] = weight.detach().permute(0, 2, 3, 1).reshape(n, 147)
        out = torch.empty((b, ho, wo, n), dtype=BF16, device=weight.device)
        stats = _stats_buffer(n, weight.device)
        m = b * ho * wo
        ctx.n = n
        if STEM_DIRECT and not _DET_STATS and _hip.call_status("u2_stem_conv_fwd", ptrs, hs, ws, b, int(is_u8), pixel_mean, pixel_std,
                                                               wk, out, stats, hpad, wpad, n, kp) == 0:
            ctx.direct = (list(images), ptrs, hs, ws, int(is_u8), pixel_mean, pixel_std, hpad, wpad)
            ctx.mark_non_differentiable(stats)
            return out, stats
        ctx.direct = None
        col = torch.empty((m, kp), dtype=BF16, device=weight.device)
        _hip.call("u2_stem_im2col_batch", ptrs, hs, ws, b, int(is_u8), pixel_mean, pixel_std, col, hpad, wpad, kp)
        # (a GEMM over col, here and in backward; no ConvGeom: out and dwk have n rows / columns as they are, not ceil32(n))
        _hip.call("u2_conv_igemm", col, wk, out, None, None if _DET_STATS else stats, 1, m, 1, kp, kp, m, 1, n, n, 1, 1, 0, 0, 1,
                  1, 0, 0, 0)
        if _DET_STATS:
            stats = _fixed_order_stats(out, n)
        ctx.save_for_backward(col)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _ds):
        n, kp = ctx.n, _StemConvFn.KP
        dout = dout.contiguous()
        dwk = zeros_f32((n, 1, kp), dout.device)
        if ctx.direct is not None:
            images, ptrs, hs, ws, is_u8, pixel_mean, pixel_std, hpad, wpad = ctx.direct
            # (the forward launcher served this call, so the same checks pass here)
            _hip.call("u2_stem_conv_wgrad", ptrs, hs, ws, len(images), is_u8, pixel_mean, pixel_std, dout, dwk, hpad, wpad, n, kp)
        else:
            (col,) = ctx.saved_tensors
            m = col.shape[0]
            _hip.call("u2_conv_wgrad", col, dout, dwk, 1, m, 1, kp, kp, m, 1, n, n, 1, 1, 0, 0, 1, 0)
        dw = dwk[:, 0, :147].view(n, 7, 7, 3).permute(0, 3, 1, 2)
        return dw, None, None, None, None, None


def stem_conv(weight, images, pixel_mean, pixel_std, hpad, wpad):
    return _StemConvFn.apply(weight, images, pixel_mean, pixel_std, hpad, wpad)


# --------------------------------------------------------------------------------------------
# normalisation
# --------------------------------------------------------------------------------------------
def _bn_exchange_stats(stats, m, c, sync):
    """The statistics a (Sync)BatchNorm forward normalises with -> (stats, count, count_dev, world): this process' column sums
    and element count m, or under SyncBN the sums over all ranks and their count on the device."""
    world = _world() if sync else 1
    count, count_dev = float(m), None
    if world > 1:
        # nn.SyncBatchNorm (layers/batch_norm.py:187) gathers (mean, invstd, count) of every rank: the ranks pad their
        # batches to their own maximum image size, so the element counts differ.  One all-reduce of [sum | sumsq | count].
        packed = getattr(stats, "_u2_packed", None)
        if packed is None or packed.numel() != 2 * c + 1:  # statistics that did not come from a conv epilogue (tests)
            packed = torch.cat([stats.reshape(-1).float(), stats.new_zeros(1, dtype=torch.float32)])
        packed[2 * c :].fill_(float(m))  # an asynchronous fill: no synchronising constant upload per batch shape
        dist.all_reduce(packed)
        stats, count_dev = packed[: 2 * c].view(2, c), packed[2 * c :]
    return stats, count, count_dev, world


def _bn_exchange_sums(sums, world, grad_dst):
    """The backward sums [sum dz | sum dz xhat] of a (Sync)BatchNorm, all-reduced in place under SyncBN
    -> (this rank's own sums, coef [5, C] scratch, direct, dgamma, dbeta): the parameter gradients go straight into their arena
    slices (direct) or into coef rows 0-1; rows 2-4 take the coefficients of dx."""
    local = sums
    if world > 1:
        local = sums.clone()
        dist.all_reduce(sums)
    coef = torch.empty((5, sums.shape[1]), dtype=torch.float32, device=sums.device)
    direct = grad_dst is not None
    dgamma, dbeta = grad_dst if direct else (coef[0], coef[1])
    return local, coef, direct, dgamma, dbeta


def _norm_grad_dst(gamma, beta):
    """The (dgamma, dbeta) arena slices a norm's backward kernels add into, or None: autograd then receives the two gradients."""
    gd, bd = grad_slot(gamma), grad_slot(beta)
    ok = gd is not None and bd is not None and gd.is_contiguous() and bd.is_contiguous() and gd.dtype == torch.float32
    return (gd, bd) if ok else None


class _BatchNormActFn(Function):
    """Training-mode (Sync)BatchNorm (+residual)(+ReLU) on a conv output whose column statistics were
    produced by the conv epilogue (reference: nn.SyncBatchNorm chosen at layers/batch_norm.py:187,
    residual add + relu_ at backbone/resnet.py:204-210)."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, residual, relu, momentum, eps, grad_dst=None,
                twin=False, sync=True, res_up=False, lazy_ok=None, tail=None, res_tail=None):
        _check_act(y)
        b, h, w, c = y.shape
        m = b * h * w
        ctx.lazy_ok = lazy_ok   # None, or the _LazyLink between this node's backward and the guard hook on y
        stats, count, count_dev, world = _bn_exchange_stats(stats, m, c, sync)
        mean = torch.empty(c, dtype=torch.float32, device=y.device)
        invstd, scale, shift = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        out = torch.empty_like(y)
        bits = None
        if res_up:
            # FPN top-down step (backbone/fpn.py:153-155): the residual is the coarser level, nearest-upsampled on the fly
            assert residual is not None and not relu and tuple(residual.shape) == (b, h // 2, w // 2, c)
            _hip.call("u2_bn_finalize_fwd", stats, count, count_dev, gamma, beta, running_mean, running_var, momentum, eps, mean,
                      invstd, scale, shift, c)
            _hip.call("u2_affine_upadd", y, scale, shift, residual.contiguous(), out, b, h, w, c, 0)
        else:
            # a residual block's tail: backward needs only the sign of the activation - kept as one bit per element, so that
            # the reduce pass reads a sixteenth of the activation's bytes for it
            cpr = c // 8
            if relu and residual is not None and c % 8 == 0 and cpr <= 256 and 256 % cpr == 0:
                bits = torch.empty((m, cpr), dtype=torch.uint8, device=y.device)
            # finalize + apply in one launch (round 4): the coefficients are derived per thread from the column sums
            _hip.call("u2_bn_act_fused", y, stats, count, count_dev, gamma, beta, running_mean, running_var, momentum, eps, mean,
                      invstd, scale, shift, residual, out, m, c, c, int(relu), bits)
        # ReLU mask in backward: without a residual it is recomputed from y (one activation read less per pass)
        remask = relu and residual is None
        keep_out = relu and not remask
        ctx.mask_bits = bool(keep_out and bits is not None)
        # tail: this block's own state, for the next block's conv1 (needs the bit mask); res_tail: the state of the block whose
        # output is this block's identity shortcut - this tail's backward posts the residual gradient there
        ctx.tail = tail if (tail is not None and ctx.mask_bits and twin) else None
        if ctx.tail is not None:
            tail.y, tail.bits, tail.mean, tail.invstd = y, bits, mean, invstd
        ctx.res_tail = res_tail
        ctx.save_for_backward(y, (bits if ctx.mask_bits else out) if keep_out else None, gamma, mean, invstd,
                              scale if remask else None, shift if remask else None)
        ctx.cfg = (relu, count, world, residual is not None)
        ctx.count_dev = count_dev
        ctx.res_up = res_up
        ctx.grad_dst = grad_dst  # (dgamma, dbeta) arena slices or None
        ctx.twin = twin
        if twin:  # two or three handles on the same activation: their gradients arrive separately and are summed in the kernel
            ctx.set_materialize_grads(False)
            return (out, out.detach(), out.detach()) if int(twin) == 3 else (out, out.detach())
        return out

    @staticmethod
    def backward(ctx, dout, dout2=None, dout3=None):
        y, out, gamma, mean, invstd, msc, msh = ctx.saved_tensors
        relu, count, world, has_res = ctx.cfg
        b, h, w, c = y.shape
        m = b * h * w
        nret = 17
        fuse = has_res and relu  # residual block tail: dz is materialised by the reduce pass and is the residual gradient
        done = _tail_take(ctx.tail, dout, dout2, dout3, y)
        if done is not None:
            dz, sums = done   # the next block's conv1 data gradient has formed them (u2_conv_dgrad_tail)
        else:
            arrived = [g.contiguous() for g in (dout, dout2, dout3) if g is not None]
            if not arrived:
                return (None,) * nret
            if not fuse and len(arrived) > 1:
                total = arrived[0]
                for g in arrived[1:]:
                    total = total + g
                arrived = [total]
            dout, dout2, dout3 = (arrived + [None, None])[:3]
            dz = torch.empty_like(y) if fuse else None
            sums = zeros_f32((2, c), y.device)
            _hip.call("u2_norm_bwd_reduce", dout, out, y, mean, invstd, sums, 1, m, c, c, int(relu), msc, msh, dout2, dz, dout3,
                      int(bool(ctx.mask_bits and fuse)))
        if fuse and ctx.res_tail is not None and TAIL_BWD_FUSE:
            ctx.res_tail.g2 = dz   # for the conv1 that shares the previous block's output with this block's shortcut
        local, coef, direct, dgamma, dbeta = _bn_exchange_sums(sums, world, ctx.grad_dst)
        if ctx.lazy_ok is not None and LAZY_BN_APPLY and (fuse or (not relu and not has_res)):
            # the producing 1x1 conv evaluates the apply step dx = k1 dz + k2 y + k3 on its staged rows (u2_conv1x1_bwd_fused_bn,
            # round 5): only the coefficients (and dgamma / dbeta) are computed here, dx is never stored.  What autograd carries
            # to the conv is a one-element placeholder expanded to the shape; _Conv2dFn.backward finds the operands by its address.
            _hip.call("u2_bn_finalize_bwd", sums, count, ctx.count_dev, gamma, mean, invstd, local, dgamma, dbeta, coef[2], coef[3],
                      coef[4], c, int(direct))
            ph = deferred.post(deferred.BN_APPLY, y.device, y.shape, (dz if fuse else dout, y, coef))
            ctx.lazy_ok.posted = ph   # what _lazy_guard must see arrive at the conv output
            return (ph, None, (None if direct else dgamma), (None if direct else dbeta), None, None, (dz if fuse else None)) \
                + (None,) * 10
        dx = torch.empty_like(y)
        # finalize (coefficients of dx, dgamma / dbeta) + apply in one launch (round 4); coef[2:5] is scratch for the channel
        # counts the one-launch form does not serve
        if fuse:
            _hip.call("u2_bn_bwd_apply_fused", sums, count, ctx.count_dev, gamma, mean, invstd, local, dgamma, dbeta, coef[2:],
                      int(direct), dz, None, y, dx, None, m, c, c, 0, None, None)
            dres = dz
        else:
            dres = torch.empty_like(y) if (has_res and not ctx.res_up) else None
            _hip.call("u2_bn_bwd_apply_fused", sums, count, ctx.count_dev, gamma, mean, invstd, local, dgamma, dbeta, coef[2:],
                      int(direct), dout, out, y, dx, dres, m, c, c, int(relu), msc, msh)
            if ctx.res_up:  # gradient of the coarser level: the 2x2 sums of dout
                dres = torch.empty((b, h // 2, w // 2, c), dtype=BF16, device=y.device)
                _hip.call("u2_fpn_upsample_add_bwd", dout, dres, b, h, w, c)
        if direct:
            dgamma = dbeta = None
        return (dx, None, dgamma, dbeta, None, None, dres) + (None,) * 10


def batch_norm_act(y, stats, gamma, beta, running_mean, running_var, residual=None, relu=False, momentum=0.1,
                   eps=1e-5, twin=False, sync=True, res_up=False):
    """twin=True: returns the activation with a second autograd handle on the same memory in `._u2_twin` (for a consumer
    pair such as the next residual block's conv1 and identity shortcut); the two gradients are summed inside the
    backward kernel instead of by autograd.  twin=3: a third handle in `._u2_third` as well.  sync=False: per-process statistics (NORM "BN"), no all-reduce.
    res_up=True: `residual` is the next coarser FPN level [B, H/2, W/2, C], nearest-upsampled inside the same pass."""
    grad_dst = _norm_grad_dst(gamma, beta)
    twin = (3 if twin == 3 else int(bool(twin))) if torch.is_grad_enabled() else 0
    lazy_ok = None
    if getattr(y, "_u2_lazy_ok", False) and y.requires_grad and torch.is_grad_enabled():
        # the conv output must reach its convolution's backward as the placeholder itself: a second consumer of y, or anything
        # else that makes autograd form a sum, would silently drop the deferred gradient - fail there and then instead
        lazy_ok = _LazyLink()
        y.register_hook(functools.partial(_lazy_guard, lazy_ok))
    # a residual block's tail with exactly two handles: the next block's conv1 may form this tail's (dz, sums) in its data-gradient
    # launch (_TailState); a tail whose residual is such a block's second handle posts its residual gradient there
    tail = _TailState() if (TAIL_BWD_FUSE and twin == 1 and relu and residual is not None and not res_up and y.requires_grad) else None
    res_tail = getattr(residual, "_u2_tail", None) if (residual is not None and not res_up and twin) else None
    out = _BatchNormActFn.apply(y, stats, gamma, beta, running_mean, running_var, residual, relu, momentum, eps, grad_dst,
                                twin, sync, res_up, lazy_ok, tail, res_tail)
    if tail is not None and tail.bits is not None:
        out[0]._u2_tail = out[1]._u2_tail = tail
    if twin == 3:  # a third handle (`._u2_third`) for a third consumer, e.g. the FPN lateral conv on a stage output
        out, other, third = out
        out._u2_twin, out._u2_third = other, third
    elif twin:
        out, other = out
        out._u2_twin = other
    return out


def affine_act(y, scale, shift, residual=None, relu=False):
    """Inference-mode normalisation: y*scale + shift (+res)(relu); no autograd."""
    b, h, w, c = y.shape
    out = torch.empty_like(y)
    _hip.call("u2_affine_act", y, scale.contiguous(), shift.contiguous(), residual, out, 1, b * h * w, c, c, int(relu), None)
    return out


class _GroupNormActFn(Function):
    """nn.GroupNorm(G, C) (+ReLU) on NHWC (reference: layers/batch_norm.py:189, semantic_seg.py:196-205)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, groups, relu, eps, grad_dst=None, ordered=False):
        _check_act(y)
        b, h, w, c = y.shape
        hw = h * w
        cg = c // groups
        ctx.grad_dst = grad_dst  # (dgamma, dbeta) arena slices or None
        if ordered:
            # sums in a fixed order: the same input gives the same bits from run to run (u2_colstats adds with atomics)
            nchunk = max(1, min(256, (hw + 255) // 256))
            part = torch.empty((b, nchunk, 2, c), dtype=torch.float32, device=y.device)
            stats = torch.empty((b, 2, c), dtype=torch.float32, device=y.device)
            _hip.call("u2_colstats_ordered", y, part, stats, b, hw, c, c, nchunk)
        else:
            stats = zeros_f32((b, 2, c), y.device)
            _hip.call("u2_colstats", y, stats, b, hw, c, c)
        coef = torch.empty((4, b, c), dtype=torch.float32, device=y.device)
        mean, invstd, scale, shift = coef[0], coef[1], coef[2], coef[3]
        _hip.call("u2_gn_finalize_fwd", stats, gamma.detach(), beta.detach(), float(hw * cg), float(eps), b, c, groups, mean,
                  invstd, scale, shift)
        out = torch.empty_like(y)
        _hip.call("u2_affine_act", y, scale, shift, None, out, b, hw, c, c, int(relu), None)
        ctx.save_for_backward(y, gamma, mean, invstd, scale if relu else None, shift if relu else None)
        ctx.cfg = (groups, relu)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gamma, mean, invstd, msc, msh = ctx.saved_tensors
        groups, relu = ctx.cfg
        b, h, w, c = y.shape
        hw, cg = h * w, c // groups
        n = float(hw * cg)
        dout = dout.contiguous()
        sums = zeros_f32((b, 2, c), y.device)
        _hip.call("u2_norm_bwd_reduce", dout, None, y, mean, invstd, sums, b, hw, c, c, int(relu), msc, msh, None, None, None, 0)
        coef = torch.empty((3, b, c), dtype=torch.float32, device=y.device)
        k1, k2, k3 = coef[0], coef[1], coef[2]
        direct = ctx.grad_dst is not None
        if direct:   # accumulated into the optimizer's arena slices by the finalize kernel: nothing for AccumulateGrad to add
            dg, db = ctx.grad_dst
        else:
            dparam = torch.empty((2, c), dtype=torch.float32, device=y.device)
            dg, db = dparam[0], dparam[1]
        _hip.call("u2_gn_finalize_bwd", sums, gamma.detach(), mean, invstd, n, b, c, groups, k1, k2, k3, dg, db, int(direct))
        dx = torch.empty_like(y)
        _hip.call("u2_norm_bwd_apply", dout, None, y, k1, k2, k3, dx, None, b, hw, c, c, int(relu), msc, msh)
        return dx, (None if direct else dg), (None if direct else db), None, None, None, None, None


def group_norm_act(y, gamma, beta, groups, relu=False, eps=1e-5):
    # without a graph (inference) the statistics are summed in a fixed order, so that a model in eval mode repeats its bits: test-time
    # augmentation compares and averages passes over the same views (modeling/test_time_augmentation.py)
    return _GroupNormActFn.apply(y, gamma, beta, groups, relu, eps, _norm_grad_dst(gamma, beta), not torch.is_grad_enabled())


# --------------------------------------------------------------------------------------------
# pooling / resampling
# --------------------------------------------------------------------------------------------
def _pooled_shape(h, w):
    """Output height and width of the 3x3 / stride-2 / pad-1 max pool."""
    return (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1


class _MaxPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        _check_act(x)
        b, h, w, c = x.shape
        ho, wo = _pooled_shape(h, w)
        y = torch.empty((b, ho, wo, c), dtype=BF16, device=x.device)
        idx = torch.empty((b, ho, wo, c), dtype=torch.uint8, device=x.device)
        _hip.call("u2_maxpool3x3s2_fwd", x, y, idx, b, h, w, c)
        ctx.save_for_backward(idx)
        ctx.shape = (b, h, w, c)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        b, h, w, c = ctx.shape
        dx = torch.empty((b, h, w, c), dtype=BF16, device=dy.device)
        _hip.call("u2_maxpool3x3s2_bwd", dy.contiguous(), idx, dx, b, h, w, c)
        return dx


def max_pool_3x3_s2(x):
    return _MaxPoolFn.apply(x)


class _BatchNormReluMaxPoolFn(Function):
    """The stem's tail, norm -> relu_ -> max_pool2d(3, 2, 1) (backbone/resnet.py:355-359), without the activation between the
    normalisation and the pool (round 6): the pool normalises its nine taps itself, and the normalisation's backward passes
    rebuild the pool's gradient per input pixel from (dy, idx).  Pooled values and winner slots are those of
    `max_pool_3x3_s2(batch_norm_act(y, ..., relu=True))`, bit for bit; the statistics steps (all-reduce of [sum | sumsq | count]
    forward, of [sum dz | sum dz xhat] backward) are `_BatchNormActFn`'s."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, momentum, eps, grad_dst, sync):
        _check_act(y)
        b, h, w, c = y.shape
        stats, count, count_dev, world = _bn_exchange_stats(stats, b * h * w, c, sync)
        coef = torch.empty((4, c), dtype=torch.float32, device=y.device)
        mean, invstd, scale, shift = coef[0], coef[1], coef[2], coef[3]
        _hip.call("u2_bn_finalize_fwd", stats, count, count_dev, gamma, beta, running_mean, running_var, momentum, eps, mean,
                  invstd, scale, shift, c)
        ho, wo = _pooled_shape(h, w)
        out = torch.empty((b, ho, wo, c), dtype=BF16, device=y.device)
        idx = torch.empty((b, ho, wo, c), dtype=torch.uint8, device=y.device)
        _hip.call("u2_affine_relu_maxpool_fwd", y, scale, shift, out, idx, b, h, w, c)
        ctx.save_for_backward(y, idx, gamma, mean, invstd, scale, shift)
        ctx.cfg = (count, world)
        ctx.count_dev = count_dev
        ctx.grad_dst = grad_dst
        return out

    @staticmethod
    def backward(ctx, dy):
        y, idx, gamma, mean, invstd, msc, msh = ctx.saved_tensors
        count, world = ctx.cfg
        b, h, w, c = y.shape
        dy = dy.contiguous()
        sums = zeros_f32((2, c), y.device)
        _hip.call("u2_affine_relu_maxpool_bwd_reduce", dy, idx, y, mean, invstd, msc, msh, sums, b, h, w, c)
        local, coef, direct, dgamma, dbeta = _bn_exchange_sums(sums, world, ctx.grad_dst)
        _hip.call("u2_bn_finalize_bwd", sums, count, ctx.count_dev, gamma, mean, invstd, local, dgamma, dbeta, coef[2], coef[3],
                  coef[4], c, int(direct))
        dx = torch.empty_like(y)
        _hip.call("u2_affine_relu_maxpool_bwd_apply", dy, idx, y, coef[2], coef[3], coef[4], msc, msh, dx, b, h, w, c)
        return dx, None, (None if direct else dgamma), (None if direct else dbeta), None, None, None, None, None, None


def stem_tail_ok(c):
    """Channel counts the one-pass stem tail serves (a thread keeps one 8-channel chunk: C / 8 must divide 256)."""
    return STEM_TAIL_FUSE and c % 8 == 0 and 1 <= c // 8 <= 256 and 256 % (c // 8) == 0


def batch_norm_relu_max_pool(y, stats, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, sync=True):
    return _BatchNormReluMaxPoolFn.apply(y, stats, gamma, beta, running_mean, running_var, momentum, eps,
                                         _norm_grad_dst(gamma, beta), sync)


def affine_relu_max_pool(y, scale, shift):
    """Inference: max_pool_3x3_s2(affine_act(y, scale, shift, relu=True)) in one pass; no autograd."""
    b, h, w, c = y.shape
    ho, wo = _pooled_shape(h, w)
    out = torch.empty((b, ho, wo, c), dtype=BF16, device=y.device)
    idx = torch.empty((b, ho, wo, c), dtype=torch.uint8, device=y.device)
    _hip.call("u2_affine_relu_maxpool_fwd", y, scale.contiguous(), shift.contiguous(), out, idx, b, h, w, c)
    return out


class _UpsampleAddFn(Function):
    @staticmethod
    def forward(ctx, lateral, top):
        _check_act(lateral)
        b, h, w, c = lateral.shape
        assert top.shape == (b, h // 2, w // 2, c), (lateral.shape, top.shape)
        out = torch.empty_like(lateral)
        _hip.call("u2_fpn_upsample_add_fwd", lateral, top.contiguous(), out, b, h, w, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        b, h, w, c = dout.shape
        dtop = torch.empty((b, h // 2, w // 2, c), dtype=BF16, device=dout.device)
        _hip.call("u2_fpn_upsample_add_bwd", dout, dtop, b, h, w, c)
        return dout, dtop


def fpn_upsample_add(lateral, top):
    return _UpsampleAddFn.apply(lateral, top)


class _BilinearUp2Fn(Function):
    @staticmethod
    def forward(ctx, x, addend):
        _check_act(x)
        b, h, w, c = x.shape
        out = torch.empty((b, 2 * h, 2 * w, c), dtype=BF16, device=x.device)
        _hip.call("u2_bilinear_up2_fwd", x, addend, out, b, h, w, c)
        ctx.shape = (b, h, w, c)
        ctx.has_add = addend is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        b, h, w, c = ctx.shape
        dout = dout.contiguous()
        # The semantic head sums its per-level branches at the common stride (semantic_seg.py:246-253), the last x2 upsample of
        # every branch adding the running sum: the SAME gradient tensor arrives here once per branch (it is handed on unchanged
        # as the addend's gradient), and its transposed upsample is the same tensor each time - computed once, shared (round 5:
        # 0.43 -> 0.16 ms of bilinear2_bwd_kernel per step).  The entry holds `dout` itself, so its address cannot be reused.
        global _UP2_BWD_LAST
        key = (dout.device.index, dout.data_ptr(), dout._version, tuple(dout.shape), torch.cuda.current_stream(dout.device).cuda_stream)
        hit = _UP2_BWD_LAST
        if hit is not None and hit[0] == key:
            dx = hit[2]
        else:
            dx = torch.empty((b, h, w, c), dtype=BF16, device=dout.device)
            _hip.call("u2_bilinear_up2_bwd", dout, dx, b, h, w, c)
            if ctx.has_add:   # (the engine runs a whole branch before the next one's node: the other upsamples must not evict it)
                _UP2_BWD_LAST = (key, dout, dx)
        return dx, (dout if ctx.has_add else None)


def bilinear_up2(x, addend=None):
    return _BilinearUp2Fn.apply(x, addend)


# --------------------------------------------------------------------------------------------
# ROI ops
# --------------------------------------------------------------------------------------------
def _level_arrays(shapes, scales):
    nl = len(shapes)
    hs = (ctypes.c_int * nl)(*[s[1] for s in shapes])
    ws = (ctypes.c_int * nl)(*[s[2] for s in shapes])
    sc = (ctypes.c_float * nl)(*scales)
    return hs, ws, sc


def _roi_group(rois, levels, b, nl):
    """ROIs grouped by (image, level) for the per-pixel gather: order int32 [R], segment offsets int32 [b*nl+1]."""
    r = rois.shape[0]
    if b * nl <= 256 and r <= 32768 and 512 * (b * nl + 2) + 2 * r <= 155648 and levels.dtype == torch.int32:
        order = torch.empty(r, dtype=torch.int32, device=rois.device)
        seg = torch.empty(b * nl + 1, dtype=torch.int32, device=rois.device)
        _hip.call("u2_roi_group", rois.contiguous(), levels.contiguous(), order, seg, r, b, nl)
        return order, seg
    key = rois[:, 0].to(torch.int64) * nl + levels.to(torch.int64)
    order = torch.argsort(key, stable=True).to(torch.int32)
    seg = torch.zeros(b * nl + 1, dtype=torch.int32, device=rois.device)
    seg[1:] = torch.cumsum(torch.bincount(key, minlength=b * nl), 0)
    return order, seg


# what a ROIAlign node's backward leaves for the gather pass; event: the point of its stream at which the four tensors are complete
_RoiSet = collections.namedtuple("_RoiSet", "rois order seg dout out_size grad_scale event", defaults=(None,))


def _roi_sets_join(sets):
    """The current stream waits for the sets left by ROIAlign nodes that ran on another stream (the mask head's) and keeps their
    tensors alive."""
    if not sets or not sets[0].dout.is_cuda:
        return
    here = torch.cuda.current_stream(sets[0].dout.device)
    for st in sets:
        if st.event is not None:
            here.wait_event(st.event)
            for t in st[:4]:
                t.record_stream(here)


def _roi_gather(shapes, scales, sets, device, level=None, addends=()):
    """sets: [_RoiSet] (at most 4) -> per-level bf16 gradient maps, each written once.
    level = l: that level's map only (a one-element list), with up to two more bf16 gradient maps of its shape (`addends`: what
    the map's other readers produced) added in fp32 before the rounding (u2_roi_align_bwd_gather_sum)."""
    nl, ns = len(shapes), len(sets)
    hs, ws, sc = _level_arrays(shapes, scales)
    lv = range(nl) if level is None else [level]
    gbuf = {l: torch.empty(shapes[l], dtype=BF16, device=device) for l in lv}
    ptrs = (ctypes.c_void_p * nl)(*[gbuf[l].data_ptr() if l in gbuf else None for l in range(nl)])
    keep = [tuple(t.contiguous() if isinstance(t, torch.Tensor) else t for t in st) for st in sets]
    arr = lambda k: (ctypes.c_void_p * ns)(*[st[k].data_ptr() for st in keep])
    ps = (ctypes.c_int * ns)(*[st[4] for st in keep])
    gs = (ctypes.c_float * ns)(*[float(st[5]) for st in keep])
    if level is None:
        _hip.call("u2_roi_align_bwd_gather_multi", ptrs, hs, ws, sc, nl, ns, arr(0), arr(1), arr(2), arr(3), ps, gs,
                  shapes[0][0], shapes[0][3])
        return [gbuf[l] for l in range(nl)]
    assert len(addends) <= 2 and all(tuple(a.shape) == tuple(shapes[level]) and a.dtype == BF16 and a.is_contiguous() for a in addends)
    adds = list(addends) + [None, None]
    a0 = (ctypes.c_void_p * nl)(*[adds[0].data_ptr() if (l == level and adds[0] is not None) else None for l in range(nl)])
    a1 = (ctypes.c_void_p * nl)(*[adds[1].data_ptr() if (l == level and adds[1] is not None) else None for l in range(nl)])
    _hip.call("u2_roi_align_bwd_gather_sum", ptrs, hs, ws, sc, nl, 1 << level, ns, arr(0), arr(1), arr(2), arr(3), ps, gs, a0, a1,
              shapes[0][0], shapes[0][3])
    return [gbuf[level]]


class _FanOutFn(Function):
    """k autograd handles on one tensor: their gradients arrive separately and are summed by one kernel (u2_add_n) instead of
    autograd's k - 1 accumulation adds."""

    @staticmethod
    def forward(ctx, x, k):
        ctx.set_materialize_grads(False)
        return tuple(x.detach() for _ in range(k))

    @staticmethod
    def backward(ctx, *grads):
        lazy = None
        for g in grads:   # one of the gradients may be the placeholder of a deferred ROIAlign gather (roi_grad_tap, round 6)
            ent = deferred.take(deferred.ROI_GATHER, g) if g is not None else None
            if ent is not None:
                assert lazy is None
                lazy, grads = ent, tuple(h for h in grads if h is not g)
        gs = [g.contiguous() for g in grads if g is not None]
        if not gs and lazy is None:
            return None, None
        while len(gs) > (2 if lazy is not None else 1):
            part, gs = gs[:4], gs[4:]
            if part[0].dtype != BF16 or part[0].numel() % 8:
                total = part[0]
                for g in part[1:]:
                    total = total + g
            else:
                total = torch.empty_like(part[0])
                part = part + [None] * (4 - len(part))
                _hip.call("u2_add_n", part[0], part[1], part[2], part[3], total, total.numel())
            gs.insert(0, total)
        if lazy is not None:
            # the ROI poolers' gradient of this map is formed HERE, with the other readers' gradients added inside the gather
            # (fp32, one rounding): the separate u2_add_n pass read the gathered map back and the other two again
            shared, level = lazy
            _roi_sets_join(shared["pend"])
            if any(g.dtype != BF16 for g in gs):
                gs = [g.to(BF16) for g in gs]
            out = _roi_gather(shared["shapes"], shared["scales"], shared["pend"], shared["device"], level, gs)[0]
            return out, None
        return gs[0], None


def fan_out(x, k):
    """`k` handles on `x` for `k` consumers (training only; without autograd the tensor itself k times)."""
    if k <= 1 or not (torch.is_grad_enabled() and x.requires_grad):
        return (x,) * max(k, 1)
    outs = _FanOutFn.apply(x, k)
    for o in outs:
        o._u2_fan = True   # its gradient goes straight to _FanOutFn.backward, which can take a deferred ROI gather (roi_grad_tap)
    return outs


class RoiGradTap:
    """Shared state of one roi_grad_tap(): the ROIAlign calls made on the tapped maps leave their (rois, dout) here in
    backward, and the tap's own backward turns all of them into the maps' gradient with one gather pass."""

    def __init__(self, feats, scales_hint=None):
        self.shapes = [tuple(f.shape) for f in feats]
        self.pending = []
        self.scales = None
        self.ids = None
        self.defer = False   # every map is a fan_out handle: the gather is left to _FanOutFn.backward (see there)


class _RoiGradTapFn(Function):
    @staticmethod
    def forward(ctx, state, *feats):
        ctx.state = state
        ctx.set_materialize_grads(False)
        return tuple(f.detach() for f in feats)

    @staticmethod
    def backward(ctx, *gfeats):
        st = ctx.state
        grads = list(gfeats)
        pend, st.pending = st.pending, []
        if st.defer and ROI_SUM_FOLD and pend and len(pend) <= 4 and all(g is None for g in grads) and pend[0].dout.is_cuda:
            # every tapped map is a fan_out handle: hand its _FanOutFn.backward a zero placeholder and let IT run the level's
            # gather, with the gradients of the map's other readers as addends (u2_roi_align_bwd_gather_sum)
            dev = pend[0].dout.device
            shared = {"shapes": st.shapes, "scales": st.scales, "pend": pend, "device": dev}
            return (None, *[deferred.post(deferred.ROI_GATHER, dev, shape, (shared, l)) for l, shape in enumerate(st.shapes)])
        _roi_sets_join(pend)
        for i in range(0, len(pend), 4):
            gbuf = _roi_gather(st.shapes, st.scales, pend[i : i + 4], pend[i].dout.device)
            grads = [g if old is None else old + g for old, g in zip(grads, gbuf)]
        return (None, *grads)


def roi_grad_tap(feats):
    """Identity on the FPN maps that defers the backward of every roi_align() made on its outputs: the cascade's three
    box poolers and the mask pooler (modeling/poolers.py:206-263 x 4) then cost one gather pass per level, and the four
    gradient maps per level that autograd would otherwise materialise and sum are never formed."""
    state = RoiGradTap(feats)
    state.defer = all(getattr(f, "_u2_fan", False) for f in feats)
    outs = _RoiGradTapFn.apply(state, *feats)
    state.ids = [id(o) for o in outs]
    for o in outs:
        o._u2_roi_tap = state
    return list(outs)


def _roi_process_order(rois, levels, nimg, nlevels):
    """Processing order of the ROIAlign forward: sorted by (level, image, top row of the box at its level / 8)."""
    key = (levels.long() * nimg + rois[:, 0].long()) * 4096 + (rois[:, 2] * (0.25 / 8)).long().clamp_(0, 4095)
    return torch.argsort(key).to(torch.int32)


class _ROIAlignFn(Function):
    """Multi-level ROIAlign(aligned=True, sampling_ratio=0) (modeling/poolers.py:206-263)."""

    @staticmethod
    def forward(ctx, rois, levels, out_size, scales, grad_scale, tap, *feats):
        nl = len(feats)
        for f in feats:
            _check_act(f)
        c = feats[0].shape[3]
        r = rois.shape[0]
        ptrs = (ctypes.c_void_p * nl)(*[f.data_ptr() for f in feats])
        hs, ws, sc = _level_arrays([f.shape for f in feats], scales)
        out = torch.empty((r, out_size, out_size, c), dtype=BF16, device=rois.device)
        order = _roi_process_order(rois, levels, feats[0].shape[0], nl) if r >= ROI_ORDER_MIN else None
        _hip.call("u2_roi_align_fwd", ptrs, hs, ws, sc, nl, rois.contiguous(), levels.contiguous(), order, out, r, c, out_size,
                  out_size)
        ctx.save_for_backward(rois, levels)
        ctx.cfg = (out_size, scales, grad_scale, [tuple(f.shape) for f in feats])
        ctx.tap = tap
        return out

    @staticmethod
    def backward(ctx, dout):
        rois, levels = ctx.saved_tensors
        out_size, scales, grad_scale, shapes = ctx.cfg
        nl = len(shapes)
        b = shapes[0][0]
        r, c = rois.shape[0], shapes[0][3]
        none = (None,) * 6
        if ROI_ALIGN_BWD_ATOMIC:
            hs, ws, sc = _level_arrays(shapes, scales)
            gbuf = [torch.zeros(s, dtype=torch.float32, device=dout.device) for s in shapes]
            ptrs = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in gbuf])
            _hip.call("u2_roi_align_bwd", ptrs, hs, ws, sc, nl, rois.contiguous(), levels.contiguous(), dout.contiguous(),
                      r, c, out_size, out_size, float(grad_scale))
            return (*none, *[g.to(BF16) for g in gbuf])
        order, seg = _roi_group(rois, levels, b, nl)
        entry = _RoiSet(rois, order, seg, dout, out_size, grad_scale)
        tap = ctx.tap
        if tap is not None:  # deferred: the tap's backward gathers all pending sets at once
            tap.scales = scales
            if dout.is_cuda:  # the tap may run on another stream than this node: mark the point its inputs are complete at
                ev = torch.cuda.Event()
                ev.record()
                entry = entry._replace(event=ev)
            tap.pending.append(entry)
            return (*none, *([None] * nl))
        return (*none, *_roi_gather(shapes, scales, [entry], dout.device))


def roi_align(feats, rois, levels, out_size, scales, grad_scale=1.0):
    tap = getattr(feats[0], "_u2_roi_tap", None)
    if tap is not None and (ROI_ALIGN_BWD_ATOMIC or tap.ids != [id(f) for f in feats]):
        tap = None  # not exactly the tapped list of maps: gather on the spot
    return _ROIAlignFn.apply(rois, levels, out_size, tuple(scales), grad_scale, tap, *feats)


# --------------------------------------------------------------------------------------------
# the state of the backward folds (layers/deferred.py)
# --------------------------------------------------------------------------------------------
class _TailState:
    """What a residual block's tail (_BatchNormActFn: residual, ReLU, two handles) shares with the two consumers of its output:
    its saved tensors for the conv1 that may run its reduce; g2, the residual gradient the next tail posts; result, the
    (dz, sums) that conv1 formed, waiting for this tail's backward (the placeholder autograd was handed is posted with this state)."""
    y = bits = mean = invstd = g2 = result = None


def _tail_take(tail, dout, dout2, dout3, y):
    """_BatchNormActFn.backward: (dz, sums) if the next block's conv1 has formed them - then `dout` must be that launch's
    placeholder and `dout2` the gradient it summed, untouched; None for the two-launch path.  Anything else that involves a
    placeholder (one that arrives at another layer, in another position or summed with a further gradient; a result whose
    placeholder never arrives) would drop a gradient silently and raises instead."""
    hits = [i for i, g in enumerate((dout, dout2, dout3)) if g is not None and deferred.holds(deferred.TAIL, g)]
    pending = tail is not None and tail.result is not None
    if not hits and not pending:
        if tail is not None:
            tail.g2 = None
        return None
    posted = deferred.take(deferred.TAIL, dout) if hits == [0] else None
    ok = pending and posted is tail and dout2 is not None and dout3 is None and tail.g2 is not None \
        and dout2.data_ptr() == tail.g2.data_ptr() and tuple(dout2.shape) == tuple(y.shape) and tuple(dout.shape) == tuple(y.shape)
    if not ok:
        n = deferred.drain()[deferred.TAIL] + (1 if posted is not None else 0)
        if tail is not None:
            tail.g2 = tail.result = None
        raise RuntimeError("a residual tail's gradient formed by the next block's conv1 did not arrive as posted (placeholder in "
                           "positions %s, result pending: %s): a further consumer of the block output, or a changed gradient; "
                           "%d deferred tail gradients dropped - set U2_TAIL_BWD_FUSE=0 for such graphs" % (hits, pending, n))
    done = tail.result
    tail.g2 = tail.result = None
    return done


class _LazyLink:
    """Between a _BatchNormActFn node that may defer its apply step and the guard hook on its input: the placeholder that the node's
    backward posted (None: it did not defer)."""
    posted = None


def _lazy_guard(link, grad):
    """Tensor hook on a conv output whose batch normalisation defers its backward apply step: the gradient autograd delivers
    must be the placeholder that normalisation posted, untouched."""
    posted, link.posted = link.posted, None
    if posted is not None and not deferred.holds(deferred.BN_APPLY, grad, posted):
        raise RuntimeError("a convolution output with a deferred batch-norm gradient has a second consumer (autograd summed "
                           "the placeholder with another gradient); %d deferred gradients dropped - set U2_LAZY_BN_APPLY=0 "
                           "for graphs that re-use conv outputs" % sum(deferred.drain().values()))
    return None


def _drain_deferred():
    """Nothing of a finished (or failed) backward pass stays referenced: the deferred gradients, and the shared upsample gradient
    of the semantic head.  Returns what was still deferred, per kind."""
    global _UP2_BWD_LAST
    _UP2_BWD_LAST = None
    return deferred.drain()


def reset_deferred_gradients(strict=True):
    """Start of a training step (solver.FlatSGD.zero_grad): nothing deferred may be left over from an earlier backward pass -
    one that raised midway leaves entries behind, which must not meet the addresses of the next pass."""
    n = sum(_drain_deferred().values())
    if n and strict:
        raise RuntimeError("%d deferred gradients of an earlier backward pass were never consumed" % n)


def assert_no_deferred_gradients():
    """After a backward pass: every deferred gradient must have been consumed by the node it was left to."""
    left = _drain_deferred()
    if any(left.values()):
        raise RuntimeError("%d deferred batch-norm gradients were not consumed by their convolutions, %d deferred ROIAlign "
                           "gathers not by their fan-out nodes, %d residual-tail gradients not by their tails"
                           % (left[deferred.BN_APPLY], left[deferred.ROI_GATHER], left[deferred.TAIL]))
