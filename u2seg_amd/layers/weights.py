"""What the layers keep between launches: the pool of zeroed fp32 scratch, the kernel layouts of weights and the rounded biases
(cached on the parameter that owns them), and the optimizer's gradient slot of a parameter."""
import torch

from .. import _hip

BF16 = torch.bfloat16


def ceil32(n):
    return (n + 31) // 32 * 32


class _ZeroPool:
    """Small zero-initialised fp32 scratch tensors (statistics, split-K gradient accumulators) carved out of 16 MB
    chunks: one fill kernel per chunk instead of one per tensor.  Slices are handed out once and never recycled."""

    CHUNK = 1 << 22

    def __init__(self):
        self.chunks = {}  # (device, stream) -> [chunk, offset]: a chunk is filled on, and only handed out to, one stream

    def take(self, shape, device):
        numel = 1
        for d in shape:
            numel *= d
        if numel * 2 > self.CHUNK or numel == 0:
            return torch.zeros(shape, dtype=torch.float32, device=device)
        n = (numel + 63) // 64 * 64
        key = (device, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
        ent = self.chunks.get(key)
        if ent is None or ent[1] + n > self.CHUNK:
            ent = self.chunks[key] = [torch.zeros(self.CHUNK, dtype=torch.float32, device=device), 0]
        v = ent[0][ent[1] : ent[1] + numel].view(shape)
        ent[1] += n
        return v


_zero_pool = _ZeroPool()


def zeros_f32(shape, device):
    return _zero_pool.take(tuple(shape), torch.device(device))


def release_library_scratch():
    """Frees the device memory libu2seg_hip.so owns (stream-K hand-over slots, weight-gradient partial tiles: include/u2seg_hip.h
    u2_release_scratch); it is allocated again by the next launch that needs it.  Call it next to torch.cuda.empty_cache()."""
    return _hip.call_nostream("u2_release_scratch")


def _check_act(x):
    assert x.is_cuda and x.dtype == BF16 and x.is_contiguous() and x.dim() == 4 and x.shape[3] % 32 == 0, (
        "expected contiguous NHWC bf16 activation with C %% 32 == 0, got %s %s" % (tuple(x.shape), x.dtype)
    )


# --------------------------------------------------------------------------------------------
# weight layouts
# --------------------------------------------------------------------------------------------
def _weight_layout(w, cp, npad, mode, owner=None):
    """bf16 kernel layout of an fp32 [N, Cin, KH, KW] weight.  `owner` is the nn.Parameter whose memory `w` is (w itself or a
    reshaped view of it).  Parameters owned by solver.FlatSGD keep their layouts: the optimizer rewrites all of them in
    one launch right after each step (u2_weight_layout_batched), so the training passes launch no layout kernels.  A cached
    layout is trusted only while the parameter's autograd version and the optimizer's step stamp are unchanged."""
    n, cin, kh, kw = w.shape
    t = kh * kw
    shape = (n, t, cp) if mode == 0 else ((cp, t, npad) if mode == 1 else (t * cp, 1, npad))
    tcache = getattr(owner, "_u2_step_layouts", None) if owner is not None else None
    if tcache is not None:
        # a derived weight that lives for one pass (the RPN's concatenated predictor, used on five levels): layouts kept on the
        # tensor itself; the caller never modifies it in place
        key = (n, cin, t, cp, npad, mode)
        out = tcache.get(key)
        if out is None:
            out = tcache[key] = torch.empty(shape, dtype=BF16, device=w.device)
            _hip.call("u2_weight_layout", w.detach().float().contiguous(), out, n, cin, t, cp, npad, mode)
        return out
    stamp_ref = getattr(owner, "_u2_stamp", None) if owner is not None else None
    if mode != 0 and cp != cin:
        stamp_ref = None  # the batched transposer has no all-zero output rows; such layouts are built on the fly
    ent = None
    if stamp_ref is not None:
        cache = owner.__dict__.setdefault("_u2_layouts", {})
        key = (n, cin, t, cp, npad, mode)
        ent = cache.get(key)
        if ent is not None and ent[1] == owner._version and ent[2] == stamp_ref[0]:
            return ent[0]
    elif owner is not None and not torch.is_grad_enabled():
        # inference without an optimizer: the weights only change through torch (load_state_dict, copy_), which bumps the
        # version counter - one layout launch per weight for the whole evaluation instead of one per forward pass
        ecache = owner.__dict__.setdefault("_u2_eval_layouts", {})
        key = (n, cin, t, cp, npad, mode)
        hit = ecache.get(key)
        if hit is not None and hit[1] == owner._version and hit[2] == owner.data_ptr():
            return hit[0]
        out = torch.empty(shape, dtype=BF16, device=w.device)
        _hip.call("u2_weight_layout", w.detach().float().contiguous(), out, n, cin, t, cp, npad, mode)
        ecache[key] = (out, owner._version, owner.data_ptr())
        return out
    out = ent[0] if ent is not None else torch.empty(shape, dtype=BF16, device=w.device)
    _hip.call("u2_weight_layout", w.detach().float().contiguous(), out, n, cin, t, cp, npad, mode)
    if stamp_ref is not None:
        if ent is None:
            ent = cache[key] = [out, owner._version, stamp_ref[0]]
            owner._u2_layout_register(owner, key, ent)
        else:
            ent[1], ent[2] = owner._version, stamp_ref[0]
    return out


def weight_fwd_layout(w, cp, owner=None):
    """[N, Cin, KH, KW] fp32 -> [N, KH*KW, cp] bf16 (channels zero padded to cp)."""
    return _weight_layout(w, cp, 0, 0, owner)


def weight_dgrad_layout(w, cp, npad, owner=None):
    """[N, Cin, KH, KW] fp32 -> [cp, KH*KW, npad] bf16 with the filter flipped in both spatial axes."""
    return _weight_layout(w, cp, npad, 1, owner)


def weight_fc_dgrad_layout(w, cp, npad, owner=None):
    """[N, Cin, KH, KW] fp32 -> [KH*KW*cp, 1, npad] bf16: dx[(kh,kw,c)] = sum_n dz[n] W[n, c, kh, kw]."""
    return _weight_layout(w, cp, npad, 2, owner)


def _conv_bias(bias, round_bias):
    """The fp32 bias vector the conv epilogue adds (rounded through bf16 as autocast rounds it).  For a parameter owned by
    solver.FlatSGD the rounded copy is kept and rewritten by the optimizer's batched layout launch after every step (two small
    cast launches per biased conv and pass otherwise: 64 per training step)."""
    step_cache = getattr(bias, "_u2_step_bias", None)
    if step_cache is not None and round_bias:
        # a derived bias that lives for one pass (the RPN's concatenated predictor bias, used on five levels): rounded once
        v = step_cache.get("v")
        if v is None:
            v = step_cache["v"] = bias.detach().bfloat16().float().contiguous()
        return v
    stamp = getattr(bias, "_u2_stamp", None)
    if stamp is None or not round_bias:
        return (bias.detach().bfloat16().float() if round_bias else bias.detach().float()).contiguous()
    ent = bias.__dict__.get("_u2_bias_rounded")
    if ent is None:
        # registered with the optimizer's layout table (mode 3): rewritten with the weight layouts in the one launch after each
        # step (it was two cast launches per biased conv and step: 40 small launches)
        ent = [torch.empty(bias.shape, dtype=torch.float32, device=bias.device), -1, -1]
        bias.__dict__["_u2_bias_rounded"] = ent
        reg = getattr(bias, "_u2_layout_register", None)
        if reg is not None and bias.dim() == 1:
            reg(bias, (bias.numel(), 1, 1, 1, 0, 3), ent)
    if ent[1] != bias._version or ent[2] != stamp[0]:
        ent[0].copy_(bias.detach().bfloat16().float())
        ent[1], ent[2] = bias._version, stamp[0]
    return ent[0]


def grad_slot(param):
    """The optimizer's flat-arena gradient view of a parameter (solver/build.py:FlatSGD), or None.  Kernels that can
    accumulate into it directly do so and report no gradient to autograd (no temporary, no AccumulateGrad add)."""
    return getattr(param, "_u2_grad", None) if torch.is_grad_enabled() and param.requires_grad else None
