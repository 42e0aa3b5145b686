"""The optimizer step (u2seg_amd/csrc/optim.hip), the pooling / resampling family (pool_resize.hip) and u2_wgrad_permute_add
(norm.hip) against float64 references computed with plain torch ops (tests/float64_refs.py; tests/test_float64_refs_host.py
checks those references on the CPU).

Shapes are the smallest that reach every branch: arena tensors starting at every b & 3 with heads that swallow the whole
tensor, tensors of one, two and four chunks; maps of one pixel, one row, one column, odd sizes; more than 65 535 grid rows
(the launchers' row loop); the non-temporal max-pool backward just above its 256 MB switch; a 33-image stem batch (second
launch of the 32-image split).

Inputs come from seeded generators, rounded to bf16 where the kernel takes bf16; both sides see the same values.  Bounds are
derived from the kernels' fp32 arithmetic (u = 2^-24), written in each docstring, to first order in u, and hold with or without
fused multiply-add (a contraction only removes a rounding).  bf16 results are compared through `Check` of
test_gpu_norm_full_size: |got - bf16(ref)| <= e + step(|ref| + e), e the bound before the last rounding; every tensor also
meets the max-normalised bound of the round-1 tests (4e-3 activations, 5e-3 gradients, 1e-4 fp32 parameter data)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as TF

from tests import float64_refs as R
from tests.test_gpu_norm_full_size import Check, U, check_vec, rnd, step  # noqa: F401  (step: the unit Check bounds in)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()  # fails loudly if libu2seg_hip.so is absent
    return functional


@pytest.fixture(scope="module")
def H():
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn_bf(shape, g):
    return torch.randn(shape, generator=g, device=DEV, dtype=BF16)


def nchw64(x):
    """NHWC (bf16) -> NCHW float64, contiguous."""
    return x.detach().permute(0, 3, 1, 2).to(F64).contiguous()


def as_nchw(x):
    return x.detach().permute(0, 3, 1, 2)


def f32(v):
    """The value a `float` argument of the C ABI carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# =================================================================================================
# A. optimizer
SGD_ROWS = [(0.9, 1.0, 1.0), (0.9, 1.0, 0.125), (0.0, 1.0, 0.5), (0.9, 0.0, 0.5)]
GUARD = 1024   # elements in front of and behind the arena: its base stays 16-byte aligned, as the kernel assumes


def seeded_grads(sizes, g, clip, scale, above, near, zero):
    """fp32 gradients per tensor: the tensors in `above` with ||g|| scale = 20 clip (clipped), the others 0.05 clip (not clipped),
    tensor `zero` all zeros, tensor `near` with ||g|| scale = 1.0005 clip (the minimum of the two branches is decided by 5e-4)."""
    c = clip if clip > 0 else 1.0
    out = []
    for t, n in enumerate(sizes):
        d = torch.randn(n, generator=g, device=DEV, dtype=F64)
        target = 20.0 * c if t in above else 0.05 * c
        if t == near:
            target = 1.0005 * c
        d = d * (target / (float(d.norm()) * scale))
        if t == zero:
            d = d * 0
        out.append(d.float())
    return torch.cat(out)


def check_sgd_step(name, sizes, got_p, got_m, p0, g, m0, wd, lr, mom, clip, scale):
    rp, rm = R.sgd_clip_ref(p0, g, m0, sizes, wd, lr, mom, clip, scale)
    ep, em = R.sgd_clip_bounds(p0, g, m0, sizes, wd, lr, mom, clip, scale, U)
    off = 0
    for t, n in enumerate(sizes):
        s = slice(off, off + n)
        check_vec("%s: m of tensor %d (%d elements at %d)" % (name, t, n, off), got_m[s], rm[s], em[s], 1e-4)
        check_vec("%s: p of tensor %d (%d elements at %d)" % (name, t, n, off), got_p[s], rp[s], ep[s], 1e-4)
        off += n


@pytest.mark.parametrize("mom,clip,scale", SGD_ROWS)
def test_sgd_clip_step_abi_vs_float64(H, mom, clip, scale):
    """u2_sgd_clip_step through the C ABI on hand-built chunk tables (float64_refs.chunk_tables restates FlatSGD's rule; the
    sizes and what each reaches are listed at A2_SIZES), the arena a slice [GUARD, GUARD + total) of larger buffers whose guard
    bands must stay bit-unchanged.  Three steps; the reference of step k starts from the kernel's own p, m after step k - 1, so
    the one-step bound applies to each.  `partial` is NaN before every step: with clip == 0 it must not be read, with clip > 0
    every entry a tensor sums must have been written.

    Reference (float64, the fp32 values of lr / mom / clip / scale / wd as the kernel receives them):
        coef = min(clip / (||g|| scale + 1e-6), 1) scale   (scale where clip == 0),   m' = mom m + g coef + wd p,   p' = p - lr m'
    Bound, per element:
        err(m') <= eps_c |g coef| + 4 u (|g coef| + |wd p| + |mom m|)
        err(p') <= lr err(m') + 2 u (|p| + lr |m'|)
      eps_c = (d / 2 + 4) u, d = float64_refs.sumsq_depth(chunks of the tensor) = 42 + chunks: n2 is a sum of non-negative terms
        through a chain of d roundings (relative error d u), the square root halves it; then sqrtf, `* grad_scale`, `+ 1e-6f`
        and the division round once each (4 u; the library is built without fast-math, so hipcc's sqrtf and fp32 division are
        correctly rounded).  fminf(., 1) does not increase an error.  With clip == 0 coef is the scalar
        itself: eps_c = 0.
      4 u: g coef passes `coef *= grad_scale`, the product, `+ wd p` and `+ momentum mm` (4 roundings); wd p its product and the
        two sums (3); mom m its product and the last sum (2).
      p': lr mm rounds once (u lr |m'|), the difference once (u |p'| <= u (|p| + lr |m'|)).
    A second call on identical inputs must give bit-identical p and m (the kernel promises clip coefficients that do not
    depend on scheduling: no atomics)."""
    sizes = R.A2_SIZES
    total = sum(sizes)
    ct, cb, cl, fc = R.chunk_tables(sizes)
    chunk_tensor = torch.tensor(ct, dtype=torch.int32, device=DEV)
    chunk_begin = torch.tensor(cb, dtype=torch.int64, device=DEV)
    chunk_len = torch.tensor(cl, dtype=torch.int32, device=DEV)
    first_chunk = torch.tensor(fc, dtype=torch.int32, device=DEV)
    wd_dev = torch.tensor([(0.0, 1e-4, 5e-2)[t % 3] for t in range(len(sizes))], dtype=torch.float32, device=DEV)
    wd = wd_dev.double().tolist()
    lr, mom, clip, scale = f32(0.1), f32(mom), f32(clip), f32(scale)
    g0 = gen(int(mom * 10) + int(scale * 1000) + int(clip))
    sentinel = torch.arange(total + 2 * GUARD, dtype=torch.int32, device=DEV) + 0x3F000000   # distinct floats near 0.5

    def buffer():
        b = torch.empty(total + 2 * GUARD, dtype=torch.float32, device=DEV)
        bits(b).copy_(sentinel)
        return b

    bufs = [buffer() for _ in range(3)]
    P, Gd, M = (b[GUARD: GUARD + total] for b in bufs)
    assert all(v.data_ptr() % 16 == 0 for v in (P, Gd, M))
    P.copy_(torch.randn(total, generator=g0, device=DEV))
    M.copy_(0.1 * torch.randn(total, generator=g0, device=DEV))
    partial = torch.empty(len(ct), dtype=torch.float32, device=DEV)

    def run(p, g, m):
        partial.fill_(NAN)
        H.call("u2_sgd_clip_step", p, g, m, chunk_tensor, chunk_begin, chunk_len, len(ct), partial, first_chunk, wd_dev, lr, mom,
               clip, scale)

    for k in range(3):
        g = seeded_grads(sizes, g0, clip, scale, above=(1, 3, 5, 7, 9), near=6, zero=2)   # 7: the four-chunk tensor
        Gd.copy_(g)
        p0, m0 = P.clone(), M.clone()
        if k == 0:   # the same step on copies, guards included: bit-identical
            twin = [b.clone() for b in bufs]
            run(*(b[GUARD: GUARD + total] for b in twin))
        run(P, Gd, M)
        if k == 0:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(twin, bufs)), "two runs on identical inputs differ"
        for b, nm in zip(bufs, "pgm"):
            assert torch.equal(bits(b)[:GUARD], sentinel[:GUARD]), "step %d wrote in front of the %s arena" % (k, nm)
            assert torch.equal(bits(b)[GUARD + total:], sentinel[GUARD + total:]), "step %d wrote behind the %s arena" % (k, nm)
        assert torch.equal(Gd, g), "the gradients were modified"
        if clip == 0:
            assert bool(partial.isnan().all()), "clip == 0: the partial sums were written"
        check_sgd_step("step %d" % k, sizes, P, M, p0, g, m0, wd, lr, mom, clip, scale)


def test_flat_sgd_step_vs_float64(H):
    """FlatSGD.step on a small module: normalisation layers, a 7-element bias followed by further parameters, a 75 000-element
    weight (two chunks).  Seeded gradients are written straight into the arena views; three steps of step(0.5), each checked
    against sgd_clip_ref from the arena's state before it, with the bound of test_sgd_clip_step_abi_vs_float64.  The
    per-parameter weight decay is the reference's rule (solver/build.py get_default_optimizer_params) restated here: a
    normalisation layer's parameters take WEIGHT_DECAY_NORM, a parameter named "bias" takes WEIGHT_DECAY_BIAS, applied last."""
    from u2seg_amd.layers.modules import BatchNorm2d, GroupNorm
    from u2seg_amd.solver import FlatSGD

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = BatchNorm2d(33)
            self.gn = GroupNorm(3, 9)
            self.small = torch.nn.Linear(300, 7)
            self.big = torch.nn.Linear(300, 250)

    torch.manual_seed(3)
    net = Net().to(DEV)
    g0 = gen(17)
    with torch.no_grad():
        for p in net.parameters():   # norm weights of 1 and biases of 0 would hide a wrong weight decay
            p.copy_(torch.randn(p.shape, generator=g0, device=DEV))
    lr0, wd_w, wd_n, wd_b, clip0 = 0.1, 1e-4, 0.0, 5e-2, 1.0
    opt = FlatSGD(net, lr=lr0, momentum=0.9, weight_decay=wd_w, weight_decay_norm=wd_n, weight_decay_bias=wd_b, clip_value=clip0)
    wd_of = {}
    for mod in net.modules():
        for pname, p in mod.named_parameters(recurse=False):
            v = wd_w
            if isinstance(mod, (BatchNorm2d, GroupNorm)):
                v = wd_n
            if pname == "bias":
                v = wd_b
            wd_of[id(p)] = f32(v)
    params = list(net.parameters())
    sizes = [p.numel() for p in params]
    assert sizes == [33, 33, 9, 9, 2100, 7, 75000, 250]
    wd = [wd_of[id(p)] for p in params]
    total = sum(sizes)
    # the chunk tables tile [0, total) without gap or overlap, no chunk crosses a tensor, first_chunk delimits each tensor's
    ct, cb, cl, fc = (t.tolist() for t in (opt.chunk_tensor, opt.chunk_begin, opt.chunk_len, opt.first_chunk))
    assert cb[0] == 0 and cb[-1] + cl[-1] == total and all(cb[i] + cl[i] == cb[i + 1] and cl[i] > 0 for i in range(len(cb) - 1))
    assert len(fc) == len(sizes) + 1 and fc[0] == 0 and fc[-1] == len(ct)
    starts = [sum(sizes[:t]) for t in range(len(sizes))]
    for t, s in enumerate(starts):
        assert fc[t] < fc[t + 1] and cb[fc[t]] == s
        for c in range(fc[t], fc[t + 1]):
            assert ct[c] == t and s <= cb[c] and cb[c] + cl[c] <= s + sizes[t] and cl[c] <= R.CHUNK
    assert fc[7] - fc[6] == 2
    assert (ct, cb, cl, fc) == R.chunk_tables(sizes)
    for p, s in zip(params, starts):   # parameters and gradients are views of the arena, in order
        assert p.data_ptr() == opt.flat_param.data_ptr() + 4 * s and p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * s
    lr, mom, clip, scale = f32(lr0), f32(0.9), f32(clip0), f32(0.5)
    for k in range(3):
        g = seeded_grads(sizes, g0, clip, scale, above=(1, 5, 6, 7), near=4, zero=3)   # 6: the two-chunk weight
        off = 0
        for p in params:
            p.grad.copy_(g[off: off + p.numel()].view(p.shape))
            off += p.numel()
        assert torch.equal(opt.flat_grad, g)
        p0, m0 = opt.flat_param.clone(), opt.flat_mom.clone()
        opt.step(0.5)
        got_p = torch.cat([p.detach().reshape(-1) for p in params])
        check_sgd_step("FlatSGD step %d" % k, sizes, got_p, opt.flat_mom, p0, g, m0, wd, lr, mom, clip, scale)


# =================================================================================================
# B. pooling and resampling
def pool_run(F, H, x):
    """y, idx and a backward closure: through functional.max_pool_3x3_s2 where its C % 32 == 0 contract admits the map, else
    the C ABI (C % 8 == 0) on NaN / 255-filled outputs."""
    b, h, w, c = x.shape
    if c % 32 == 0:
        xd = x.detach().requires_grad_(True)
        y = F.max_pool_3x3_s2(xd)
        idx = y.grad_fn.saved_tensors[0]

        def bwd(dy):
            y.backward(dy)
            return xd.grad
        return y.detach(), idx, bwd
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.full((b, ho, wo, c), NAN, dtype=BF16, device=DEV)
    idx = torch.full((b, ho, wo, c), 255, dtype=torch.uint8, device=DEV)
    H.call("u2_maxpool3x3s2_fwd", x, y, idx, b, h, w, c)

    def bwd(dy):
        dx = torch.full((b, h, w, c), NAN, dtype=BF16, device=DEV)
        H.call("u2_maxpool3x3s2_bwd", dy, idx, dx, b, h, w, c)
        return dx
    return y, idx, bwd


def check_pool(F, H, x, name, seed):
    """Forward: y bit-equal to max_pool2d, idx bit-equal to the slot of torch's return_indices (first maximum in scan order).
    Backward: float64 autograd; a pixel sums the dy of at most four windows in fp32 (3 additions: e = 3 u sum|terms|)."""
    w = x.shape[2]
    xr = nchw64(x).requires_grad_(True)
    yr, ind = TF.max_pool2d(xr, 3, 2, 1, return_indices=True)
    y, idx, bwd = pool_run(F, H, x)
    assert torch.equal(as_nchw(y).to(F64), yr.detach()), name + ": pooled values"
    assert torch.equal(as_nchw(idx), R.slots_from_indices(ind, w)), name + ": winner slots"
    gy = randn_bf(y.shape, gen(seed))
    dx = bwd(gy)
    (gr,) = torch.autograd.grad(yr, xr, nchw64(gy), retain_graph=True)
    (ga,) = torch.autograd.grad(yr, xr, nchw64(gy).abs())
    chk = Check(name + ": dx", 5e-3)
    chk.add(as_nchw(dx), gr, 3 * U * ga)
    chk.done()


POOL_SHAPES = [(2, 64, 13, 18), (1, 8, 1, 1), (1, 8, 2, 1), (3, 16, 1, 7), (2, 32, 14, 2), (1, 24, 5, 5)]   # (B, C, H, W)


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("ties", [False, True], ids=["randn", "ties"])
def test_max_pool_vs_float64(F, H, shape, ties):
    """Max pool 3x3 s2 p1: one-pixel, one-row, one-column, odd and even maps; `ties`: values on multiples of 0.5 in [-2, 0],
    so that most windows hold their maximum several times (the first in scan order must win) and many are all negative (the
    padding must never win)."""
    b, c, h, w = shape
    g = gen(h * 100 + w + c)
    if ties:
        x = R.tie_values((b, h, w, c), g, DEV).to(BF16)
    else:
        x = randn_bf((b, h, w, c), g)
    check_pool(F, H, x, "maxpool %s" % (shape,), h + w)


def upadd_run(F, H, lat, top):
    b, h, w, c = lat.shape
    if c % 32 == 0:
        ld, td = lat.detach().requires_grad_(True), top.detach().requires_grad_(True)
        out = F.fpn_upsample_add(ld, td)

        def bwd(dout):
            out.backward(dout)
            return ld.grad, td.grad
        return out.detach(), bwd
    out = torch.full((b, h, w, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_fpn_upsample_add_fwd", lat, top, out, b, h, w, c)
    return out, None


def upadd_bwd_run(H, dout):
    b, h, w, c = dout.shape
    dtop = torch.full((b, h // 2, w // 2, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_fpn_upsample_add_bwd", dout, dtop, b, h, w, c)
    return dtop


def check_upadd_fwd(out, lat, top, name):
    """out = bf16(lateral + nearest_x2(top)): one fp32 addition of two bf16 values, e = u |ref|."""
    ref = lat.to(F64) + top.to(F64).repeat_interleave(2, 1).repeat_interleave(2, 2)
    chk = Check(name + ": out", 4e-3)
    chk.add(out, ref, U * ref.abs())
    chk.done()


def check_upadd_dtop(dtop, dout, name):
    """dtop = bf16(fp32 sum of the 2 x 2 block of dout): three additions, e = 3 u sum|terms|."""
    b, h, w, c = dout.shape
    d6 = dout.to(F64).view(b, h // 2, 2, w // 2, 2, c)
    chk = Check(name + ": dtop", 5e-3)
    chk.add(dtop, d6.sum((2, 4)), 3 * U * d6.abs().sum((2, 4)))
    chk.done()


@pytest.mark.parametrize("shape", [(2, 64, 12, 16), (1, 8, 2, 2), (1, 256, 26, 42)])
def test_fpn_upsample_add_vs_float64(F, H, shape):
    b, c, h, w = shape
    g = gen(h * 100 + w)
    lat, top, dout = randn_bf((b, h, w, c), g), randn_bf((b, h // 2, w // 2, c), g), randn_bf((b, h, w, c), g)
    name = "upadd %s" % (shape,)
    out, bwd = upadd_run(F, H, lat, top)
    check_upadd_fwd(out, lat, top, name)
    if bwd is not None:
        dlat, dtop = bwd(dout)
        assert torch.equal(dlat, dout), name + ": the lateral's gradient is dout itself"
    else:
        dtop = upadd_bwd_run(H, dout)
    check_upadd_dtop(dtop, dout, name)


@pytest.mark.parametrize("h,w", [(3, 4), (4, 5), (1, 2)])
def test_fpn_upsample_add_refuses_odd_maps(F, H, h, w):
    """Odd H or W: the launchers answer -1, which `_hip.call` turns into a RuntimeError; nothing is written."""
    b, c = 1, 32
    g = gen(h + w)
    lat, top = randn_bf((b, h, w, c), g), randn_bf((b, max(h // 2, 1), max(w // 2, 1), c), g)
    out = torch.full((b, h, w, c), NAN, dtype=BF16, device=DEV)
    before = bits(out).clone()
    with pytest.raises(RuntimeError, match="status -1"):
        H.call("u2_fpn_upsample_add_fwd", lat, top, out, b, h, w, c)
    dtop = torch.full_like(top, NAN)
    before_t = bits(dtop).clone()
    with pytest.raises(RuntimeError, match="status -1"):
        H.call("u2_fpn_upsample_add_bwd", lat, dtop, b, h, w, c)
    torch.cuda.synchronize()
    assert torch.equal(bits(out), before) and torch.equal(bits(dtop), before_t)
    if top.shape[1:3] == (h // 2, w // 2):   # the wrapper hands the refusal on
        with pytest.raises(RuntimeError, match="status -1"):
            F.fpn_upsample_add(lat, top)


class per_pixel_kernel:
    """U2_BILINEAR_PER_PIXEL=1 for the calls inside: the launcher reads it per call."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("U2_BILINEAR_PER_PIXEL")
        if self.on:
            os.environ["U2_BILINEAR_PER_PIXEL"] = "1"
        else:
            os.environ.pop("U2_BILINEAR_PER_PIXEL", None)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("U2_BILINEAR_PER_PIXEL", None)
        else:
            os.environ["U2_BILINEAR_PER_PIXEL"] = self.old


def bilinear_run(F, H, x, add):
    b, h, w, c = x.shape
    if c % 32 == 0:
        xd = x.detach().requires_grad_(True)
        ad = add.detach().requires_grad_(True) if add is not None else None
        out = F.bilinear_up2(xd, ad)

        def bwd(dout):
            out.backward(dout)
            return xd.grad, (ad.grad if ad is not None else None)
        return out.detach(), bwd
    out = torch.full((b, 2 * h, 2 * w, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_bilinear_up2_fwd", x, add, out, b, h, w, c)
    return out, None


def bilinear_bwd_run(H, dout):
    b, h2, w2, c = dout.shape
    dx = torch.full((b, h2 // 2, w2 // 2, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_bilinear_up2_bwd", dout, dx, b, h2 // 2, w2 // 2, c)
    return dx


def up2(v):
    return TF.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)


def check_bilinear_fwd(out, x, add, name):
    """f = hy (hx v00 + lx v01) + ly (hx v10 + lx v11), the weights exact (0, 0.25, 0.75, 1): a tap passes at most two products
    and two sums, e = 6 u sum w |v| leaves room for both.  With an addend the kernel rounds f to bf16 first (the reference model's
    upsample returns a bf16 tensor) and adds in fp32, exactly (a sum of two bf16 values rounds once, as torch's bf16 add does):
    the chain is evaluated at both ends of [f - e, f + e] (Check.add_interval)."""
    xr = nchw64(x)
    yr, e = up2(xr), 6 * U * up2(xr.abs())
    got = as_nchw(out)
    if add is None:
        chk = Check(name + ": out", 4e-3)
        chk.add(got, yr, e)
    else:
        a32 = as_nchw(add).float()
        chain = lambda v: (v.to(BF16).float() + a32).to(BF16).to(F64)  # noqa: E731
        lo, hi = rnd(yr - e) + a32.to(F64), rnd(yr + e) + a32.to(F64)   # the sum before its last rounding, at both ends
        chk = Check(name + ": out", None)
        chk.add_interval(got, chain(yr - e), chain(yr + e), yr + a32.to(F64))
        # Two roundings lie between yr + add and the output, so the one-rounding bound 4e-3 of the largest element is taken
        # against the sum before its LAST rounding, the intermediate bf16 value being that of either end of the interval
        # (they differ on the few elements where [f - e, f + e] holds a rounding midpoint).
        err = torch.minimum((got.to(F64) - lo).abs(), (got.to(F64) - hi).abs())
        assert float(err.max()) <= 4e-3 * float(torch.maximum(lo.abs(), hi.abs()).max()), name
    chk.done()


def check_bilinear_bwd(dx, dout, name):
    """The transpose: an input pixel gathers at most 4 x 4 outputs, g += (wy wx) dout with wy wx exact: one product and at most
    16 sums per term, e = 20 u sum |w dout|.  Reference: float64 autograd of interpolate(scale 2, bilinear, ac=False)."""
    b, h2, w2, c = dout.shape
    xr = torch.zeros((b, c, h2 // 2, w2 // 2), dtype=F64, device=DEV, requires_grad=True)
    yr = up2(xr)
    d = nchw64(dout)
    (gr,) = torch.autograd.grad(yr, xr, d, retain_graph=True)
    (ga,) = torch.autograd.grad(yr, xr, d.abs())
    chk = Check(name + ": dx", 5e-3)
    chk.add(as_nchw(dx), gr, 20 * U * ga)
    chk.done()


@pytest.mark.parametrize("shape", [(2, 32, 7, 9), (1, 8, 1, 1), (3, 64, 1, 5), (2, 128, 12, 1), (1, 128, 25, 42)])
@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "addend"])
def test_bilinear_up2_vs_float64(F, H, shape, with_addend):
    """Both forward kernels (blocked, and per pixel through U2_BILINEAR_PER_PIXEL) and the backward on every shape."""
    b, c, h, w = shape
    g = gen(h * 50 + w + int(with_addend))
    x = randn_bf((b, h, w, c), g)
    add = randn_bf((b, 2 * h, 2 * w, c), g) if with_addend else None
    dout = randn_bf((b, 2 * h, 2 * w, c), g)
    name = "bilinear %s%s" % (shape, " + addend" if with_addend else "")
    with per_pixel_kernel(True):
        out_pp, _ = bilinear_run(F, H, x, add)
    check_bilinear_fwd(out_pp, x, add, name + " per pixel")
    with per_pixel_kernel(False):
        out, bwd = bilinear_run(F, H, x, add)
    check_bilinear_fwd(out, x, add, name + " blocked")
    if bwd is not None:
        dx, dadd = bwd(dout)
        if with_addend:
            assert torch.equal(dadd, dout), name + ": the addend's gradient is dout itself"
    else:
        dx = bilinear_bwd_run(H, dout)
    check_bilinear_bwd(dx, dout, name)


# ---- B4: more than 65 535 grid rows (every launcher caps grid.y there and loops) ----
def test_row_loop_max_pool(F, H):
    """B H = 131 100 input rows (backward), B Ho = 65 550 pooled rows (forward)."""
    x = randn_bf((3, 43700, 2, 8), gen(41))
    check_pool(F, H, x, "maxpool rows", 42)
    check_pool(F, H, R.tie_values(x.shape, gen(43), DEV).to(BF16), "maxpool rows, ties", 44)


def test_row_loop_bilinear_bwd(H):
    """B H = 131 100 rows of the input gradient."""
    dout = randn_bf((3, 87400, 4, 8), gen(45))
    check_bilinear_bwd(bilinear_bwd_run(H, dout), dout, "bilinear rows")


def test_row_loop_upadd_and_bilinear_fwd(F, H):
    """B H = 65 550 rows: the up-add forward; the per-pixel bilinear forward has B 2H = 131 100, the blocked one
    B (H + 1) = 65 553."""
    g = gen(46)
    b, h, w, c = 3, 21850, 2, 8
    lat, top = randn_bf((b, h, w, c), g), randn_bf((b, h // 2, w // 2, c), g)
    out, _ = upadd_run(F, H, lat, top)
    check_upadd_fwd(out, lat, top, "upadd rows")
    for add in (None, randn_bf((b, 2 * h, 2 * w, c), g)):
        for pp in (True, False):
            with per_pixel_kernel(pp):
                o, _ = bilinear_run(F, H, lat, add)
            check_bilinear_fwd(o, lat, add, "bilinear rows%s%s" % (" per pixel" if pp else " blocked", " + addend" if add is not None else ""))


def test_row_loop_upadd_bwd(H):
    """B H / 2 = 65 556 rows of the coarse level's gradient."""
    dout = randn_bf((3, 43704, 2, 8), gen(47))
    check_upadd_dtop(upadd_bwd_run(H, dout), dout, "upadd rows")


# ---- B5: the non-temporal max-pool backward ----
def check_pool_in_bands(x, dy, y, idx, dx, band):
    """check_pool's comparisons for a map too large for one float64 pass, in bands of `band` (even) input rows of a one-image
    map: the band's rows with one more row on each side (-inf where that is the padding) hold every window that touches the
    band; forward values and slots are compared on those windows, the gradient on the band's own rows."""
    b, h, w, c = x.shape
    ho = (h - 1) // 2 + 1
    assert b == 1 and band % 2 == 0
    chk = Check("maxpool nt: dx", 5e-3)
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        o_lo, o_hi = r0 // 2, min(ho - 1, r1 // 2)            # the windows that touch rows r0 .. r1 - 1
        a, z = 2 * o_lo - 1, 2 * o_hi + 1                     # their first and last input row
        slab = nchw64(x[:, max(a, 0): min(z, h - 1) + 1])
        slab = TF.pad(slab, (0, 0, int(a < 0), int(z > h - 1)), value=float("-inf")).requires_grad_(True)
        yr, ind = TF.max_pool2d(slab, 3, 2, (0, 1), return_indices=True)
        assert yr.shape[2] == o_hi - o_lo + 1
        assert torch.equal(as_nchw(y[:, o_lo: o_hi + 1]).to(F64), yr.detach()), "maxpool nt: pooled values, rows from %d" % r0
        assert torch.equal(as_nchw(idx[:, o_lo: o_hi + 1]), R.slots_from_indices(ind, w, row_off=0)), "maxpool nt: slots, rows from %d" % r0
        gy = nchw64(dy[:, o_lo: o_hi + 1])
        (gr,) = torch.autograd.grad(yr, slab, gy, retain_graph=True)
        (ga,) = torch.autograd.grad(yr, slab, gy.abs())
        chk.add(as_nchw(dx[:, r0:r1]), gr[:, :, r0 - a: r1 - a], 3 * U * ga[:, :, r0 - a: r1 - a])
        del slab, yr, ind, gy, gr, ga
    chk.done()
    assert chk.n == dx.numel()


def test_max_pool_bwd_nontemporal(H):
    """maxpool_bwd_kernel<true> on the smallest map above the launcher's 256 MB switch (1 x 1026 x 2048 x 64: 16 809 984
    16-byte items against 16 777 216).  The float64 reference runs on the device in bands of 128 input rows (check_pool_in_bands, the bound
    of check_pool).  The same dy / idx run
    as two half-height calls (maxpool_bwd_kernel<false>: 8 M items each) must give the bit-identical gradient wherever a half
    holds all windows of a row: rows 0 .. 510 and 514 .. 1025."""
    b, h, w, c = 1, 1026, 2048, 64
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert b * h * w * (c // 8) * 16 > 256 << 20 and (h // 2) * w * (c // 8) * 16 <= 256 << 20
    g = gen(51)
    x = randn_bf((b, h, w, c), g)
    dy = randn_bf((b, ho, wo, c), g)
    y = torch.full((b, ho, wo, c), NAN, dtype=BF16, device=DEV)
    idx = torch.full((b, ho, wo, c), 255, dtype=torch.uint8, device=DEV)
    dx = torch.full((b, h, w, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_maxpool3x3s2_fwd", x, y, idx, b, h, w, c)
    H.call("u2_maxpool3x3s2_bwd", dy, idx, dx, b, h, w, c)
    check_pool_in_bands(x, dy, y, idx, dx, 128)
    half = h // 2 - 1                                         # 512 rows: windows 0 .. 255 / 257 .. 512
    hh = half // 2
    top = torch.full((b, half, w, c), NAN, dtype=BF16, device=DEV)
    bot = torch.full((b, half, w, c), NAN, dtype=BF16, device=DEV)
    H.call("u2_maxpool3x3s2_bwd", dy[:, :hh], idx[:, :hh], top, b, half, w, c)
    H.call("u2_maxpool3x3s2_bwd", dy[:, ho - hh:], idx[:, ho - hh:], bot, b, half, w, c)
    assert torch.equal(bits(top[:, : half - 1]), bits(dx[:, : half - 1]))
    assert torch.equal(bits(bot), bits(dx[:, h - half:]))


# ---- B6: the stem's input ----
PIXEL_MEAN, PIXEL_STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
GUARD_ROWS = 8


def stem_images(sizes, u8, g):
    if u8:
        return [torch.randint(0, 256, (3, h, w), generator=g, device=DEV, dtype=torch.uint8) for h, w in sizes]
    return [255 * torch.rand((3, h, w), generator=g, device=DEV, dtype=torch.float32) for h, w in sizes]


def stem_col(rows, kp):
    return torch.full((rows + GUARD_ROWS, kp), NAN, dtype=BF16, device=DEV)


def stem_batch(H, imgs, mean, std, col, hpad, wpad, kp):
    n = len(imgs)
    ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in imgs])
    hs = (ctypes.c_int * n)(*[im.shape[1] for im in imgs])
    ws = (ctypes.c_int * n)(*[im.shape[2] for im in imgs])
    H.call("u2_stem_im2col_batch", ptrs, hs, ws, n, int(imgs[0].dtype == torch.uint8), mean, std, col, hpad, wpad, kp)


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float32"])
@pytest.mark.parametrize("case", ["ragged", "batch33"])
def test_stem_im2col_vs_float64(H, case, u8):
    """u2_stem_im2col_batch and u2_stem_im2col, direct.  Reference: unfold(7, stride 2, pad 3) of (img - mean) / std in float64
    on the zero canvas, columns reordered to (kh, kw, c) (float64_refs.stem_unfold_ref).  The kernel's fp32 (img - mean) / std
    is within a few u of it, far below a bf16 step, so each stored value is rnd(ref) or - where the fp32 value falls on the other
    side of a rounding midpoint - its neighbour: |got - rnd(ref)| <= one bf16 step at |ref|, and exactly 0 where ref is 0:
    canvas pixels outside the image, the conv padding, columns 147 .. KP - 1.
    ragged: four images on a 64 x 96 canvas (32 x 48 output pixels: the second tile column is half empty, images end inside a
    tile, one image is a single pixel).  batch33: 33 images of 8 x 8 on a 16 x 32 canvas: image 32 goes through the second launch
    of the 32-image split and its rows must land at slot 32.  The single-slot entry must reproduce the batch entry's rows bit
    for bit; rows behind the last image stay untouched."""
    kp = 160
    g = gen(61 + int(u8))
    if case == "ragged":
        sizes, hpad, wpad = [(50, 70), (64, 61), (1, 1), (16, 32)], 64, 96
    else:
        sizes, hpad, wpad = [(8, 8)] * 33, 16, 32
    imgs = stem_images(sizes, u8, g)
    mean, std = torch.tensor(PIXEL_MEAN, device=DEV), torch.tensor(PIXEL_STD, device=DEV)
    n, ho, wo = len(imgs), hpad // 2, wpad // 2
    rows = n * ho * wo
    col = stem_col(rows, kp)
    untouched = bits(col).clone()
    stem_batch(H, imgs, mean, std, col, hpad, wpad, kp)
    assert torch.equal(bits(col)[rows:], untouched[rows:]), "rows behind the last image were written"
    canvas, inside = R.stem_canvas(imgs, mean, std, hpad, wpad)
    ref, ins = R.stem_unfold_ref(canvas), R.stem_unfold_ref(inside)
    got = col[:rows].view(n, ho * wo, kp)
    chk = Check("stem im2col %s" % case, 4e-3)
    chk.add(got[..., :147], ref, torch.zeros_like(ref))
    chk.done()
    assert bool((bits(got[..., 147:]) == 0).all()), "columns 147 .. KP - 1 are not zero"
    assert bool((bits(got[..., :147])[ins == 0] == 0).all()), "padding or pixels outside the image are not zero"
    if case == "batch33":   # every image is different, so a row block at the wrong slot cannot pass; say so explicitly for slot 32
        assert not torch.equal(got[32], got[0])
    single = stem_col(rows, kp)
    for i, im in enumerate(imgs):
        H.call("u2_stem_im2col", im, int(u8), mean, std, single, i, im.shape[1], im.shape[2], hpad, wpad, kp)
    assert torch.equal(bits(single), bits(col)), "u2_stem_im2col differs from the batch entry"


@pytest.mark.parametrize("kp", [146, 150, 544])
def test_stem_im2col_refuses_bad_kp(H, kp):
    """KP below 147, not a multiple of 32, above 512: -1 from both entries, nothing written."""
    imgs = stem_images([(8, 8)], True, gen(63))
    mean, std = torch.tensor(PIXEL_MEAN, device=DEV), torch.tensor(PIXEL_STD, device=DEV)
    col = stem_col(8 * 16, 544)
    before = bits(col).clone()
    with pytest.raises(RuntimeError, match="status -1"):
        stem_batch(H, imgs, mean, std, col, 16, 32, kp)
    with pytest.raises(RuntimeError, match="status -1"):
        H.call("u2_stem_im2col", imgs[0], 1, mean, std, col, 0, 8, 8, 16, 32, kp)
    torch.cuda.synchronize()
    assert torch.equal(bits(col), before)


# ---- B7: weight gradients into the arena ----
@pytest.mark.parametrize("n,cin,t,cp", [(40, 24, 9, 32), (256, 256, 9, 256), (64, 3, 49, 32)])
def test_wgrad_permute_add_exact(H, n, cin, t, cp):
    """grad[n][c][t] += scratch[n][t][c]: one fp32 addition per element, so the result is bit-equal to torch's fp32 sum.  The
    scratch holds more rows than N and Cp >= Cin channels, NaN beyond N and Cin (Cin < Cp only): none may leak; the arena
    behind the N rows stays untouched."""
    g = gen(n + cin + t)
    npad = n + 24
    scratch = torch.randn((npad, t, cp), generator=g, device=DEV)
    scratch[n:] = NAN
    scratch[:, :, cin:] = NAN
    guard = 512
    arena = torch.randn(n * cin * t + guard, generator=g, device=DEV)
    prior = arena.clone()
    H.call("u2_wgrad_permute_add", scratch, arena, n, cin, t, cp)
    want = prior[: n * cin * t].view(n, cin, t) + scratch[:n, :, :cin].permute(0, 2, 1)
    assert not bool(want.isnan().any())
    assert torch.equal(bits(arena[: n * cin * t]), bits(want.contiguous().view(-1)))
    assert torch.equal(bits(arena[n * cin * t:]), bits(prior[n * cin * t:]))
