"""The convolution family (conv_igemm.hip, conv_tile.hip, conv_halo.hip, conv_stream.hip, conv_wgrad.hip, wgrad_halo.hip, wgrad_stream.hip and
the fused 1x1 backward) per element against float64 - tests/test_gpu_kernel_variants.py holds the same kernels to 4e-3 of the
LARGEST element of a mean-zero result, which passes truncation for rounding, a bf16 hand-over of a partial tile and a dropped
product with small factors.

Two kinds of check, every element of every output, none masked out (references: tests/float64_refs.py, unfold + matmul in float64
on the CPU, checked against torch's conv2d and its autograd by tests/test_float64_refs_host.py):

A. exact inputs, zero tolerance.  Operands are small integers (bf16 values).  Every product and every partial sum is then an
   integer; the reference also forms A = sum |term| and the test asserts max A < 2^24, so every partial sum in ANY order - split K,
   stream-K hand-over, atomics - is an fp32 value and the fp32 sum is the exact integer.  The stored bf16 output must equal
   RNE_bf16(exact sum) bit for bit (amplitudes by float64_refs.exact_amp put a good share of the sums past 256, where bf16 no
   longer holds every integer: the share is asserted), fp32 weight / bias gradients and the column sum of the BN statistics must
   equal the integer; the sum of squares too wherever it stays below 2^24 (asserted on a low-amplitude launch), bound B otherwise.

B. activation-like inputs, derived interval.  x = relu(N(mu_c, 1)) with channel means from {0, 1, 4}, an all-zero channel and a
   channel with a few 2^6; filters N(0, 1/K) plus a per-filter offset; gradients N(0, 1) 2^-10.  The products of two bf16 values
   are exact in fp32 (16-bit significands), so the only error of the kernel's value is that of adding L terms in fp32: every one
   of the L - 1 additions rounds a partial sum of magnitude <= A = sum |term| by at most u = 2^-24 relative, in any order; with
   the bias add and the epilogue that is E = (L + 2) 2^-24 A (float64_refs.fp32_sum_bound; L = taps Cin forward, taps Cout data
   gradient, B Hout Wout weight / bias gradient and statistics).  fp32 outputs: |got - ref| <= E.  bf16 outputs: rounding is
   monotone, so the stored value lies in [RNE_bf16(ref - E), RNE_bf16(ref + E)], with the ReLU and the accumulating epilogue's
   second rounding applied to both ends.  No threshold comes from the code under test; each test prints the largest |err| / E it
   saw (fp32 outputs) and the share of bf16 outputs equal to RNE_bf16(ref) as information.

Every forced case asserts u2_conv_last_kernel (or the fused launchers' return value): the intended kernel really ran."""
import functools

import pytest
import torch

from tests import float64_refs as R
from tests.conv_variants import (CONV_VARIANTS, HALO, K, NEVER_TILE, STREAM, TINY, WGRAD_HALO_VARIANTS, WGRAD_TAP_VARIANTS, WS_FORCE,
                                 forced, igemm_code, last_kernel, stream_code, ws_variant)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
MODES = ["exact", "real"]


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()
    return functional


def ceil32(n):
    return (n + 31) // 32 * 32


def dev_act(t):
    """float64 [B, C, H, W] holding bf16 values -> NHWC bf16 on the device, channels zero padded to a multiple of 32."""
    b, c, h, w = t.shape
    out = torch.zeros((b, h, w, ceil32(c)), dtype=BF16, device=DEV)
    out[..., :c] = t.permute(0, 2, 3, 1).to(BF16)
    return out


def host_act(t, c):
    """NHWC device tensor -> float64 [B, c, H, W] on the CPU, and the largest magnitude in the padded channels."""
    pad = float(t[..., c:].float().abs().max()) if t.shape[3] > c else 0.0
    return t[..., :c].permute(0, 3, 1, 2).to(F64).cpu(), pad


def report(name, what, value):
    print("CONV64 %s | %s | %.4g" % (name, what, value))


def check_bf16(name, got, ref, a, length, mode, relu=False, old=None):
    """A bf16 output against float64: bit for bit (exact) or inside the derived interval (real).  All elements."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if mode == "exact":
        assert float(a.max()) < R.TWO24, (name, "precondition: sum |term| = %g" % float(a.max()))
        lo, hi = R.bf16_interval(ref, torch.zeros_like(ref), relu, old)
        assert torch.equal(lo, hi)
    else:
        lo, hi = R.bf16_interval(ref, R.fp32_sum_bound(length, a), relu, old)
        mid = R.bf16_interval(ref, torch.zeros_like(ref), relu, old)[0]
        report(name, "share of outputs equal to RNE_bf16(ref)", float((got == mid).double().mean()))
    bad = (got < lo) | (got > hi) | ~torch.isfinite(got)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside [lo, hi]; first at %s: got %r, lo %r, hi %r, ref %r" % (
            name, int(bad.sum()), bad.numel(), i, float(got[i]), float(lo[i]), float(hi[i]), float(ref[i])))


def check_f32(name, got, ref, a, length, mode):
    """An fp32 output against float64: equal (exact) or within E (real).  All elements.  On the reference's device."""
    got = got.to(F64).to(ref.device)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if mode == "exact":
        assert float(a.max()) < R.TWO24, (name, "precondition: sum |term| = %g" % float(a.max()))
        e = torch.zeros_like(ref)
    else:
        e = R.fp32_sum_bound(length, a)
        err = (got - ref).abs()
        report(name, "max |err| / E", float((err[e > 0] / e[e > 0]).max()) if bool((e > 0).any()) else 0.0)
    bad = ((got - ref).abs() > e) | ~torch.isfinite(got)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond E; first at %s: got %r, ref %r, E %r" % (
            name, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(e[i])))


def check_stats(name, stats, y, mode, need_exact_squares=False, depth=None):
    """[sum | sum of squares] over the STORED outputs y (float64 [B, N, H, W] of bf16 values; y^2 is an fp32 value).
    depth: the longest chain of fp32 additions behind a column sum by the launch geometry (float64_refs.stream_stats_depth), for
    maps with so many pixels that sum |y| passes 2^24 at the exact generator's amplitudes (which are chosen for the outputs'
    rounding).  Recursive summation over chains of length d errs by at most d u sum |term|, so both rows are then held to
    (depth + 2) 2^-24 sum |term| instead of (pixels + 2) 2^-24 sum |term| - in both modes - and the column sum stays exact
    wherever its own sum |y| is below 2^24."""
    m = y.shape[0] * y.shape[2] * y.shape[3]
    s0, a0, s1 = y.sum((0, 2, 3)), y.abs().sum((0, 2, 3)), (y * y).sum((0, 2, 3))
    if depth is not None:
        assert depth < m
        small = a0 < R.TWO24
        if mode == "exact" and bool(small.any()):
            check_f32(name + " stats[0] (columns below 2^24)", stats[0][small.to(stats.device)], s0[small], a0[small], depth, "exact")
        check_f32(name + " stats[0]", stats[0], s0, a0, depth, "real")
        check_f32(name + " stats[1]", stats[1], s1, s1, depth, "real")
        return
    check_f32(name + " stats[0]", stats[0], s0, a0, m, mode)
    squares_exact = mode == "exact" and float(s1.max()) < R.TWO24
    if need_exact_squares:
        assert squares_exact, (name, "precondition: sum y^2 = %g" % float(s1.max()))
    check_f32(name + " stats[1]", stats[1], s1, s1, m, "exact" if squares_exact else "real")


@functools.lru_cache(maxsize=3)
def plain_refs(geom, mode, amp=None):
    """Operands and the float64 references of the plain leg (no bias, no ReLU), computed once per case and shared."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    x, wt, bias, gy, old = R.conv_operands(geom, mode, amp)
    return dict(x=x, w=wt, bias=bias, gy=gy, old=old,
                y=R.conv_fwd_ref(x, wt, stride, ph, pw), yb=R.conv_fwd_ref(x, wt, stride, ph, pw, bias),
                dx=R.conv_dgrad_ref(gy, wt, (h, w), stride, ph, pw), dw=R.conv_wgrad_ref(x, gy, kh, kw, stride, ph, pw))


def code_ok(expected):
    """u2_conv_last_kernel against a code, or against a family given as a predicate."""
    return expected(last_kernel()) if callable(expected) else last_kernel() == expected


def igemm_family(code):
    """conv_igemm_kernel<BK, GLDS, TM, TN, NST> (igemm_code): what is left when the persistent tile kernels are forbidden."""
    return code >= igemm_code(32, 128, 128, 2, 0)


def big_share(ref):
    return float((ref.abs() > 256).double().mean())


def run_layer(F, geom, mode, conv=None, wgrad=None, fwd_code=None, wgrad_code=None, stats=True, bias_leg="full", linear=False,
              name=""):
    """One layer through the product path (_Conv2dFn / F.linear): forward with statistics, data gradient and weight gradient;
    then with bias + ReLU (bias_leg "full": forward and all gradients incl. the bias', "fwd": forward only, None: skipped)."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    assert ph == pw, "the product path pads both axes alike"
    ho, wo = R.conv_out_size(h, w, kh, kw, stride, ph, pw)
    m, taps = b * ho * wo, kh * kw
    r = plain_refs(geom, mode)
    name = "%s %s %s" % (name, geom, mode)
    if mode == "exact" and taps * cin >= 32:
        # rounding and ties of the store are really exercised: the generator aims at a standard deviation of 512 over the terms
        # inside the map, P(|N(0, 512)| > 256) = 0.62; border pixels have fewer terms
        assert big_share(r["y"][0]) > 0.25, (name, big_share(r["y"][0]))
    xd = dev_act(r["x"]).requires_grad_(True)
    wd = r["w"].float().to(DEV).requires_grad_(True)
    gyd = dev_act(r["gy"])

    def apply(x_, w_, bias_, relu, want_stats):
        if linear:
            return F.linear(x_.view(h, x_.shape[3]), w_.view(cout, cin), bias_, relu).view(1, h, 1, -1), None
        return F._Conv2dFn.apply(x_, w_, bias_, stride, ph, relu, want_stats)

    with forced(conv=conv, wgrad=wgrad):
        y, st = apply(xd, wd, None, False, stats)
        if fwd_code is not None:
            assert code_ok(fwd_code), (name, "forward ran kernel %d, expected %s" % (last_kernel(), fwd_code))
        y.backward(gyd)
        F.join_all_streams()
        if wgrad_code is not None:
            assert last_kernel() == wgrad_code, (name, "wgrad ran kernel %d, expected %d" % (last_kernel(), wgrad_code))
    yy, pad = host_act(y, cout)
    assert pad == 0.0, name
    check_bf16(name + " fwd", yy, r["y"][0], r["y"][1], taps * cin, mode)
    if stats:
        check_stats(name, st, yy, mode)
    dx, pad = host_act(xd.grad, cin)
    assert pad == 0.0, name
    check_bf16(name + " dgrad", dx, r["dx"][0], r["dx"][1], taps * cout, mode)
    check_f32(name + " wgrad", wd.grad, r["dw"][0], r["dw"][1], m, mode)
    if bias_leg is None:
        return
    bd = r["bias"].float().to(DEV).requires_grad_(bias_leg == "full")
    xd2 = dev_act(r["x"]).requires_grad_(bias_leg == "full")
    wd2 = r["w"].float().to(DEV).requires_grad_(bias_leg == "full")
    with forced(conv=conv, wgrad=wgrad), torch.set_grad_enabled(bias_leg == "full"):
        y2, _ = apply(xd2, wd2, bd, True, False)
        if fwd_code is not None:
            assert code_ok(fwd_code), (name, last_kernel(), fwd_code)
        if bias_leg == "full":
            y2.backward(gyd)
            F.join_all_streams()
    out, pad = host_act(y2, cout)
    assert pad == 0.0, name
    check_bf16(name + " fwd bias relu", out, r["yb"][0], r["yb"][1], taps * cin, mode, relu=True)
    if bias_leg != "full":
        return
    # the backward kernels read the STORED output's sign: the reference gradient is masked with it
    dz = r["gy"] * (out > 0)
    ref_dx = R.conv_dgrad_ref(dz, r["w"], (h, w), stride, ph, pw)
    ref_dw = R.conv_wgrad_ref(r["x"], dz, kh, kw, stride, ph, pw)
    dx, pad = host_act(xd2.grad, cin)
    assert pad == 0.0, name
    check_bf16(name + " dgrad relu", dx, ref_dx[0], ref_dx[1], taps * cout, mode)
    check_f32(name + " wgrad relu", wd2.grad, ref_dw[0], ref_dw[1], m, mode)
    check_f32(name + " bias grad", bd.grad, dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3)), m, mode)


def low_amplitude_statistics(F, geom, conv, code, name):
    """Integers in {-1, 0, 1}: the column sums of squares stay below 2^24 as well, so BOTH statistics rows are exact."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    x, wt, _, _, _ = R.conv_operands(geom, "exact", amp=1)
    with forced(conv=conv), torch.no_grad():
        y, st = F._Conv2dFn.apply(dev_act(x), wt.float().to(DEV), None, stride, ph, False, True)
        assert last_kernel() == code, (name, last_kernel(), code)
    ref, a = R.conv_fwd_ref(x, wt, stride, ph, pw)
    yy, _ = host_act(y, cout)
    check_bf16(name + " low amplitude fwd", yy, ref, a, kh * kw * cin, "exact")
    check_stats(name + " low amplitude", st, yy, "exact", need_exact_squares=True)


# ---- 1. every forward instantiation ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant,code", CONV_VARIANTS)
@pytest.mark.parametrize("geom", R.VARIANT_SHAPES)
def test_forward_instantiations(F, geom, variant, code, mode):
    """All of CONV_VARIANTS (igemm rings and tiles, igemm256 plain / staggered, conv_tile configurations 1-6 with and without the
    8-work-group grid, the stream-K forms, conv_halo) on 3x3 64 -> 256 over 2 x 36 x 32 (nine 256-pixel tiles) and 2 x 35 x 31 (a
    partial last tile: stream-K shares end inside it): forward + statistics, bias + ReLU forward, data gradient (through the same
    forced launcher) and weight gradient."""
    run_layer(F, geom, mode, conv=variant, fwd_code=code, bias_leg="fwd", name="variant %#x" % variant)
    if mode == "exact":
        low_amplitude_statistics(F, geom, variant, code, "variant %#x" % variant)


# ---- 2. generic path geometry ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("never_tile", [False, True])
@pytest.mark.parametrize("geom", R.GENERIC_GEOMS)
def test_generic_geometry(F, geom, never_tile, mode):
    """1x1 / 3x3 / 5x5 / 7x7, strides 1 and 2, on one-pixel, one-row, one-column, odd and even maps, through the automatic
    dispatch and with the persistent tile kernels forbidden (conv_igemm_kernel: asserted); all gradients incl. bias + ReLU."""
    run_layer(F, geom, mode, conv=NEVER_TILE if never_tile else None, fwd_code=igemm_family if never_tile else None, name="generic")


def abi_conv(F, x, wt, geom, bias=None, relu=False, old=None, want_stats=False, variant=0):
    """u2_conv_igemm through the C ABI (forward of `geom`).  Returns (out NHWC, stats)."""
    from u2seg_amd import _hip

    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    ho, wo = R.conv_out_size(h, w, kh, kw, stride, ph, pw)
    xd = dev_act(x)
    cp, npad = xd.shape[3], ceil32(cout)
    wk = F.weight_fwd_layout(wt.float().to(DEV), cp)
    out = dev_act(old) if old is not None else torch.zeros((b, ho, wo, npad), dtype=BF16, device=DEV)
    st = torch.zeros((2, cout), dtype=torch.float32, device=DEV) if want_stats else None
    _hip.call("u2_conv_igemm", xd, wk, out, None if bias is None else bias.float().to(DEV), st, b, h, w, cp, cp, ho, wo, cout, npad,
              kh, kw, ph, pw, stride, 1, int(relu), int(old is not None), variant)
    return out, st


def abi_dgrad(F, dz, wt, geom, bias=None, relu=False, old=None, variant=0):
    """The data gradient of `geom` as _Conv2dFn.backward launches it (flipped, transposed filter; div = stride), with the
    epilogue options the product path never combines with it.  Returns dx NHWC."""
    from u2seg_amd import _hip

    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    ho, wo = R.conv_out_size(h, w, kh, kw, stride, ph, pw)
    dzd = dev_act(dz)
    cp, npad = ceil32(cin), dzd.shape[3]
    wdl = F.weight_dgrad_layout(wt.float().to(DEV), cp, npad)
    dx = dev_act(old) if old is not None else torch.zeros((b, h, w, cp), dtype=BF16, device=DEV)
    bias_f = None
    if bias is not None:
        bias_f = torch.zeros(cp, dtype=torch.float32, device=DEV)
        bias_f[:cin] = bias.float().to(DEV)
    _hip.call("u2_conv_igemm", dzd, wdl, dx, bias_f, None, b, ho, wo, npad, npad, h, w, cp, cp, kh, kw, kh - 1 - ph, kw - 1 - pw, 1,
              stride, int(relu), int(old is not None), variant)
    return dx


def abi_wgrad(F, x, dz, geom, variant=0):
    from u2seg_amd import _hip

    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    ho, wo = R.conv_out_size(h, w, kh, kw, stride, ph, pw)
    xd, dzd = dev_act(x), dev_act(dz)
    cp, npad = xd.shape[3], dzd.shape[3]
    dwk = torch.zeros((npad, kh * kw, cp), dtype=torch.float32, device=DEV)
    _hip.call("u2_conv_wgrad", xd, dzd, dwk, b, h, w, cp, cp, ho, wo, npad, npad, kh, kw, ph, pw, stride, variant)
    assert float(dwk[cout:].abs().max()) == 0.0 if npad > cout else True
    return dwk[:cout, :, :cin].view(cout, kh, kw, cin).permute(0, 3, 1, 2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", [0, NEVER_TILE])
def test_asymmetric_filter_through_the_abi(F, variant, mode):
    """KH != KW with pad_h != pad_w, which include/u2seg_hip.h documents: a 1x3 filter with padding (0, 1) - forward with bias +
    ReLU and statistics, data gradient and weight gradient through the C ABI (the product path only has square filters)."""
    geom = R.ASYM_GEOM
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    x, wt, bias, gy, _ = R.conv_operands(geom, mode)
    m = b * h * w
    y, st = abi_conv(F, x, wt, geom, want_stats=True, variant=variant)
    ref, a = R.conv_fwd_ref(x, wt, stride, ph, pw)
    yy, pad = host_act(y, cout)
    assert pad == 0.0
    check_bf16("1x3 fwd", yy, ref, a, kh * kw * cin, mode)
    check_stats("1x3", st, yy, mode)
    yb, _ = abi_conv(F, x, wt, geom, bias=bias, relu=True, variant=variant)
    ref, a = R.conv_fwd_ref(x, wt, stride, ph, pw, bias)
    check_bf16("1x3 fwd bias relu", host_act(yb, cout)[0], ref, a, kh * kw * cin, mode, relu=True)
    dx = abi_dgrad(F, gy, wt, geom, variant=variant)
    ref, a = R.conv_dgrad_ref(gy, wt, (h, w), stride, ph, pw)
    check_bf16("1x3 dgrad", host_act(dx, cin)[0], ref, a, kh * kw * cout, mode)
    ref, a = R.conv_wgrad_ref(x, gy, kh, kw, stride, ph, pw)
    check_f32("1x3 wgrad", abi_wgrad(F, x, gy, geom), ref, a, m, mode)


# ---- 3. stride-2 data gradient (div = 2) ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", R.STRIDE2_GEOMS)
def test_stride2_data_gradient_parity_classes(F, geom, mode):
    """The data gradient of a stride-2 layer runs one launch per parity class of the input map (conv_api.hip:u2_conv_igemm,
    div = 2): maps of 1 x 1, 1 x 2 and 2 x 1 pixels (classes with py >= Hout / px >= Wout), 7 x 9 and 8 x 10; 1x1 / pad 0 (three
    classes meet no tap: one zero-fill launch, N % 8 == 0) and 3x3 / pad 1; through the product path, and through the C ABI with
    a bias + ReLU and with the accumulating epilogue onto a non-zero map (every class then keeps its own launch)."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    run_layer(F, geom, mode, bias_leg=None, name="stride 2")
    x, wt, bias, gy, _ = R.conv_operands(geom, mode)
    ref, a = R.conv_dgrad_ref(gy, wt, (h, w), stride, ph, pw)
    g = torch.Generator().manual_seed(h * 16 + w)
    if mode == "exact":
        dbias, old = R.ints((cin,), 64, g), R.ints((b, cin, h, w), 64, g)
    else:
        dbias = R.bf16_round(torch.randn((cin,), generator=g, dtype=F64) * 2.0 ** -10)
        old = R.bf16_round(torch.randn((b, cin, h, w), generator=g, dtype=F64) * 2.0 ** -8)
    dx = abi_dgrad(F, gy, wt, geom, bias=dbias, relu=True)
    check_bf16("stride 2 dgrad bias relu", host_act(dx, cin)[0], ref + dbias.view(1, cin, 1, 1), a + dbias.abs().view(1, cin, 1, 1),
               kh * kw * cout, mode, relu=True)
    dx = abi_dgrad(F, gy, wt, geom, old=old)
    check_bf16("stride 2 dgrad accumulate", host_act(dx, cin)[0], ref, a, kh * kw * cout, mode, old=old)


# ---- 4. conv_halo ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tiny", [0, 1])
@pytest.mark.parametrize("geom", R.HALO_GEOMS)
def test_conv_halo_patches(F, geom, tiny, mode):
    """conv_halo.hip (16 x 32 pixel patches, forced): a map inside one patch, exactly one patch, one pixel over on each axis, and
    33 x 65; 128-channel tiles (K_HALO) and the 64-channel tiles (K_HALO_N64), ragged channel tails; all gradients."""
    code = K.K_HALO_N64 if geom[4] <= 64 else K.K_HALO
    variant = HALO | (TINY if tiny else 0)
    run_layer(F, geom, mode, conv=variant, fwd_code=code, name="halo tiny %d" % tiny)
    if mode == "exact":
        low_amplitude_statistics(F, geom, variant, code, "halo")


# ---- 5. conv_stream ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", R.STREAM_GEOMS)
def test_conv_stream_ring(F, geom, mode):
    """conv_stream.hip (1x1, pixel rows through the LDS ring, forced): one pixel, 63 pixels, and - on the 8-work-group grid -
    one pixel short of and one pixel past the point where every walker's ring is full (float64_refs.stream_pixel_counts)."""
    cin, cout, m = geom[3], geom[4], geom[2]
    code = stream_code(cin, cout)
    variant = STREAM | (TINY if m > 63 else 0)
    run_layer(F, geom, mode, conv=variant, fwd_code=code, bias_leg="fwd", name="stream")


def stream_forward_on_device(F, geom, mode, variant, code, name):
    """run_layer's forward legs - plain with the fused statistics, bias + ReLU - with the operands drawn on the host as ever and the
    float64 references formed on the device: an output of these cases has up to 10^8 elements.  1x1 / stride 1 only."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    assert (kh, kw, stride, ph, pw) == (1, 1, 1, 0, 0)
    name = "%s %s %s" % (name, geom, mode)
    x, wt, bias, _, _ = R.conv_operands(geom, mode, forward_only=True)
    xd, wd, bd = dev_act(x), wt.float().to(DEV), bias.float().to(DEV)
    x64 = xd[..., :cin].to(F64).view(-1, cin)
    w64 = wt.to(DEV).view(cout, cin).t().contiguous()
    y_ref, a_ref = x64 @ w64, x64.abs() @ w64.abs()
    del x64

    def stored(y):   # [B, H, W, Np] -> float64 [M, cout]; the padded channels must hold zeros
        assert y.shape[3] == cout or float(y[..., cout:].float().abs().max()) == 0.0, name
        return y[..., :cout].to(F64).view(-1, cout)

    with forced(conv=variant), torch.no_grad():
        y, st = F._Conv2dFn.apply(xd, wd, None, 1, 0, False, True)
        assert last_kernel() == code, (name, "forward ran kernel %d, expected %d" % (last_kernel(), code))
        y2, _ = F._Conv2dFn.apply(xd, wd, bd, 1, 0, True, False)
        assert last_kernel() == code, (name, last_kernel(), code)
    if mode == "exact":
        assert big_share(y_ref) > 0.25, (name, big_share(y_ref))
    yy = stored(y)
    check_bf16(name + " fwd", yy, y_ref, a_ref, cin, mode)
    depth = R.stream_stats_depth(R.stream_geometry(cin, cout, b * h * w, False))
    check_stats(name, st, yy.t().reshape(1, cout, 1, -1), mode, depth=depth)
    b64 = bias.to(DEV)
    check_bf16(name + " fwd bias relu", stored(y2), y_ref + b64, a_ref + b64.abs(), cin, mode, relu=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", R.STREAM_PROD_GEOMS)
def test_conv_stream_production_grid(F, geom, mode):
    """conv_stream.hip forced onto its production grid (256 work-groups per resident group: 64 / 21 / 10 walkers per XCD and
    channel block, tiles taken nwalk apart) at the smallest pixel count that has it in steady state with uneven shares
    (float64_refs.stream_steady_pixels): some walker owns ring + 2 tiles, another ring + 1, the XCDs' ranges differ by a tile, the
    last tile holds one pixel.  One cout with three channel blocks (520), one with a single 64-channel block (40)."""
    cin, cout, m = geom[3], geom[4], geom[2]
    geo = R.stream_geometry(cin, cout, m, False)
    counts = R.walker_tiles(geo)
    assert counts[-1] == geo["ring"] + 2 and geo["ring"] + 1 in counts and len(set(geo["xcnt"])) == 2 and m % geo["TM"] == 1
    stream_forward_on_device(F, geom, mode, STREAM, stream_code(cin, cout), "stream production grid")


# ---- 6. accumulating epilogue ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom,code", list(zip(R.ACC_GEOMS, [None, K.K_TILE + 4, None])))
def test_accumulating_epilogue(F, geom, code, mode):
    """conv2d_add_: out = relu(bf16(conv1x1(x) + bias) + out) in place - conv_tile_kernel<4, 1, 3, ACC> (K_TILE + 4) and, where the map
    is too small for it, conv_igemm_kernel's accumulate path (asserted: an igemm code); both roundings in the reference."""
    b, h, w, cin, cout = geom[:5]
    x, wt, bias, _, old = R.conv_operands(geom, mode)
    out = dev_act(old)
    with torch.no_grad(), forced():
        got = F.conv2d_add_(dev_act(x), wt.float().to(DEV), bias.float().to(DEV), out, 1, 0, relu=True)
        assert code_ok(code if code is not None else igemm_family), last_kernel()
    assert got.data_ptr() == out.data_ptr()
    ref, a = R.conv_fwd_ref(x, wt, 1, 0, 0, bias)
    if mode == "exact":
        assert big_share(ref) > 0.25
    check_bf16("accumulate %s" % (geom,), host_act(got, cout)[0], ref, a, cin, mode, relu=True, old=old)


# ---- 7. long K ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom,linear", list(zip(R.LONGK_GEOMS, [False, True, True])))
def test_long_reductions(F, geom, linear, mode):
    """K = 2048 (res5 conv1 on 2 x 5 x 7) and the ViT linears through F.linear (768 -> 2304, 3072 -> 768 on 65 rows): E is no longer
    negligible beside the bf16 step here."""
    run_layer(F, geom, mode, stats=not linear, linear=linear, name="long K")


# ---- 8. fully connected 7x7 ----
@pytest.mark.parametrize("mode", MODES)
def test_fully_connected_7x7(F, mode):
    """The box head's fc1 as a 7x7 conv over 37 ROIs of 7 x 7 x 256 -> 1024: forward, the plain-GEMM data-gradient branch of
    _Conv2dFn.backward and the wide-tile weight-gradient rule (Hout == Wout == 1: conv_wgrad256_kernel, K_WGRAD256)."""
    run_layer(F, R.FC_GEOM, mode, wgrad_code=K.K_WGRAD256, bias_leg="fwd", name="fc1")


# ---- 9. weight-gradient kernels ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant,code", WGRAD_TAP_VARIANTS)
def test_wgrad_per_tap_variants(F, variant, code, mode):
    """conv_wgrad_kernel<GLDS, TR> (all four), the XCD-grouped launch, conv_wgrad256_kernel, atomics and partial tiles +
    wgrad_reduce_kernel, on 3x3 128 -> 136 and 1x1 256 -> 264 over 2 x 21 x 27."""
    for geom in R.WGRAD_TAP_GEOMS:
        run_layer(F, geom, mode, wgrad=variant, wgrad_code=code, stats=False, bias_leg=None, name="wgrad %d" % variant)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", WGRAD_HALO_VARIANTS)
@pytest.mark.parametrize("geom", R.WGRAD_HALO_GEOMS)
def test_wgrad_halo_variants(F, geom, variant, mode):
    """conv_wgrad_halo_kernel forced: atomics, partial blocks + reduction pass, two rounds.  Its launcher serves H >= 2 and
    W >= 11 (wgrad_halo.hip:launch_wgrad_halo); the 5 x 7, 1 x 1 and 1 x 9 maps go on to the per-tap kernel (K_WGRAD + 3)."""
    code = K.K_WGRAD_HALO if geom[1] >= 2 and geom[2] >= 11 else K.K_WGRAD + 3
    run_layer(F, geom, mode, wgrad=variant, wgrad_code=code, stats=False, bias_leg=None, name="wgrad halo %d" % variant)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tiny", [0, 1])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
def test_wgrad_stream_configurations(F, cfg, tiny, mode):
    """wgrad_stream_kernel, every block configuration, 8 pixel ranges and the full grid: one pixel, 323, 1073 and 1386 pixels (no
    multiple of the 32-pixel step or of a range), channel tails on both operands."""
    for geom in R.WGRAD_STREAM_GEOMS:
        variant = ws_variant(cfg, tiny)
        b, h, w, cin, cout = geom[:5]
        r = plain_refs(geom, mode)
        with forced(wgrad=variant):
            got = abi_wgrad(F, r["x"], r["gy"], geom)
            assert last_kernel() // 100 == K.K_WGRAD_STREAM // 100 and (cfg == 0 or last_kernel() == K.K_WGRAD_STREAM + cfg), (cfg, last_kernel())
        check_f32("wgrad stream %d %d %s" % (cfg, tiny, geom), got, r["dw"][0], r["dw"][1], b * h * w, mode)


def guarded_destination(n_valid, c_valid, taps, g, mode):
    """A weight-gradient destination in the reference's [N][Cin][KH][KW] order inside a larger buffer: a band in front, a gap
    after every filter's row and a band behind, everything holding non-zero values (the launch ADDS).  Returns the buffer, the
    view's offset, (stride_n, stride_tap, stride_c) and the boolean map of the elements the launch may write."""
    row = c_valid * taps + 5
    total = 64 + n_valid * row + 64
    base = (R.ints((total,), 8, g) * 2 + 1) if mode == "exact" else (torch.randn((total,), generator=g, dtype=F64) * 1e-3).float().to(F64)
    written = torch.zeros(total, dtype=torch.bool)
    for n in range(n_valid):
        written[64 + n * row: 64 + n * row + c_valid * taps] = True
    return base, 64, (row, 1, taps), written


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom,variant,code", [
    (R.WGRAD_TAP_GEOMS[0], K.WG_HALO_FORBID, K.K_WGRAD + 3), (R.WGRAD_TAP_GEOMS[0], K.WG_HALO_FORCE, K.K_WGRAD_HALO),
    (R.WGRAD_TAP_GEOMS[0], K.WG_HALO_FORCE | K.WG_PARTIALS_FORCE, K.K_WGRAD_HALO),
    (R.WGRAD_TAP_GEOMS[1], K.WG_STREAM_FORBID, K.K_WGRAD + 3), (R.WGRAD_TAP_GEOMS[1], WS_FORCE, K.K_WGRAD_STREAM + 3),
    (R.WGRAD_TAP_GEOMS[1], K.WG_WIDE_FORCE, K.K_WGRAD256)])
def test_wgrad_into_strided_destination(F, geom, variant, code, mode):
    """u2_conv_wgrad_into: += into a destination that holds non-zero values, laid out with the reference's [N][Cin][KH][KW]
    strides, n_valid < N and c_valid < C; the bands around and between the written rows come back untouched (bit for bit in
    both modes).  Per-tap, halo (atomics / partial blocks), streaming and 256-wide kernels."""
    from u2seg_amd import _hip

    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    taps = kh * kw
    n_valid, c_valid = cout - 3, cin - 5
    r = plain_refs(geom, mode)
    g = torch.Generator().manual_seed(variant % 1013)
    base, off, (sn, st_, sc), written = guarded_destination(n_valid, c_valid, taps, g, mode)
    buf = base.float().to(DEV)
    xd, dzd = dev_act(r["x"]), dev_act(r["gy"])
    _hip.call("u2_conv_wgrad_into", xd, dzd, buf[off:], b, h, w, xd.shape[3], xd.shape[3], h, w, dzd.shape[3], dzd.shape[3], kh, kw,
              ph, pw, stride, n_valid, c_valid, sn, st_, sc, variant)
    assert last_kernel() == code, (last_kernel(), code)
    got = buf.to(F64).cpu()
    assert torch.equal(got[~written], base[~written]), "guard bands were written"
    rows = torch.arange(n_valid).view(-1, 1) * sn + off + torch.arange(c_valid * taps).view(1, -1)
    ref = base[rows].view(n_valid, c_valid, kh, kw) + r["dw"][0][:n_valid, :c_valid]
    a = base[rows].abs().view(n_valid, c_valid, kh, kw) + r["dw"][1][:n_valid, :c_valid]
    check_f32("wgrad_into %d %s" % (variant, geom), got[rows].view(n_valid, c_valid, kh, kw), ref, a, b * h * w + 1, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tiny", [0, 1])
@pytest.mark.parametrize("geom", R.FUSED_GEOMS)
def test_fused_1x1_backward(F, geom, tiny, mode):
    """u2_conv1x1_bwd_fused (U2_WD_FORCE lifts the size rule; U2_WD_TINY: 8 pixel ranges): dx (all physical channels written, the
    padded ones zero) and dw += into a non-zero [N][Cin] destination, blocks of N <= 256 by C <= 64 (2751) and N <= 512 by
    C <= 128 (2752), one pixel and 2 x 37 x 41 pixels, channel tails.  The launcher must answer 0 (launched)."""
    from u2seg_amd import _hip

    b, h, w, cin, cout = geom[:5]
    m = b * h * w
    r = plain_refs(geom, mode)
    g = torch.Generator().manual_seed(cin + cout + tiny)
    base = (R.ints((cout * cin + 64,), 8, g) * 2 + 1) if mode == "exact" else \
        (torch.randn((cout * cin + 64,), generator=g, dtype=F64) * 1e-3).float().to(F64)
    buf = base.float().to(DEV)
    xd, dzd = dev_act(r["x"]), dev_act(r["gy"])
    cp, npad = xd.shape[3], dzd.shape[3]
    wdl = F.weight_dgrad_layout(r["w"].float().to(DEV), cp, npad)
    dx = torch.full((b, h, w, cp), 7.0, dtype=BF16, device=DEV)
    rc = _hip.call_status("u2_conv1x1_bwd_fused", xd, dzd, wdl, dx, buf, m, cp, cp, npad, npad, npad, cp, cout, cin, cin, 1,
                          K.WD_FORCE | (K.WD_TINY if tiny else 0))
    assert rc == 0 and last_kernel() == K.K_WDGRAD + (1 if cout <= 256 else 2), (rc, last_kernel())
    got_dx, pad = host_act(dx, cin)
    assert pad == 0.0
    check_bf16("fused dx %s" % (geom,), got_dx, r["dx"][0], r["dx"][1], cout, mode)
    got = buf.to(F64).cpu()
    assert torch.equal(got[cout * cin:], base[cout * cin:])
    check_f32("fused dw %s" % (geom,), got[:cout * cin].view(cout, cin, 1, 1), base[:cout * cin].view(cout, cin, 1, 1) + r["dw"][0],
              base[:cout * cin].abs().view(cout, cin, 1, 1) + r["dw"][1], m + 1, mode)


@pytest.mark.parametrize("tiny", [0, 1])
@pytest.mark.parametrize("geom", R.FUSED_GEOMS[:3])
def test_fused_1x1_backward_with_norm_apply_exact(F, geom, tiny):
    """u2_conv1x1_bwd_fused_bn (2761): dy = k1 dz + k2 y + k3 with k1, k2 in {+-1, +-2}, integer k3 and integer dz, y of amplitude
    16 - |dy| <= 80, an integer and a bf16 value, so the apply step's rounding is exact and dx, dw are those of the integer dy."""
    from u2seg_amd import _hip

    b, h, w, cin, cout = geom[:5]
    m = b * h * w
    g = torch.Generator().manual_seed(cin * 3 + cout + tiny)
    x, wt = R.ints((b, cin, h, w), 4, g), R.ints((cout, cin, 1, 1), 4, g)
    dz, yn = R.ints((b, cout, h, w), 16, g), R.ints((b, cout, h, w), 16, g)
    k1 = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=F64)[torch.randint(0, 4, (cout,), generator=g)]
    k2 = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=F64)[torch.randint(0, 4, (cout,), generator=g)]
    k3 = R.ints((cout,), 16, g)
    dy = k1.view(1, -1, 1, 1) * dz + k2.view(1, -1, 1, 1) * yn + k3.view(1, -1, 1, 1)
    assert float(dy.abs().max()) <= 256 and torch.equal(R.rne_bf16(dy), dy)
    ref_dx, ref_dw = R.conv_dgrad_ref(dy, wt, (h, w), 1, 0, 0), R.conv_wgrad_ref(x, dy, 1, 1, 1, 0, 0)
    base = R.ints((cout * cin + 64,), 8, g) * 2 + 1
    buf = base.float().to(DEV)
    xd, dzd, ynd = dev_act(x), dev_act(dz), dev_act(yn)
    cp, npad = xd.shape[3], dzd.shape[3]
    ks = torch.zeros((3, npad), dtype=torch.float32, device=DEV)
    for i, k in enumerate((k1, k2, k3)):
        ks[i, :cout] = k.float().to(DEV)
    wdl = F.weight_dgrad_layout(wt.float().to(DEV), cp, npad)
    dx = torch.full((b, h, w, cp), 7.0, dtype=BF16, device=DEV)
    rc = _hip.call_status("u2_conv1x1_bwd_fused_bn", xd, dzd, ynd, ks[0], ks[1], ks[2], wdl, dx, buf, m, cp, cp, npad, npad, npad, cp,
                          cout, cin, cin, 1, K.WD_FORCE | (K.WD_TINY if tiny else 0))
    assert rc == 0 and last_kernel() == K.K_WDGRAD_BN + 1, (rc, last_kernel())
    got_dx, pad = host_act(dx, cin)
    assert pad == 0.0
    check_bf16("fused bn dx %s" % (geom,), got_dx, ref_dx[0], ref_dx[1], cout, "exact")
    got = buf.to(F64).cpu()
    assert torch.equal(got[cout * cin:], base[cout * cin:])
    check_f32("fused bn dw %s" % (geom,), got[:cout * cin].view(cout, cin, 1, 1), base[:cout * cin].view(cout, cin, 1, 1) + ref_dw[0],
              base[:cout * cin].abs().view(cout, cin, 1, 1) + ref_dw[1], m + 1, "exact")


# ---- 10. bias gradient paths ----
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,cp,n", [(1000, 32, 15), (16 * 37 * 29, 256, 256), (4111, 64, 40), (7, 32, 32), (1, 32, 8)])
def test_bias_gradient_kernels(F, rows, cp, n, mode):
    """u2_colsum_add and u2_relu_bwd_colsum into a non-zero destination of n < npad channels (channels >= n untouched), and
    u2_colstats: integer sums exact, realistic gradients within E with L = rows + 1 (the destination's old value is a term)."""
    from u2seg_amd import _hip

    g = torch.Generator().manual_seed(rows + cp + n)
    if mode == "exact":
        dout, base = R.ints((rows, cp), 8, g), R.ints((cp,), 100, g)
    else:
        dout = R.bf16_round(torch.randn((rows, cp), generator=g, dtype=F64) * 2.0 ** -10)
        base = (torch.randn((cp,), generator=g, dtype=F64) * 2.0 ** -6).float().to(F64)
    out = R.bf16_round(torch.randn((rows, cp), generator=g, dtype=F64))
    dd, od = dout.to(BF16).to(DEV), out.to(BF16).to(DEV)
    dst = base.float().to(DEV)
    _hip.call("u2_colsum_add", dd, dst, rows, cp, cp, n)
    got = dst.to(F64).cpu()
    assert torch.equal(got[n:], base[n:])
    check_f32("colsum_add", got[:n], (base + dout.sum(0))[:n], (base.abs() + dout.abs().sum(0))[:n], rows + 1, mode)
    dz = torch.empty_like(dd)
    dst = base.float().to(DEV)
    _hip.call("u2_relu_bwd_colsum", dd, od, dz, dst, torch.zeros(cp, device=DEV), rows, cp, cp, n)
    want_dz = dout * (out > 0)
    assert torch.equal(dz.to(F64).cpu(), want_dz)
    got = dst.to(F64).cpu()
    assert torch.equal(got[n:], base[n:])
    check_f32("relu_bwd_colsum", got[:n], (base + want_dz.sum(0))[:n], (base.abs() + want_dz.abs().sum(0))[:n], rows + 1, mode)
    sums = torch.zeros((1, 2, cp), dtype=torch.float32, device=DEV)
    _hip.call("u2_colstats", dd, sums, 1, rows, cp, cp)
    check_f32("colstats sum", sums[0, 0], dout.sum(0), dout.abs().sum(0), rows, mode)
    sq = (dout * dout).sum(0)
    check_f32("colstats squares", sums[0, 1], sq, sq, rows, mode)
