"""The grouped 3x3 kernels (conv_grouped.hip: u2_gconv3x3_fwd / _dgrad / _wgrad) through the C ABI, every element of every output
against float64 (tests/grouped_conv_refs.py), in the two modes of tests/test_gpu_conv_float64.py:

A. exact integers, bit for bit, with sum |term| < 2^24 asserted;
B. activation-like inputs inside float64_refs.bf16_interval / fp32_sum_bound with L = 9 cg forward and backward and
   L = B Hout Wout for dw and the statistics.  The filter the references multiply with is W' = bf16(fp32(w) * fp32(scale)), the
   contract of include/u2seg_hip.h (grouped_conv_refs.fold); in mode B the fp32 filter is not a bf16 number, so the kernels'
   rounding while staging is part of what is checked.

Legs per case: plain forward with statistics, data gradient, weight gradient into zeros; bias + ReLU forward; with `scale`: forward
(W'), data gradient and the scaled weight gradient accumulated onto a non-zero destination."""
import functools

import pytest
import torch

from tests import float64_refs as R
from tests import grouped_conv_refs as G
from tests.test_gpu_conv_float64 import check_bf16, check_f32, check_stats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
CANARY = 12345.0


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF16).to(DEV)


def nchw(t):
    return t.permute(0, 3, 1, 2).to(F64).cpu()


def f32(t):
    return t.float().contiguous().to(DEV)


@functools.lru_cache(maxsize=2)
def refs(case, stride, mode):
    """Operands and every float64 reference of one case, computed once and left unchanged."""
    c, groups, b, h, w = case
    x, wt, bias, gy, scale, old = G.grouped_operands(case, stride, mode)
    ws = G.fold(wt, scale)
    wp = G.fold(wt, torch.ones_like(scale))
    r = dict(x=x, w=wt, bias=bias, gy=gy, scale=scale, old=old)
    r["y"] = G.gconv_fwd_ref(x, wp, groups, stride)
    r["yb"] = G.gconv_fwd_ref(x, wp, groups, stride, bias)
    r["dx"] = G.gconv_dgrad_ref(gy, wp, groups, (h, w), stride)
    r["dw"] = G.gconv_wgrad_ref(x, gy, groups, stride)
    r["ys"] = G.gconv_fwd_ref(x, ws, groups, stride)
    r["dxs"] = G.gconv_dgrad_ref(gy, ws, groups, (h, w), stride)
    s4 = scale.view(-1, 1, 1, 1)
    r["dws"] = (s4 * r["dw"][0] + old, s4.abs() * r["dw"][1] + old.abs())
    return r


@pytest.mark.parametrize("mode", ["exact", "real"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: "C%d_G%d_%dx%dx%d" % c)
def test_grouped_kernels(H, case, stride, mode):
    c, groups, b, h, w = case
    cg = c // groups
    ho, wo = G.out_hw(h, w, stride)
    m = b * ho * wo
    r = refs(case, stride, mode)
    name = "gconv %s s%d %s" % (case, stride, mode)
    if mode == "exact":
        assert float(r["w"].abs().max()) <= 256 and float((r["w"] * r["scale"].view(-1, 1, 1, 1)).abs().max()) <= 256
    xd, gyd, wd = nhwc(r["x"]), nhwc(r["gy"]), f32(r["w"])
    dims = (b, h, w, c, groups, stride)

    # plain: forward + statistics, data gradient, weight gradient into zeros
    out = torch.full((b, ho, wo, c), CANARY, dtype=BF16, device=DEV)
    stats = torch.zeros((2, c), dtype=torch.float32, device=DEV)
    H.call("u2_gconv3x3_fwd", xd, wd, None, None, out, stats, *dims, 0)
    yy = nchw(out)
    check_bf16(name + " fwd", yy, r["y"][0], r["y"][1], 9 * cg, mode)
    check_stats(name, stats, yy, mode)
    dx = torch.full((b, h, w, c), CANARY, dtype=BF16, device=DEV)
    H.call("u2_gconv3x3_dgrad", gyd, wd, None, dx, *dims)
    check_bf16(name + " dgrad", nchw(dx), r["dx"][0], r["dx"][1], 9 * cg, mode)
    dw = torch.zeros((c, cg, 3, 3), dtype=torch.float32, device=DEV)
    H.call("u2_gconv3x3_wgrad", xd, gyd, None, dw, *dims)
    check_f32(name + " wgrad", dw, r["dw"][0], r["dw"][1], m, mode)

    # bias + ReLU
    out = torch.full((b, ho, wo, c), CANARY, dtype=BF16, device=DEV)
    H.call("u2_gconv3x3_fwd", xd, wd, None, f32(r["bias"]), out, None, *dims, 1)
    check_bf16(name + " fwd bias relu", nchw(out), r["yb"][0], r["yb"][1], 9 * cg, mode, relu=True)

    # scale: W' in the forward pass and the data gradient, the scaled weight gradient added onto a non-zero destination
    sd = f32(r["scale"])
    out = torch.full((b, ho, wo, c), CANARY, dtype=BF16, device=DEV)
    H.call("u2_gconv3x3_fwd", xd, wd, sd, None, out, None, *dims, 0)
    check_bf16(name + " fwd scale", nchw(out), r["ys"][0], r["ys"][1], 9 * cg, mode)
    dx = torch.full((b, h, w, c), CANARY, dtype=BF16, device=DEV)
    H.call("u2_gconv3x3_dgrad", gyd, wd, sd, dx, *dims)
    check_bf16(name + " dgrad scale", nchw(dx), r["dxs"][0], r["dxs"][1], 9 * cg, mode)
    dw = f32(r["old"])
    H.call("u2_gconv3x3_wgrad", xd, gyd, sd, dw, *dims)
    check_f32(name + " wgrad scale onto old", dw, r["dws"][0], r["dws"][1], m + 1, mode)
    torch.cuda.synchronize()


def test_low_amplitude_statistics(H):
    """Integers in {-1, 0, 1}: the sums of squares stay below 2^24 too, so both statistics rows are exact."""
    c, groups, b, h, w = 64, 8, 2, 33, 47
    g = torch.Generator().manual_seed(5)
    x, wt = R.ints((b, c, h, w), 1, g), R.ints((c, c // groups, 3, 3), 1, g)
    out = torch.empty((b, h, w, c), dtype=BF16, device=DEV)
    stats = torch.zeros((2, c), dtype=torch.float32, device=DEV)
    H.call("u2_gconv3x3_fwd", nhwc(x), f32(wt), None, None, out, stats, b, h, w, c, groups, 1, 0)
    ref, a = G.gconv_fwd_ref(x, wt, groups, 1)
    yy = nchw(out)
    check_bf16("gconv low amplitude fwd", yy, ref, a, 9 * c // groups, "exact")
    check_stats("gconv low amplitude", stats, yy, "exact", need_exact_squares=True)


@pytest.mark.parametrize("c,groups", [(64, 32), (48, 4), (40, 5), (64, 1), (128, 1)], ids=str)
def test_shapes_not_served_write_nothing(H, c, groups):
    """cg = 2, C % 32 != 0 and a dense layer: a non-zero return code and untouched outputs, from all three entries."""
    b, h, w = 1, 5, 7
    cg = c // groups
    x = torch.ones((b, h, w, c), dtype=BF16, device=DEV)
    wt = torch.ones((c, cg, 3, 3), dtype=torch.float32, device=DEV)
    for stride in (1, 2):
        ho, wo = G.out_hw(h, w, stride)
        gy = torch.ones((b, ho, wo, c), dtype=BF16, device=DEV)
        out = torch.full((b, ho, wo, c), CANARY, dtype=BF16, device=DEV)
        stats = torch.full((2, c), CANARY, dtype=torch.float32, device=DEV)
        dx = torch.full((b, h, w, c), CANARY, dtype=BF16, device=DEV)
        dw = torch.full((c, cg, 3, 3), CANARY, dtype=torch.float32, device=DEV)
        lib = H.load()
        s = H.stream_ptr()
        p = lambda t: t.data_ptr()
        assert lib.u2_gconv3x3_fwd(p(x), p(wt), None, None, p(out), p(stats), b, h, w, c, groups, stride, 0, s) != 0
        assert lib.u2_gconv3x3_dgrad(p(gy), p(wt), None, p(dx), b, h, w, c, groups, stride, s) != 0
        assert lib.u2_gconv3x3_wgrad(p(x), p(gy), None, p(dw), b, h, w, c, groups, stride, s) != 0
        torch.cuda.synchronize()
        for t in (out, stats, dx, dw):
            assert bool((t.float() == float(torch.tensor(CANARY, dtype=t.dtype))).all())


def test_stride_3_is_not_served(H):
    x = torch.ones((1, 5, 7, 64), dtype=BF16, device=DEV)
    wt = torch.ones((64, 8, 3, 3), dtype=torch.float32, device=DEV)
    out = torch.full((1, 5, 7, 64), CANARY, dtype=BF16, device=DEV)
    assert H.load().u2_gconv3x3_fwd(x.data_ptr(), wt.data_ptr(), None, None, out.data_ptr(), None, 1, 5, 7, 64, 8, 3, 0, H.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((out.float() == float(torch.tensor(CANARY, dtype=BF16))).all())
