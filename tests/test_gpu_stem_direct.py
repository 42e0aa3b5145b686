"""The direct stem kernels (u2seg_amd/csrc/stem_conv.hip: u2_stem_conv_fwd, u2_stem_conv_wgrad) against the im2col path they
replace and against float64, per element, nothing sampled.

The operand of both paths is a[m][k] = bf16((x - mean) / std), zero in the padding and in the canvas beyond the image, K ordered
(kh, kw, c): the matrix u2_stem_im2col_batch writes (checked against float64 by tests/test_gpu_optim_resample_float64.py).  The
references below are float64 products of THAT matrix with the bf16 weights / gradient, so what is compared is the arithmetic
behind the operand: fp32 sums of exact bf16 x bf16 products, in an order that differs between the two paths.

Exact inputs: small-integer pixels (mean 0, std 1), weights and gradients, amplitudes chosen so that for every output element the
sum of |term| stays below 2^24 (asserted): every partial sum is an integer fp32 holds, whatever the order, so the stored bf16
output (one RNE of the exact sum), the column statistics of the stored values and dW are bit-equal to the im2col path and to the
integer reference built from tests/float64_refs.py (stem_canvas + stem_unfold_ref).

Random inputs, with u = 2^-24 and gamma_n = n u / (1 - n u):
  output: |got - ref| <= one bf16 step at |ref| + e, plus e = gamma_160 sum |a||w| (an fp32 sum of <= 160 exact products errs by
    at most gamma sum |term|; the result is rounded once to bf16);
  column sums: the kernels add the M stored bf16 values of a channel (exact in fp32) in some tree: |got - sum| <= gamma_M sum |v|;
  sums of squares: each term is one fma rounding more: gamma_(M + 1) sum v^2;
  dW: an fp32 sum of M exact products in some tree (registers, then one atomic per work-group): gamma_M sum |dy||a|.
"""
import ctypes
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = torch.float64
N, KP, K = 64, 160, 147

# name -> (image sizes (h, w), canvas (hpad, wpad))
CASES = {
    "tiny": ([(5, 9)], (32, 32)),                                   # an image smaller than one 8 x 32 patch
    "odd": ([(37, 53)], (64, 64)),
    "inside": ([(30, 45)], (64, 96)),                               # well inside its canvas: the zero (not normalised-zero) padding
    "batch3": ([(20, 33), (64, 50), (41, 96)], (64, 96)),           # the pointer table
    "ragged": ([(40, 72), (33, 61)], (40, 72)),                     # output 20 x 36: ragged against 8 x 32 both ways
    "many": ([(256, 1024), (250, 1001), (256, 1024), (131, 517)], (256, 1024)),   # 1024 patches on 512 work-groups
}
DTYPES = ["uint8", "float32"]


def gamma(n):
    return n * R.U24 / (1 - n * R.U24)


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()
    return functional


def _out_hw(hpad, wpad):
    return (hpad + 6 - 7) // 2 + 1, (wpad + 6 - 7) // 2 + 1


def _tables(images):
    b = len(images)
    return ((ctypes.c_void_p * b)(*[im.data_ptr() for im in images]), (ctypes.c_int * b)(*[im.shape[1] for im in images]),
            (ctypes.c_int * b)(*[im.shape[2] for im in images]))


def _inputs(case, dtype, mode):
    """images, mean, std, weight [64, 3, 7, 7] (bf16 values in fp32), dy [B, Ho, Wo, 64] bf16 - all on the device."""
    sizes, (hpad, wpad) = CASES[case]
    g = torch.Generator().manual_seed(sum(ord(c) for c in case + dtype + mode))
    ho, wo = _out_hw(hpad, wpad)
    m = len(sizes) * ho * wo
    if mode == "exact":
        # Amplitudes (pixels 0 .. ax as uint8, -ax .. ax as float32; weights -aw .. aw; gradient -ad .. ad): a channel's sum of
        # squared outputs is about (pixels that see the image) 147 E[x^2] E[w^2] and has to stay below 2^24 (asserted by the test,
        # with the other preconditions).  "tiny": ~50 output pixels see the 5 x 9 image, so the amplitudes can be large enough for
        # sums past 256, where bf16 no longer holds every integer; "many" (M = 262 144): sparse {-1, 0, 1}.  (uint8 pixels are
        # not centred: a channel's outputs then have the mean E[x] sum_k w, whose square counts M times as well.)
        ax, aw, ad = {"tiny": (15, 4, 2), "many": (1, 1, 1)}.get(case, (2, 2, 2))
        if dtype == "uint8":
            images = [torch.randint(0, ax + 1, (3, h, w), generator=g, dtype=torch.uint8) for h, w in sizes]
        else:
            images = [torch.randint(-ax, ax + 1, (3, h, w), generator=g).float() for h, w in sizes]
        mean, std = torch.zeros(3), torch.ones(3)
        w = torch.randint(-aw, aw + 1, (N, 3, 7, 7), generator=g).float()
        if case == "many":
            w = w * (torch.rand((N, 3, 7, 7), generator=g) < 0.1).float()
        dy = torch.randint(-ad, ad + 1, (len(sizes), ho, wo, N), generator=g).float()
    else:
        if dtype == "uint8":
            images = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in sizes]
        else:
            images = [torch.rand((3, h, w), generator=g) * 255 for h, w in sizes]
        mean, std = torch.tensor([123.675, 116.28, 103.53]), torch.tensor([58.395, 57.12, 57.375])
        w = (torch.randn((N, 3, 7, 7), generator=g) * 0.05).bfloat16().float()
        dy = torch.randn((len(sizes), ho, wo, N), generator=g) * 2.0 ** -6
    return ([im.to(DEV) for im in images], mean.to(DEV), std.to(DEV), w.to(DEV), dy.bfloat16().to(DEV).contiguous())


def _wk(w):
    wk = torch.zeros((w.shape[0], 1, KP), dtype=torch.bfloat16, device=DEV)
    wk[:, 0, :K] = w.permute(0, 2, 3, 1).reshape(w.shape[0], K)
    return wk


def _direct(images, mean, std, wk, dy, hpad, wpad):
    from u2seg_amd import _hip
    b = len(images)
    ho, wo = _out_hw(hpad, wpad)
    ptrs, hs, ws = _tables(images)
    is_u8 = int(images[0].dtype == torch.uint8)
    out = torch.full((b, ho, wo, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros((2, N), dtype=torch.float32, device=DEV)
    assert _hip.call_status("u2_stem_conv_fwd", ptrs, hs, ws, b, is_u8, mean, std, wk, out, stats, hpad, wpad, N, KP) == 0
    dw = torch.zeros((N, KP), dtype=torch.float32, device=DEV)
    assert _hip.call_status("u2_stem_conv_wgrad", ptrs, hs, ws, b, is_u8, mean, std, dy, dw, hpad, wpad, N, KP) == 0
    torch.cuda.synchronize()
    return out.view(-1, N), stats, dw


def _im2col(images, mean, std, wk, dy, hpad, wpad):
    from u2seg_amd import _hip
    b = len(images)
    ho, wo = _out_hw(hpad, wpad)
    m = b * ho * wo
    ptrs, hs, ws = _tables(images)
    is_u8 = int(images[0].dtype == torch.uint8)
    col = torch.empty((m, KP), dtype=torch.bfloat16, device=DEV)
    _hip.call("u2_stem_im2col_batch", ptrs, hs, ws, b, is_u8, mean, std, col, hpad, wpad, KP)
    out = torch.empty((m, N), dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros((2, N), dtype=torch.float32, device=DEV)
    _hip.call("u2_conv_igemm", col, wk, out, None, stats, 1, m, 1, KP, KP, m, 1, N, N, 1, 1, 0, 0, 1, 1, 0, 0, 0)
    dw = torch.zeros((N, 1, KP), dtype=torch.float32, device=DEV)
    _hip.call("u2_conv_wgrad", col, dy, dw, 1, m, 1, KP, KP, m, 1, N, N, 1, 1, 0, 0, 1, 0)
    torch.cuda.synchronize()
    return col, out, stats, dw.view(N, KP)


@functools.lru_cache(maxsize=None)
def _run(case, dtype, mode):
    """Both paths and the float64 references of one case, computed once; only the [M][64] / [64][160] results are kept."""
    _, (hpad, wpad) = CASES[case]
    images, mean, std, w, dy = _inputs(case, dtype, mode)
    wk = _wk(w)
    out, stats, dw = _direct(images, mean, std, wk, dy, hpad, wpad)
    col, out2, stats2, dw2 = _im2col(images, mean, std, wk, dy, hpad, wpad)
    a = col[:, :K].to(F64)
    assert not bool(col[:, K:].any())
    wm = wk[:, 0, :K].to(F64)
    d = dy.view(-1, N).to(F64)
    res = dict(m=a.shape[0], out=out, stats=stats, dw=dw, out2=out2, stats2=stats2, dw2=dw2,
               ref=a @ wm.t(), mag=a.abs() @ wm.abs().t(), dw_ref=d.t() @ a, dw_mag=d.abs().t() @ a.abs())
    if mode == "exact":
        canvas, _ = R.stem_canvas(images, mean, std, hpad, wpad)
        res["a_is_integer_ref"] = torch.equal(R.stem_unfold_ref(canvas).reshape(-1, K), a)
    return res


def _bf16_step(x):
    """Spacing of the bf16 numbers at magnitude x (float64): 2^(floor(log2 x) - 7); the smallest normal's below it."""
    return torch.exp2(torch.floor(torch.log2(x.clamp(min=2.0 ** -126))) - 7)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_exact_inputs_bit_equal(F, case, dtype):
    r = _run(case, dtype, "exact")
    assert r["a_is_integer_ref"], "the im2col matrix is not the integer canvas"
    ref = R.rne_bf16(r["ref"])
    got = r["out"].to(F64)
    # the preconditions of "exact": every sum of |term| an fp32 integer
    assert float(r["mag"].max()) < R.TWO24 and float(r["dw_mag"].max()) < R.TWO24
    assert float(ref.abs().sum(0).max()) < R.TWO24 and float((ref * ref).sum(0).max()) < R.TWO24
    print("%s %s: largest |output| %g" % (case, dtype, float(ref.abs().max())))
    assert float(ref.abs().max()) > 256 or case != "tiny", "no sum past the integers bf16 holds: no case checks the rounding"
    assert torch.equal(got, ref), "output differs from the integer reference"
    assert torch.equal(r["out"], r["out2"]), "output differs from the im2col path"
    st_ref = torch.stack([ref.sum(0), (ref * ref).sum(0)])
    assert torch.equal(r["stats"].to(F64), st_ref), "statistics differ from the integer reference"
    assert torch.equal(r["stats"], r["stats2"]), "statistics differ from the im2col path"
    assert torch.equal(r["dw"][:, :K].to(F64), r["dw_ref"]), "dW differs from the integer reference"
    assert torch.equal(r["dw"], r["dw2"]), "dW differs from the im2col path"
    assert not bool(r["dw"][:, K:].any()), "the padding columns of dW were written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_random_inputs_vs_float64(F, case, dtype):
    r = _run(case, dtype, "real")
    m = r["m"]
    got = r["out"].to(F64)
    assert bool(torch.isfinite(got).all())
    e = gamma(KP) * r["mag"]
    err, tol = (got - r["ref"]).abs(), _bf16_step(r["ref"].abs() + e) + e
    print("%s %s: output max err / tol %.3g" % (case, dtype, float((err / tol).max())))
    assert bool((err <= tol).all()), "output outside one bf16 step + gamma_160 sum |a||w|"
    s_ref, s_mag, q_ref = got.sum(0), got.abs().sum(0), (got * got).sum(0)
    es, eq = (r["stats"][0].to(F64) - s_ref).abs(), (r["stats"][1].to(F64) - q_ref).abs()
    print("%s %s: sums %.3g, squares %.3g of their bounds" % (case, dtype, float((es / (gamma(m) * s_mag)).max()),
                                                            float((eq / (gamma(m + 1) * q_ref)).max())))
    assert bool((es <= gamma(m) * s_mag).all()), "column sums outside gamma_M sum |v|"
    assert bool((eq <= gamma(m + 1) * q_ref).all()), "sums of squares outside gamma_(M+1) sum v^2"
    ew = (r["dw"][:, :K].to(F64) - r["dw_ref"]).abs()
    print("%s %s: dW %.3g of its bound" % (case, dtype, float((ew / (gamma(m) * r["dw_mag"]).clamp(min=1e-300)).max())))
    assert bool((ew <= gamma(m) * r["dw_mag"]).all()), "dW outside gamma_M sum |dy||a|"
    assert not bool(r["dw"][:, K:].any()), "the padding columns of dW were written"


class _Recorder:
    """Names of the C-ABI launches made through _hip.call / _hip.call_status while active (with their arguments)."""

    def __enter__(self):
        from u2seg_amd import _hip
        self.hip, self.saved, self.calls = _hip, (_hip.call, _hip.call_status), []

        def wrap(fn):
            def rec(name, *args):
                rc = fn(name, *args)
                self.calls.append((name, args, rc))
                return rc
            return rec

        _hip.call, _hip.call_status = wrap(_hip.call), wrap(_hip.call_status)
        return self

    def __exit__(self, *exc):
        self.hip.call, self.hip.call_status = self.saved

    def names(self):
        return [c[0] for c in self.calls if c[2] in (None, 0)]


def _autograd(F, case, dtype, direct):
    _, (hpad, wpad) = CASES[case]
    images, mean, std, w, dy = _inputs(case, dtype, "real")
    wd = w.clone().requires_grad_(True)
    saved = []
    old = F.STEM_DIRECT
    F.STEM_DIRECT = direct
    try:
        with _Recorder() as rec, torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t.numel()) or t, lambda t: t):
            y, stats = F.stem_conv(wd, images, mean, std, hpad, wpad)
            y.backward(dy)
    finally:
        F.STEM_DIRECT = old
    torch.cuda.synchronize()
    return y.detach().view(-1, N), stats.detach(), wd.grad.detach(), saved, rec.names()


@pytest.mark.parametrize("case,dtype", [("batch3", "uint8"), ("ragged", "float32")])
def test_autograd_matches_old_path_and_saves_no_matrix(F, case, dtype):
    r = _run(case, dtype, "real")
    m = r["m"]
    y, stats, gw, saved, names = _autograd(F, case, dtype, True)
    y0, stats0, gw0, saved0, names0 = _autograd(F, case, dtype, False)
    assert "u2_stem_conv_fwd" in names and "u2_stem_conv_wgrad" in names and "u2_stem_im2col_batch" not in names
    assert "u2_stem_im2col_batch" in names0 and "u2_conv_igemm" in names0 and "u2_conv_wgrad" in names0
    assert max(saved0) == m * KP, "the old path keeps the matrix (what this test compares against)"
    assert all(n < m * KP for n in saved), "something of the matrix's size is saved for backward"
    assert torch.equal(y, r["out"])   # the Function runs the launch checked above
    e = gamma(KP) * r["mag"]
    for got in (y.to(F64), y0.to(F64)):
        assert bool(((got - r["ref"]).abs() <= _bf16_step(r["ref"].abs() + e) + e).all())
    dw_ref = r["dw_ref"].view(N, 7, 7, 3).permute(0, 3, 1, 2)
    dw_mag = r["dw_mag"].view(N, 7, 7, 3).permute(0, 3, 1, 2)
    for got in (gw.to(F64), gw0.to(F64)):
        assert got.shape == (N, 3, 7, 7) and bool(((got - dw_ref).abs() <= gamma(m) * dw_mag).all())
    for st, out in ((stats, y), (stats0, y0)):
        v = out.to(F64)
        assert bool(((st[0].to(F64) - v.sum(0)).abs() <= gamma(m) * v.abs().sum(0)).all())
        assert bool(((st[1].to(F64) - (v * v).sum(0)).abs() <= gamma(m + 1) * (v * v).sum(0)).all())


def test_refusals_launch_nothing_and_fall_back(F):
    from u2seg_amd import _hip
    _, (hpad, wpad) = CASES["inside"]
    images, mean, std, w, dy = _inputs("inside", "uint8", "real")
    ptrs, hs, ws = _tables(images)
    ho, wo = _out_hw(hpad, wpad)
    for n, kp in ((32, KP), (N, 128)):
        wk = torch.zeros((n, kp), dtype=torch.bfloat16, device=DEV)
        out = torch.full((1, ho, wo, n), 7.0, dtype=torch.bfloat16, device=DEV)
        stats = torch.zeros((2, n), dtype=torch.float32, device=DEV)
        dw = torch.zeros((n, kp), dtype=torch.float32, device=DEV)
        gy = torch.ones((1, ho, wo, n), dtype=torch.bfloat16, device=DEV)
        assert _hip.call_status("u2_stem_conv_fwd", ptrs, hs, ws, 1, 1, mean, std, wk, out, stats, hpad, wpad, n, kp) == 1
        assert _hip.call_status("u2_stem_conv_wgrad", ptrs, hs, ws, 1, 1, mean, std, gy, dw, hpad, wpad, n, kp) == 1
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and not bool(stats.any()) and not bool(dw.any()), "a refused call wrote something"
    # a 32-channel stem through the Function: the direct launcher declines, the im2col GEMM serves it
    w32 = w[:32].clone().requires_grad_(True)
    with _Recorder() as rec:
        y, _ = F.stem_conv(w32, images, mean, std, hpad, wpad)
        y.backward(dy[..., :32].contiguous())
    torch.cuda.synchronize()
    assert ("u2_stem_conv_fwd", 1) in [(c[0], c[2]) for c in rec.calls]
    assert "u2_stem_im2col_batch" in rec.names() and "u2_conv_igemm" in rec.names() and "u2_conv_wgrad" in rec.names()
    r = _run("inside", "uint8", "real")
    e = gamma(KP) * r["mag"][:, :32]
    ref = r["ref"][:, :32]
    assert bool(((y.view(-1, 32).to(F64) - ref).abs() <= _bf16_step(ref.abs() + e) + e).all())
    gref = r["dw_ref"][:32].view(32, 7, 7, 3).permute(0, 3, 1, 2)
    gmag = r["dw_mag"][:32].view(32, 7, 7, 3).permute(0, 3, 1, 2)
    assert bool(((w32.grad.to(F64) - gref).abs() <= gamma(r["m"]) * gmag).all())


def test_switches_take_the_old_path(F):
    # the environment switch is read when the module is imported: a fresh interpreter (no GPU work in it)
    code = "from u2seg_amd.layers import functional as F; import sys; sys.exit(0 if F.STEM_DIRECT is False else 3)"
    env = dict(os.environ, U2_STEM_DIRECT="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    assert subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, timeout=120).returncode == 0
    assert F.STEM_DIRECT is True, "the direct path is the default"
    _, _, _, _, names = _autograd(F, "tiny", "uint8", False)
    assert "u2_stem_conv_fwd" not in names and "u2_stem_conv_wgrad" not in names and "u2_conv_igemm" in names
    # deterministic statistics: the im2col GEMM without epilogue statistics, recorded as a u2_conv_igemm call
    _, (hpad, wpad) = CASES["tiny"]
    images, mean, std, w, dy = _inputs("tiny", "uint8", "real")
    wd = w.clone().requires_grad_(True)
    F.set_deterministic_stats(True)
    try:
        with _Recorder() as rec:
            y, stats = F.stem_conv(wd, images, mean, std, hpad, wpad)
            y.backward(dy)
    finally:
        F.set_deterministic_stats(False)
    torch.cuda.synchronize()
    igemm = [c for c in rec.calls if c[0] == "u2_conv_igemm"]
    assert len(igemm) == 1 and igemm[0][1][2].data_ptr() == y.data_ptr() and igemm[0][1][4] is None and igemm[0][1][21] == 0
    assert "u2_stem_conv_fwd" not in [c[0] for c in rec.calls] and "u2_conv_wgrad" in rec.names()
    v = y.detach().view(-1, N).to(F64)   # (the fixed-order reduction of the stored output)
    assert torch.allclose(stats.to(F64), torch.stack([v.sum(0), (v * v).sum(0)]), rtol=1e-5, atol=1e-6)
