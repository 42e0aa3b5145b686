"""The head-loss kernels of u2seg_amd/csrc/losses.hip off their benchmark widths: softmax_ce_kernel<STATS>, semseg_ce_kernel,
scale_to_bf16_kernel, mask_predict_bce_kernel<STATS>, rpn_loss_level_kernel<FUSED3> and box_reg_l1_kernel at the smallest shapes
that reach every branch of the kernels and of their launchers (tests/loss_cases.py; tests/test_loss_cases_host.py holds the
tables to those branches), every element of every output against the float64 references of tests/float64_refs.py.

The kernels are called through the C ABI, so the test owns the buffers: output buffers are prefilled with NaN (an element the
kernel does not write fails every comparison), accumulators with a known non-zero prior (the kernels ADD to them).

Bounds.  None is measured.  They are the bounds of tests/test_gpu_heads_full_size.py - its module docstring derives the error of
the fast intrinsics, each of its tests the error of one kernel - with only the chain lengths re-derived from each case's launch
geometry.  Where that module wrote a chain length as a number of its one shape, the general form is stated here, once:

  an fp32 sum that a thread, wave or work-group forms over `local` terms and then sends through `atomics` atomic additions
  onto an accumulator holding `prior` errs by at most  u ((local + 2) A + atomics (A + |prior|)),  A = sum |term|     (acc_bound)

  softmax:  a lane sums 16 exponentials in the register form (two pieces of 8, pads add exact zeros), ceil(NC / 64) in the
            general form, then 6 levels of the wave sum; a wave adds the rows it walks, ceil(R / (4 grid)), and the launch sends
            4 grid = 4 min(512, ceil(R / 4)) wave atomics - R of them in the general form, one per row.
  semantic: a thread adds at most 2 cell rows x 16 pixels x 3 terms, the work-group sum adds 8 levels, one atomic per tile.
  mask:     a wave walks ceil(P / (4 slices)) positions, the four waves meet (3), then `slices` atomics per ROI: on the loss from
            every ROI, on dW / db from the ROIs of the class.  (The full-size test's 25 + 3 + 8 nk + 2 is P = 784.)
  RPN:      a thread takes ceil(B HW / (256 grid)) positions with A objectness and 4 A delta terms each, the work-group sum 8
            levels, one atomic per work-group.  (The full-size test counts 3 x 3 terms for both losses; 4 A per position is the
            chain of the localisation loss, used here.)
  box L1:   4 terms per row, ceil(R / (256 grid)) rows per thread, 8 levels, one atomic per work-group.

Each test prints the worst ratio to its bound on a line starting LOSS64, for information; no assertion uses it."""
import pytest
import torch
import torch.nn.functional as TF

from tests import float64_refs as R
from tests import loss_cases as C
from tests.test_gpu_heads_full_size import TINY, check_l1_grad, exp_rel, get_deltas64
from tests.test_gpu_norm_full_size import Check, check_vec, rnd, step  # noqa: F401  (rnd, step: what Check bounds in)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -24
PRIOR = 0.5                       # what the fp32 loss accumulators hold before a launch
CNT_PRIOR = [7, 11, 13, 17, 19]   # and the integer counters
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
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def status(H, name, *args):
    """The launcher's own return value (H.call raises on anything but 0)."""
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a   # noqa: E731
    return getattr(H.load(), name)(*[ptr(a) for a in args], H.stream_ptr())


def nans(shape, dtype=BF16):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)


def prior(n=1, value=PRIOR):
    return torch.full((n,), value, dtype=torch.float32, device=DEV)


def counters(n):
    return torch.tensor(CNT_PRIOR[:n], dtype=torch.int32, device=DEV)


def acc_bound(local, atomics, a, before=PRIOR):
    """Module docstring: a sum over `local` terms in registers / LDS, then `atomics` additions onto an accumulator."""
    return U * ((local + 2) * a + atomics * (a + abs(before)))


def worst(got, ref, bound):
    return float(((got.to(F64) - ref).abs() / (bound + 1e-300)).max()) if got.numel() else 0.0


def ident(case):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case)


# =================================================================================================
# softmax cross-entropy
def softmax_bounds(ref, case, gs):
    """test_softmax_ce_full_size's bounds with the width's term count: (dlogits bound before its doubling, loss-sum bound)."""
    _, _, walk, atomics, terms = C.softmax_geometry(*case)
    de = exp_rel(ref["z"] - ref["mx"])
    d_se = de.amax(1, keepdim=True) + (terms + 6) * U      # the lane's terms + the wave's 6 levels
    d_p = de + d_se + 2 * U
    e = gs * (d_p * ref["p"] + U * ref["grad"].abs() + TINY)
    ln_se = (ref["lse"] - ref["mx"]).abs()
    e_row = d_se + 4 * U * ln_se + TINY + 2 * U * (ref["mx"].abs() + ln_se + ref["zt"].abs())
    return e, float(e_row.sum()) + acc_bound(walk, atomics, float(ref["rows"].abs().sum()))


@pytest.mark.parametrize("case", C.SOFTMAX_CASES, ids=ident)
def test_softmax_ce(H, case):
    """u2_softmax_ce and u2_softmax_ce_stats.  dlogits: |got - bf16(ref)| within gscale (d_p p + u |p - onehot| + TINY), doubled,
    with d_p = exp_rel + d_se + 2 u and d_se = max exp_rel + (terms + 6) u; pad columns exactly 0; the two entry points bit for
    bit.  Loss: the row-wise bound d_se + 4 u ln(se) + TINY + 2 u (|max| + ln(se) + |z_t|), plus acc_bound(rows a wave walks,
    wave atomics of the launch).  Counters: equal to the counts torch forms from the bf16 values, first index among equal maxima."""
    r, nc, lp = case
    z, lab = (t.to(DEV) for t in C.softmax_case(*case))
    gs = C.softmax_gscale(case)
    ref = R.softmax_ce_ref(z, lab, nc)
    e, lbound = softmax_bounds(ref, case, gs)
    d0, l0 = nans((r, lp)), prior()
    H.call("u2_softmax_ce", z, lab, d0, l0, r, nc, lp, gs)
    d1, l1, cnt = nans((r, lp)), prior(), counters(5)
    H.call("u2_softmax_ce_stats", z, lab, d1, l1, r, nc, lp, gs, cnt, nc - 1)
    chk = Check("softmax %s: dlogits" % ident(case), 4e-3)
    chk.add(d0[:, :nc], ref["grad"] * gs, 2 * e)
    errs = [abs(float(l) - PRIOR - float(ref["loss"])) for l in (l0, l1)]
    print("LOSS64 softmax %s: dlogits %.3g, loss %.3g / %.3g" % (
        ident(case), chk.worst, errs[0] / (2 * lbound), errs[1] / (2 * lbound)))
    chk.done()
    assert bool((d0[:, nc:] == 0).all()), "a pad column of dlogits is not exactly 0"
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16)), "the two entry points differ"
    assert max(errs) <= 2 * lbound, (errs, lbound, float(ref["loss"]))
    zz = z[:, :nc].to(F64)
    pred, bg = R.first_argmax(zz), nc - 1
    fg = (lab >= 0) & (lab < bg)
    want = [r, int((pred == lab).sum()), int(fg.sum()), int((fg & (pred == lab)).sum()), int((fg & (pred == bg)).sum())]
    assert cnt.tolist() == [a + b for a, b in zip(CNT_PRIOR, want)], (cnt.tolist(), want)


@pytest.mark.parametrize("case", C.SOFTMAX_WRAPPER, ids=ident)
def test_softmax_ce_wrapper(F, H, case):
    """F.softmax_cross_entropy, one call per form: the loss is the sum / R (within the sum's bound / R and the division's
    rounding) and the backward is the kernel's dlogits at gscale = 1 / R times the upstream gradient (2: exact in bf16)."""
    r, nc, lp = case
    z, lab = (t.to(DEV) for t in C.softmax_case(*case))
    gs = C.f32(1.0 / r)
    ref = R.softmax_ce_ref(z, lab, nc)
    _, lbound = softmax_bounds(ref, case, gs)
    d, l0 = nans((r, lp)), prior(1, 0.0)
    H.call("u2_softmax_ce", z, lab, d, l0, r, nc, lp, gs)
    zd = z.detach().requires_grad_(True)
    loss = F.softmax_cross_entropy(zd, lab, nc)
    (2.0 * loss).backward()
    want = float(ref["loss"]) / r
    assert abs(float(loss.detach()) - want) <= 2 * lbound / r + U * abs(want), (float(loss.detach()), want)
    assert torch.equal(zd.grad.float(), d.float() * 2)


# =================================================================================================
# the semantic head's loss
def sem_bounds(ref, nc):
    """test_sem_seg_loss_full_size's bounds with cnt_err = 0: the per-pixel bound of (softmax - onehot) sent through the
    transposed interpolation -> the per-tap bound [B, h, w, nc] (before its doubling); the loss's error sum and magnitude sum."""
    z, up, t, valid = ref["z"], ref["up"], ref["target"], ref["valid"][:, None]
    with torch.no_grad():
        zabs = TF.interpolate(z.abs(), scale_factor=4, mode="bilinear", align_corners=False)
        mx = up.amax(1, keepdim=True)
        lse = torch.logsumexp(up, 1, keepdim=True)
        p = torch.exp(up - lse)
        oh = TF.one_hot(t.clamp_max(nc - 1), nc).permute(0, 3, 1, 2).to(F64)
        de = exp_rel(up - mx)
        dz = 4 * U * zabs.amax(1, keepdim=True)          # the kernel's interpolated logits (fp32, ATen's association)
        d_p = de + de.amax(1, keepdim=True) + 12 * U + 2 * dz
        epix = torch.where(valid, d_p * p + 15 * U * (p - oh).abs() + TINY, torch.zeros_like(p))
        zt = up.gather(1, t.clamp_max(nc - 1)[:, None])
        ln = lse - mx
        zero = torch.zeros_like(lse)
        asum = float(torch.where(valid, mx.abs() + ln.abs() + zt.abs(), zero).sum())
        esum = float(torch.where(valid, 2 * dz + de.amax(1, keepdim=True) + 12 * U + 14 * U * ln.abs() + TINY, zero).sum())
    (eg,) = torch.autograd.grad(up, z, epix, retain_graph=True)
    return eg.permute(0, 2, 3, 1), esum, asum


@pytest.mark.parametrize("case", C.SEM_CASES, ids=ident)
def test_semseg_upsample_ce(H, case):
    """u2_semseg_upsample_ce.  valid_cnt: exact.  grad_acc (fp32, unscaled): within the transposed interpolation of the
    per-pixel bounds, doubled - a bound per tap that does not depend on the map size; channels NC .. LP - 1 exactly 0; every
    element written.  Loss sum: the per-pixel error sum plus acc_bound(3 x 32 + 8 terms, one atomic per tile)."""
    b, h, w, nc, lp, ignore, _ = case
    z, t = (v.to(DEV) for v in C.sem_case(*case))
    ref = R.semseg_ce_ref(z, t, nc, ignore)
    e, esum, asum = sem_bounds(ref, nc)
    acc, ls, cnt = nans((b, h, w, lp), torch.float32), prior(), prior(1, 3.0)
    H.call("u2_semseg_upsample_ce", z, t, acc, ls, cnt, b, h, w, lp, nc, ignore)
    ny, nx = C.sem_tiles(h, w)
    lbound = esum + acc_bound(3 * 32 + 8, b * ny * nx, asum)
    lerr = abs(float(ls) - PRIOR - float(ref["loss"]))
    print("LOSS64 semseg %s: grad_acc %.3g, loss %.3g" % (
        ident(case), worst(acc[..., :nc], ref["grad"], 2 * e), lerr / (2 * lbound)))
    assert float(cnt) == 3.0 + ref["count"], (float(cnt), ref["count"])
    check_vec("semseg %s: grad_acc" % ident(case), acc[..., :nc], ref["grad"], 2 * e)
    assert bool((acc[..., nc:] == 0).all()), "a channel past NC is not exactly 0"
    assert lerr <= 2 * lbound, (float(ls), float(ref["loss"]), lbound)


@pytest.mark.parametrize("case", [(3, 8, 16, 28, 32), (1, 1, 1, 28, 32), (1, 15, 31, 17, 64)], ids=ident)
def test_semseg_without_a_valid_pixel(H, case):
    b, h, w, nc, lp = case
    z, t = C.sem_case(b, h, w, nc, lp)
    t[:] = 255
    acc, ls, cnt = nans((b, h, w, lp), torch.float32), prior(1, 0.0), prior(1, 0.0)
    H.call("u2_semseg_upsample_ce", z.to(DEV), t.to(DEV), acc, ls, cnt, b, h, w, lp, nc, 255)
    assert float(cnt) == 0.0 and float(ls) == 0.0 and bool((acc == 0).all())


@pytest.mark.parametrize("n", C.SCALE_N)
def test_scale_to_bf16(H, n):
    """out = bf16(acc * (mult * num / den)) with num or den absent = 1: the stored value lies in bf16_interval of the float64
    product widened by the three fp32 roundings (mult * num, / den, * acc): (1 + u)^3 - 1 < 3.001 u.  Nothing past n is written."""
    g = torch.Generator().manual_seed(n)
    acc = torch.randn(n, generator=g).to(DEV)
    num, den = prior(1, C.SCALE_NUM), prior(1, C.SCALE_DEN)
    for has_num, has_den, mult in C.SCALE_ARGS:
        out = nans((n + 64,))
        H.call("u2_scale_to_bf16", acc, num if has_num else None, den if has_den else None, mult, out, n)
        ref = acc.to(F64) * (mult * (float(num) if has_num else 1.0) / (float(den) if has_den else 1.0))
        lo, hi = R.bf16_interval(ref, 3.001 * U * ref.abs())
        chk = Check("scale_to_bf16 n = %d" % n, None)
        chk.add_interval(out[:n], lo, hi, ref)
        chk.done()
        assert bool(out[n:].isnan().all())
    print("LOSS64 scale_to_bf16 %d: inside the interval" % n)


@pytest.mark.parametrize("case", C.SEM_WRAPPER, ids=ident)
def test_sem_seg_loss_wrapper(F, case):
    """F.sem_seg_loss forward and backward, one call per map: the mean and u2_scale_to_bf16's division by the count."""
    b, h, w, nc, lp, ignore, _ = case
    z, t = (v.to(DEV) for v in C.sem_case(*case))
    ref = R.semseg_ce_ref(z, t, nc, ignore)
    e, esum, asum = sem_bounds(ref, nc)
    n = ref["count"]
    zd = z.detach().requires_grad_(True)
    loss = F.sem_seg_loss(zd, t, nc, ignore)
    loss.backward()
    ny, nx = C.sem_tiles(h, w)
    want = float(ref["loss"]) / n
    lbound = (esum + acc_bound(3 * 32 + 8, b * ny * nx, asum, 0.0)) / n + 2 * U * abs(want)
    assert abs(float(loss.detach()) - want) <= 2 * lbound, (float(loss.detach()), want, lbound)
    g = ref["grad"] / n
    chk = Check("sem_seg_loss %s: dlogits" % ident(case), 4e-3)
    chk.add(zd.grad[..., :nc], g, 2 * (e / n + 3 * U * g.abs()))
    chk.done()
    assert bool((zd.grad[..., nc:] == 0).all())


# =================================================================================================
# the mask predictor
def run_mask(H, xin, w, bias, cls, tgt, n, p, gs, side):
    k = w.shape[0]
    out = dict(dx=nans(xin.shape), dW=prior(k * C.MASK_C, 0.25).view(k, -1), db=prior(k, -0.125), loss=prior(), z=nans((n, p)))
    H.call("u2_mask_predict_bce", xin, w, bias, cls, tgt, out["dx"], out["dW"], out["db"], out["loss"], out["z"], n, p, C.MASK_C,
           gs, side, None)
    if side:
        out["dx"] = C.from_phases(out["dx"], side)
    return out


def check_mask(name, out, x, w, bias, cls, tgt, gs, loss_only=None):
    """test_mask_predict_bce_full_size's checks: the logit in the interval of the fp32 dot product's bound 2 (12 u sum |x w| +
    u |v|); loss, dx, dW, db at the kernel's own bf16 logit with that test's bounds and this case's chains."""
    n, p, _ = x.shape
    slices = C.mask_slices(p)
    npos = -(-p // (4 * slices))
    first = R.mask_bce_ref(x, w, bias, cls, tgt)
    v = first["logit"]
    ez = 2 * (12 * U * first["logit_abs"] + U * v.abs())
    chk_z = Check(name + ": logit", None)
    chk_z.add_interval(out["z"], rnd(v - ez), rnd(v + ez), v)
    chk_z.done()
    z = out["z"].to(F64)
    ref = R.mask_bce_ref(x, w, bias, cls, tgt, z)
    t = tgt.to(F64)
    sg = torch.sigmoid(z)
    g64 = ref["g"] * gs
    # sg = 1 / (1 + __expf(-z)): sigma (1 - sigma) exp_rel(|z|) + 2 u sigma; (sg - t): u; * gscale: 2 u
    e_g = (sg * (1 - sg) * exp_rel(z) + 2 * U * sg) * gs + 3 * U * g64.abs() + 2.0 ** -140
    wq = ref["wq"][:, None, :]
    chk_x = Check(name + ": dx", 5e-3)
    chk_x.add(out["dx"], ref["dx"] * gs, 2 * (e_g[:, :, None] * wq.abs() + U * (ref["dx"] * gs).abs()))
    chk_x.done()
    k = w.shape[0]
    xa = x.to(F64).abs()
    put = lambda val: torch.zeros((k,) + val.shape[1:], dtype=F64, device=DEV).index_add_(0, cls, val)   # noqa: E731
    nk = torch.bincount(cls, minlength=k).to(F64)
    # a class without a ROI keeps its prior exactly: its bound is 0
    dw_b = 2 * (acc_bound(npos + 3, slices * nk[:, None], ref["dW_abs"] * gs, 0.25) * (nk[:, None] > 0)
                + put(torch.einsum("np,npc->nc", e_g, xa)))
    db_b = 2 * (acc_bound(npos + 3, slices * nk, ref["db_abs"] * gs, 0.125) * (nk > 0) + put(e_g.sum(1)))
    check_vec(name + ": dW", out["dW"], 0.25 + ref["dW"] * gs, dw_b)
    check_vec(name + ": db", out["db"], -0.125 + ref["db"] * gs, db_b)
    # loss: max(z, 0) - z t + log1pf(__expf(-|z|)) per position
    y = torch.exp(-z.abs())
    lp = torch.log1p(y)
    li = ref["terms"]
    e_l = exp_rel(z) * y / (1 + y) + 4 * U * lp + TINY + 2 * U * (li.abs() + lp)
    lbound = float(e_l.sum()) + acc_bound(npos + 3, n * slices, float(li.abs().sum())) + U * float(ref["loss"])
    losses = [out["loss"]] + ([loss_only] if loss_only is not None else [])
    errs = [abs(float(l) - PRIOR - float(ref["loss"])) for l in losses]
    assert max(errs) <= 2 * lbound, (name, errs, lbound)
    return "logit %.3g dx %.3g dW %.3g db %.3g loss %.3g" % (
        chk_z.worst, chk_x.worst, worst(out["dW"], 0.25 + ref["dW"] * gs, dw_b), worst(out["db"], -0.125 + ref["db"] * gs, db_b),
        max(errs) / (2 * lbound))


@pytest.mark.parametrize("case", C.MASK_CASES, ids=ident)
def test_mask_predict_bce(H, case):
    """u2_mask_predict_bce on the pixel-order input, and for the phased cases on the re-ordered input as well: the same checks,
    and logit_out bit for bit.  u2_mask_predict_bce_stats in the case's own form: the four counters equal the counts formed from
    logit_out and the targets, its loss within the same bound."""
    n, side, phased, k = case
    p = side * side
    x, w, bias, cls, tgt = (t.to(DEV) for t in C.mask_case(*case))
    gs = C.f32(1.0 / (n * p))
    name = "mask %s" % ident(case)
    xin = C.to_phases(x, side) if phased else x
    ls, cnt = prior(), counters(4)
    H.call("u2_mask_predict_bce_stats", xin, w, bias, cls, tgt, ls, cnt, n, p, C.MASK_C, side if phased else 0)
    plain = run_mask(H, x, w, bias, cls, tgt, n, p, gs, 0)
    print("LOSS64 %s plain: %s" % (name, check_mask(name, plain, x, w, bias, cls, tgt, gs, None if phased else ls)))
    zk = plain["z"]
    if phased:
        ph = run_mask(H, xin, w, bias, cls, tgt, n, p, gs, side)
        print("LOSS64 %s phased: %s" % (name, check_mask(name + " phased", ph, x, w, bias, cls, tgt, gs, ls)))
        assert torch.equal(ph["z"].view(torch.int16), zk.view(torch.int16)), "logit_out differs between the two orders"
    on, hot = tgt != 0, zk.float() > 0
    want = [int((hot & ~on).sum()), int((~hot & on).sum()), int(on.sum()), n * p]
    assert cnt.tolist() == [a + b for a, b in zip(CNT_PRIOR, want)], (cnt.tolist(), want)
    assert float(zk.float().abs().max()) > 20


# =================================================================================================
# the RPN's level loss
def run_rpn(H, c, b, hw, lpo, lpd, gs, labels=None):
    obj, dlt = c["obj"].to(DEV), None if c["dlt"] is None else c["dlt"].to(DEV)
    dobj, ddlt = nans(obj.shape), None if dlt is None else nans(dlt.shape)
    loss = torch.tensor([PRIOR, -PRIOR], dtype=torch.float32, device=DEV)
    lab = (c["labels"] if labels is None else labels).to(DEV)
    H.call("u2_rpn_loss_level", obj, dlt, lab, c["match"].to(DEV), c["gt"].to(DEV), c["anchors"].to(DEV), dobj, ddlt, loss,
           b, hw, c["a"], lpo, lpd, c["atot"], c["lvl_off"], c["G"], gs)
    return dobj, ddlt, loss


@pytest.mark.parametrize("case", C.RPN_CASES, ids=ident)
def test_rpn_loss_level(H, case):
    """u2_rpn_loss_level as the second of two levels.  The objectness gradient within gscale (sigma (1 - sigma) exp_rel + 2 u sigma
    + u |sigma - t|), doubled, exactly 0 on ignored anchors; the delta gradient the exact sign times bf16(gscale), either sign
    allowed only within get_deltas' fp32 error - at most the case's constructed ties; every pad column exactly 0 and every row
    written; both losses within test_rpn_loss_full_size's error sums plus acc_bound(A or 4 A terms per position + 8, grid)."""
    b, hw, a, lpo, lpd, fused = case
    c = C.rpn_case(*case)
    gs = C.f32(1.0 / (256 * b))
    dobj, ddlt, loss = run_rpn(H, c, b, hw, lpo, lpd, gs)
    o, d, lab, mt = (t.to(DEV) for t in C.rpn_views(c))
    ref = R.rpn_level_ref(o, d, lab, mt, c["gt"].to(DEV), c["anchors"].to(DEV), a)
    name = "rpn %s" % ident(case)
    z, t, valid, pos = ref["z"], ref["t"], ref["valid"], ref["pos"]
    sg = torch.sigmoid(z)
    zero = torch.zeros_like(z)
    e = torch.where(valid, gs * (sg * (1 - sg) * exp_rel(z) + 2 * U * sg + U * (sg - t).abs()) + 2.0 ** -140, zero)
    chk = Check(name + ": dobj", 5e-3)
    chk.add(dobj[..., :a], ref["dobj"] * gs, 2 * e)
    chk.done()
    gd = (dobj[..., a: 5 * a] if fused else ddlt[..., : 4 * a]).reshape(b, hw, a, 4)
    d64, ed = get_deltas64(ref["src"], ref["dst"], (1.0, 1.0, 1.0, 1.0))
    amb = check_l1_grad(name + ": deltas", gd[pos], ref["pred"], d64, ed, C.bf16_of(gs), exact_zero=ref["df"] == 0)
    assert amb <= c["ties"], (amb, c["ties"])
    assert bool((gd[~pos] == 0).all()), "a delta gradient off the positives"
    if fused:
        assert bool((dobj[..., 15:] == 0).all())
    else:
        assert bool((dobj[..., a:] == 0).all()) and bool((ddlt[..., 4 * a:] == 0).all())
    grid = C.rpn_grid(b, hw)
    rows = -(-b * hw // (256 * grid))
    y = torch.exp(-z.abs())
    lp = torch.log1p(y)
    li = ref["terms"]
    e_lc = float(torch.where(valid, exp_rel(z) * y / (1 + y) + 4 * U * lp + TINY + 2 * U * (li.abs() + lp), zero).sum())
    b_c = e_lc + acc_bound(rows * a + 8, grid, float(li.abs().sum())) + U * float(ref["loss_cls"])
    b_l = float(ed.sum()) + acc_bound(rows * 4 * a + 8, grid, float(ref["loss_loc"])) + U * float(ref["loss_loc"])
    e_c, e_l = abs(float(loss[0]) - PRIOR - float(ref["loss_cls"])), abs(float(loss[1]) + PRIOR - float(ref["loss_loc"]))
    print("LOSS64 %s: dobj %.3g, losses %.3g %.3g, %d of %d ties open" % (
        name, chk.worst, e_c / (2 * b_c), e_l / (2 * b_l), amb, c["ties"]))
    assert e_c <= 2 * b_c, (float(loss[0]), float(ref["loss_cls"]), b_c)
    assert e_l <= 2 * b_l, (float(loss[1]), float(ref["loss_loc"]), b_l)


@pytest.mark.parametrize("case", [C.RPN_CASES[2], C.RPN_CASES[-1]], ids=ident)
def test_rpn_loss_level_without_a_label(H, case):
    """Every label -1: exactly 0 is added to both losses and every gradient row is written as zeros."""
    b, hw, a, lpo, lpd, fused = case
    c = C.rpn_case(*case)
    dobj, ddlt, loss = run_rpn(H, c, b, hw, lpo, lpd, 1.0, torch.full_like(c["labels"], -1))
    assert loss.tolist() == [PRIOR, -PRIOR] and bool((dobj == 0).all()) and (fused or bool((ddlt == 0).all()))


# =================================================================================================
# the box head's L1
@pytest.mark.parametrize("weights", C.BOX_WEIGHTS, ids=lambda w: "w%d" % w[0])
@pytest.mark.parametrize("case", C.BOX_CASES, ids=ident)
def test_box_reg_l1(H, case, weights):
    """u2_box_reg_l1: the exact sign times bf16(gscale) on the four columns of the foreground rows (either sign only within
    get_deltas' fp32 error: at most the constructed ties, which must be exactly 0), exactly 0 everywhere else; the loss within
    get_deltas' error sum plus acc_bound(4 terms per row + 8, grid)."""
    r, lp, all_bg = case
    pred, prop, gt, lab, ties = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in C.box_case(r, lp, all_bg, weights))
    gs = C.f32(1.0 / r)
    dpred, loss = nans((r, lp)), prior()
    H.call("u2_box_reg_l1", pred, prop, gt, lab, dpred, loss, r, lp, C.BOX_BG, *weights, gs)
    ref = R.box_l1_ref(pred, prop, gt, lab, C.BOX_BG, weights)
    fg = ref["fg"]
    gr = dpred.to(F64)
    assert bool((gr[~fg] == 0).all()) and bool((gr[:, 4:] == 0).all())
    d64, e = get_deltas64(prop, gt, weights)
    name = "box_l1 %s" % ident(case)
    amb = 0
    if bool(fg.any()):
        amb = check_l1_grad(name, gr[fg][:, :4], pred[fg][:, :4], d64[fg], e[fg], C.bf16_of(gs), exact_zero=ref["df"][fg] == 0)
    assert amb <= ties, (amb, ties)
    grid = C.box_grid(r)
    a = float(ref["loss"])
    bound = float(e[fg].sum()) + acc_bound(4 * -(-r // (256 * grid)) + 8, grid, a) + U * a
    err = abs(float(loss) - PRIOR - a)
    print("LOSS64 %s w%d: loss %.3g, %d of %d ties open" % (name, weights[0], err / (2 * bound), amb, ties))
    assert err <= 2 * bound, (float(loss), a, bound)
    if all_bg:
        assert float(loss) == PRIOR


# =================================================================================================
# what the launchers refuse, and launches without rows
def test_refusals_are_decided_before_any_launch(H):
    """Every refusal returns -1 and leaves the outputs as they were."""
    z = torch.zeros((2, 4, 4, 64), dtype=BF16, device=DEV)
    t = torch.zeros((2, 16, 16), dtype=torch.uint8, device=DEV)
    acc, ls, cnt = nans((2, 4, 4, 64), torch.float32), prior(), prior()
    for lp, nc, ignore in ((40, 33, 255), (24, 28, 255), (36, 28, 255), (32, 28, -1), (32, 28, 256)):
        assert status(H, "u2_semseg_upsample_ce", z, t, acc, ls, cnt, 2, 4, 4, lp, nc, ignore) == -1, (lp, nc, ignore)
    assert bool(acc.isnan().all()) and float(ls) == PRIOR and float(cnt) == PRIOR

    n, p = 2, 36
    x = torch.zeros((n, p, 256), dtype=BF16, device=DEV)
    w, bias = torch.zeros((3, 256), device=DEV), torch.zeros(3, device=DEV)
    cls, tgt = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros((n, p), dtype=torch.uint8, device=DEV)
    dx, dw, db, zk, c4 = nans(x.shape), prior(3 * 256), prior(3), nans((n, p)), counters(4)
    for pp, ch, side in ((36, 128, 0), (25, 256, 5), (36, 256, 4)):   # C = 128; phased with an odd side; phased with side^2 != P
        rc = status(H, "u2_mask_predict_bce", x, w, bias, cls, tgt, dx, dw, db, ls, zk, n, pp, ch, 1.0, side, None)
        assert rc == -1, (pp, ch, side)
        assert status(H, "u2_mask_predict_bce_stats", x, w, bias, cls, tgt, ls, c4, n, pp, ch, side) == -1, (pp, ch, side)
    assert status(H, "u2_mask_predict_bce_stats", x, w, bias, cls, tgt, ls, None, n, p, 256, 0) == -1      # no counters
    assert bool(dx.isnan().all()) and bool(zk.isnan().all()) and bool((dw == PRIOR).all()) and bool((db == PRIOR).all())
    assert c4.tolist() == CNT_PRIOR[:4] and float(ls) == PRIOR

    b, hw = 2, 9
    obj, dlt = torch.zeros((b, hw, 40), dtype=BF16, device=DEV), torch.zeros((b, hw, 40), dtype=BF16, device=DEV)
    lab, mt = torch.zeros((b, hw * 5), dtype=torch.int8, device=DEV), torch.zeros((b, hw * 5), dtype=torch.int32, device=DEV)
    gt, an = torch.ones((b, 1, 4), device=DEV), torch.ones((hw * 5, 4), device=DEV)
    dobj, ddlt, l2 = nans(obj.shape), nans(dlt.shape), prior(2)
    refused = [(obj, dlt, dobj, ddlt, 5, 8, 24),      # A = 5
               (obj, dlt, dobj, ddlt, 3, 12, 16),     # LPo = 12
               (obj, None, dobj, None, 2, 16, 0),     # fused with A = 2
               (obj, None, dobj, None, 3, 8, 0),      # fused with LPo = 8
               (obj, None, dobj, ddlt, 3, 16, 0),     # fused with ddlt given
               (obj, dlt, dobj, ddlt, 2, 8, 8)]       # separate with LPd = 8
    for o, d, go, gd, a, lpo, lpd in refused:
        rc = status(H, "u2_rpn_loss_level", o, d, lab, mt, gt, an, go, gd, l2, b, hw, a, lpo, lpd, hw * a, 0, 1, 1.0)
        assert rc == -1, (a, lpo, lpd)
    assert bool(dobj.isnan().all()) and bool(ddlt.isnan().all()) and l2.tolist() == [PRIOR, PRIOR]

    zr, lr, dr = torch.zeros((4, 8), dtype=BF16, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), nans((4, 8))
    assert status(H, "u2_softmax_ce_stats", zr, lr, dr, ls, 4, 8, 8, 1.0, None, 7) == -1                    # no counters
    assert bool(dr.isnan().all()) and float(ls) == PRIOR
    torch.cuda.synchronize()


def test_launches_without_rows_leave_the_outputs_alone(H):
    zr, lr, dr = torch.zeros((4, 8), dtype=BF16, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), nans((4, 8))
    ls, c5 = prior(), counters(5)
    assert status(H, "u2_softmax_ce", zr, lr, dr, ls, 0, 8, 8, 1.0) == 0
    assert status(H, "u2_softmax_ce_stats", zr, lr, dr, ls, 0, 8, 8, 1.0, c5, 7) == 0
    boxes = torch.ones((4, 4), device=DEV)
    assert status(H, "u2_box_reg_l1", zr, boxes, boxes, lr, dr, ls, 0, 8, 80, 10.0, 10.0, 5.0, 5.0, 1.0) == 0
    x = torch.zeros((1, 4, 256), dtype=BF16, device=DEV)
    w, bias = torch.zeros((1, 256), device=DEV), torch.zeros(1, device=DEV)
    cls, tgt = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros((1, 4), dtype=torch.uint8, device=DEV)
    dx, dw, db, zk = nans(x.shape), prior(256), prior(1), nans((1, 4))
    assert status(H, "u2_mask_predict_bce", x, w, bias, cls, tgt, dx, dw, db, ls, zk, 0, 4, 256, 1.0, 0, None) == 0
    assert status(H, "u2_mask_predict_bce_stats", x, w, bias, cls, tgt, ls, c5, 0, 4, 256, 0) == 0
    torch.cuda.synchronize()
    assert bool(dr.isnan().all()) and bool(dx.isnan().all()) and bool(zk.isnan().all()) and float(ls) == PRIOR
    assert bool((dw == PRIOR).all()) and float(db) == PRIOR and c5.tolist() == CNT_PRIOR
