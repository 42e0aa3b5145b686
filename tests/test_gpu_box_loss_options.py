"""u2_sigmoid_ce and u2_box_reg_loss (u2seg_amd/csrc/losses.hip) against the float64 restatements of tests/box_loss_refs.py,
through layers/functional.py and directly through the C ABI, and the ROI heads with the options on against the torch
definitions of u2seg_amd/modeling/box_losses.py on the inputs the HIP path was given.

Bounds (u = 2^-24, fp contraction off, exp_rel / TINY of tests/test_gpu_heads_full_size.py; every bound is doubled for the
second-order terms, and Check adds the rounding of the bf16 output):

Sigmoid CE, per element.  e = __expf(-|x|) errs by de = exp_rel(|x|) relative.  1 + e and the division round once each (two
u allowed for the division), e * inv once more: sigmoid errs by at most (2 de + 5 u) relative.  (sg - t), * w, * gscale: u each:
    |err| <= gscale w (sg (2 de + 5 u) + 3 u |sg - t|) + TINY.
Loss term max(x, 0) - x t + log1pf(e): the first two are exact (t is 0 or 1); log1p moves by de e / (1 + e) <= de log1p(e) for
the error of e and log1pf itself by 4 u; two sums and the weight: 3 u:
    |err| <= w ((de + 4 u) log1p(e) + 3 u (|max(x, 0) - x t| + log1p(e))) + TINY,
and the sum: a lane adds its columns, then its rows, the wave 6 levels, the work-group 4, one atomic per work-group:
depth u sum |terms| (recursive summation).

Box losses.  Decode (box_regression.py:78-116 in fp32), with pw the proposal's width, cx its centre, dx = d0 / wx:
    pcx: width u |pw|, centre u |cx| + u |pw| / 2, dx u, dx pw u, the sum u:   e_c = u (3 |dx pw| + 1.5 |pw| + |cx| + |pcx|)
    bw = expf(dw) pw: dw = d2 / ww u |dw| (the fp32 clamp: the same), expf 2 u, the product u:   e_w = (|dw| + 5) u bw
    x1, x2 = pcx -+ bw / 2:   e_x = e_c + e_w / 2 + u max(|x1|, |x2|)
and the same for y.  First order, the loss moves by sum_q |dL/db_q| e_q and the box gradient gb = dL/db by
sum_j |d2L/db_q db_j| e_j (float64 autograd, taken twice).  Evaluating the loss in fp32 adds roundings of its O(1) terms:
24 u (1 + |L|); evaluating gb adds 64 u S with S = 1 / min(bw, bh) + 1 / min(gw, gh): every piece of gb (dI / U <= 1 / side,
dA / U, dC / C, d dist / diag, term d diag / diag, alpha dv / d side <= 2.6 / side) is below 3 S and there are about 20 roundings.
Back through the decode: gd0 = (gb0 + gb2) pw / wx, gd2 = (gb2 - gb0) bw / (2 ww):
    e(gd0) = (e(gb0) + e(gb2)) pw / wx + 6 u (|gb0| + |gb2|) pw / wx
    e(gd2) = ((e(gb0) + e(gb2)) + (|dw| + 8) u (|gb0| + |gb2|)) bw / (2 ww),  nothing through a clamp (exactly 0).
Rows in which a max / min pair or an overlap test lies within 4 e_x of its switching point are ambiguous: the kernel's
gradient must lie between the smallest and the largest of the float64 gradients at the 16 corners b +- 8 e_x (either branch,
or torch's half-and-half at an exact tie).  Away from the constructed rows they may be at most 1 % of the foreground rows.
Smooth L1: the target carries get_deltas' fp32 error e_t (get_deltas64); df = pred - target: e_t + u |df|; the loss and its
gradient are continuous in df across |df| = beta and 0: value |df| / beta-Lipschitz below beta, 1 above; gradient 1 / beta.
"""
import json
import math
import os

import pytest
import torch

from tests import box_loss_refs as refs
from tests.test_gpu_heads_full_size import TINY, U, exp_rel, get_deltas64
from tests.test_gpu_norm_full_size import Check, rnd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
CLAMP = math.log(1000.0 / 16)
STAGE_WEIGHTS = [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)]
KINDS = ["smooth_l1", "giou", "diou", "ciou"]
BETA = 0.5
WORST = {}   # kind -> worst ratio to the bound over the session (printed by the last box test)


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

    return _hip


# =================================================================================================
# sigmoid cross-entropy
# =================================================================================================
def sigmoid_inputs(R, NC, LP, seed):
    """Drawn on the host, so that every machine tests the same rows."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((R, LP), generator=g) * 3
    if R > 16:
        z[0:8, :NC] = (torch.randn((8, NC), generator=g) * 25).clamp(-60, 60)   # saturated
        z[8:12, :NC] = 0.0                                                                   # zeros: every column ties
        z[12:16, :NC] = z[12:16, :NC].round()                                                # ties between columns
        z[12:14, NC - 1] = z[12:14, :NC].amax(1)                                             # ... the background among them
    else:
        z[0, 0], z[0, 1] = 60.0, -60.0
    z[:, NC:] = 1e4
    z = z.to(BF16)
    bg = NC - 1
    lab = torch.full((R,), bg, dtype=torch.int64)
    fgr = torch.rand(R, generator=g) < 0.25
    lab[fgr] = torch.randint(0, bg, (int(fgr.sum()),), generator=g)
    if R > 16:
        lab[0:4] = torch.tensor([0, 1, 2, 3])        # saturated rows with a positive column
        lab[16:32] = bg                                          # a run of all-background rows
    else:
        lab[0] = 0
    w = torch.rand(bg, generator=g) + 0.5
    w[torch.rand(bg, generator=g) < 0.3] = 0.0       # the federated mask drops classes
    w[0] = 1.0
    return z.to(DEV), lab.to(DEV), w.to(DEV)


def sigmoid_expect(z, lab, NC, LP, w, gs):
    """(reference gradient [R, NC - 1], its bound, reference loss sum / R, its bound) for the launch geometry of u2_sigmoid_ce."""
    R = z.shape[0]
    k = NC - 1
    zz = z[:, :NC].to(F64)
    terms, grad = refs.sigmoid_ce_terms(zz, lab, k, w)
    x = zz[:, :k]
    t = (torch.arange(k, device=z.device)[None] == lab[:, None]).to(F64)
    wv = torch.ones(k, dtype=F64, device=z.device) if w is None else w.to(F64)
    de = exp_rel(x)
    sg = torch.sigmoid(x)
    e_g = gs * wv * (sg * (2 * de + 5 * U) + 3 * U * (sg - t).abs()) + TINY
    l1p = torch.log1p(torch.exp(-x.abs()))
    e_t = wv * ((de + 4 * U) * l1p + 3 * U * ((x.clamp_min(0) - x * t).abs() + l1p)) + TINY
    grid = min((R + 3) // 4, 1024)
    cols = -(-(LP // 8) // 64) * 8 if LP % 8 == 0 else -(-LP // 64)
    depth = cols + -(-R // (grid * 4)) + 6 + 4 + grid
    ref_l = float(terms.sum()) / R
    bound = (float(e_t.sum()) + depth * U * float(terms.abs().sum())) / R + 2 * U * abs(ref_l)
    return grad * gs, e_g, ref_l, bound


def check_sigmoid_grad(name, d, NC, w, ref, e):
    k = NC - 1
    chk = Check(name, None)
    chk.add(d[:, :k], ref, 2 * e)
    chk.done()
    assert float(d[:, k:].abs().max()) == 0.0, name + ": the background column and the pads"
    if w is not None:
        assert float(d[:, :k][:, w == 0].float().abs().sum()) == 0.0, name + ": columns of weight 0"
    return chk.worst


@pytest.mark.parametrize("R,NC,LP", [(1, 3, 32), (63, 801, 832), (513, 801, 832), (2049, 1025, 1056), (37, 11, 13)])
def test_sigmoid_ce(F, H, R, NC, LP):
    """(37, 11, 13): rows that are no multiple of 8 wide take the kernel's 2-byte accesses."""
    z, lab, w = sigmoid_inputs(R, NC, LP, 100 + R)
    gs = 1.0 / R
    # C ABI, NULL weight, with counters: against float64 and against u2_softmax_ce_stats' counts on the same logits
    d = torch.full((R, LP), 7.0, dtype=BF16, device=DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    cnt = torch.full((5,), 1000, dtype=torch.int32, device=DEV)
    H.call("u2_sigmoid_ce", z, lab, None, d, loss, R, NC, LP, gs, cnt, NC - 1)
    ref, e, ref_l, bound = sigmoid_expect(z, lab, NC, LP, None, gs)
    worst = check_sigmoid_grad("sigmoid_ce %d (C ABI)" % R, d, NC, None, ref, e)
    err_a = abs(float(loss) / R - ref_l)
    print("sigmoid_ce R=%d NC=%d: worst ratio %.3g; loss %.9g ref %.9g error %.3g of bound %.3g" % (
        R, NC, worst, float(loss) / R, ref_l, err_a, 2 * bound))
    assert err_a <= 2 * bound
    cnt_sm = torch.full((5,), 1000, dtype=torch.int32, device=DEV)
    H.call("u2_softmax_ce_stats", z, lab, torch.empty_like(z), torch.zeros(1, dtype=torch.float32, device=DEV), R, NC, LP, gs,
           cnt_sm, NC - 1)
    assert torch.equal(cnt, cnt_sm) and int(cnt[0]) == 1000 + R, (cnt.tolist(), cnt_sm.tolist())
    # layers/functional.py, a weight vector with zeros, no counters
    zd = z.detach().requires_grad_(True)
    out = F.sigmoid_cross_entropy(zd, lab, NC, w)
    out.backward()
    ref, e, ref_l, bound = sigmoid_expect(z, lab, NC, LP, w, gs)
    worst = check_sigmoid_grad("sigmoid_ce %d (weights)" % R, zd.grad, NC, w, ref, e)
    err_b = abs(float(out.detach()) - ref_l)
    print("sigmoid_ce R=%d NC=%d weighted: worst ratio %.3g; loss %.9g ref %.9g error %.3g of bound %.3g" % (
        R, NC, worst, float(out.detach()), ref_l, err_b, 2 * bound))
    assert err_b <= 2 * bound


def test_sigmoid_ce_no_rows(F, H):
    NC, LP = 801, 832
    z = torch.zeros((4, LP), dtype=BF16, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    d = torch.full((4, LP), 7.0, dtype=BF16, device=DEV)
    loss = torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    cnt = torch.full((5,), 1000, dtype=torch.int32, device=DEV)
    H.call("u2_sigmoid_ce", z, lab, None, d, loss, 0, NC, LP, 1.0, cnt, NC - 1)      # R == 0: nothing is launched
    assert float(loss) == 3.0 and bool((cnt == 1000).all()) and bool((d == 7.0).all())
    zd = z[:0].detach().requires_grad_(True)
    out = F.sigmoid_cross_entropy(zd, lab[:0], NC)
    out.backward()
    assert float(out) == 0.0 and zd.grad.shape == (0, LP)
    with pytest.raises(RuntimeError):
        H.call("u2_sigmoid_ce", z, lab, None, d, loss, 4, 900, LP, 1.0, None, 899)   # NC > LP is refused


# =================================================================================================
# box regression losses
# =================================================================================================
N_PLANTED = 8


def box_inputs(R, weights, kind, seed, LP=32):
    """Boxes drawn as test_box_reg_l1_full_size draws them, 25 % foreground; with R >= 65 the first rows are constructed.
    Drawn on the host, so that every machine tests the same rows."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((R, 2), generator=g) * torch.tensor([1300.0, 780.0])
    wh = 2 + torch.rand((R, 2), generator=g) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((R, 4), generator=g) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    lab = torch.where(torch.rand(R, generator=g) < 0.25,
                      torch.randint(0, 800, (R,), generator=g), torch.full((R,), 800))
    pred = torch.randn((R, LP), generator=g)
    if R == 1:
        lab[0] = 3
    if R >= 65:
        lab[:N_PLANTED] = 3
        pred[:N_PLANTED, :4] = 0
        grow = wh[:N_PLANTED].repeat(1, 2) * torch.tensor([-0.3, -0.3, 0.3, 0.3])
        gt[0] = prop[0] + 5000.0                     # disjoint: the intersection is masked to 0
        gt[1] = prop[1] + grow[1]                    # the prediction (deltas 0: the proposal) inside the ground truth
        gt[2] = prop[2] - 0.5 * grow[2]              # the ground truth inside the prediction
        gt[3] = prop[3]                              # prediction = ground truth (up to the decode's roundings: ambiguous)
        gt[4] = prop[4] + grow[4]
        pred[4, 2] = 5.0 * weights[2]                # dw = 5 above the clamp: no gradient through it
        gt[5] = prop[5]
        gt[5, 2] = gt[5, 0] + 1                      # a ground truth 1 px wide
        tgt = refs.get_deltas(prop[6:8].to(F64), gt[6:8].to(F64), weights)
        pred[6, :4] = (tgt[0] + torch.tensor([0.5, -0.5, 0.9, -0.9], dtype=F64) * BETA).float()   # |d| < beta
        pred[7, :4] = (tgt[1] + torch.tensor([1.1, -1.1, 3.0, -3.0], dtype=F64) * BETA).float()   # |d| > beta
    return pred.to(BF16).to(DEV), prop.to(DEV), gt.to(DEV), lab.to(DEV)


def box_expect(kind, pred, prop, gt, fg, weights, gs):
    """Foreground rows only.  Returns dict(loss rows, e_loss rows, grad [n, 4] (x gs), e_grad, lo, hi, ambiguous, clamped)."""
    d = pred[fg][:, :4].to(F64)
    p, g = prop[fg].to(F64), gt[fg].to(F64)
    wx, wy, ww, wh = weights
    if kind == "smooth_l1":
        tgt, e_t = get_deltas64(prop[fg], gt[fg], weights)          # (e_t is doubled there already)
        dl = d.clone().requires_grad_(True)
        rows = refs.smooth_l1_rows(dl, tgt, BETA)
        (grad,) = torch.autograd.grad(rows.sum(), dl)
        df = d - tgt
        e_df = e_t + U * df.abs()
        e_loss = ((df.abs() / BETA).clamp(max=1) * e_df).sum(1) + 8 * U * rows.detach()
        e_grad = e_df / BETA + 2 * U * grad.abs()
        none = torch.zeros(len(d), dtype=torch.bool, device=d.device)
        return dict(rows=rows.detach(), e_rows=e_loss, grad=grad * gs, e_grad=e_grad * gs + TINY, amb=none,
                    clamped=torch.zeros_like(d, dtype=torch.bool))
    b0, cl = refs.decode(d, p, weights, CLAMP)
    clamped = torch.zeros_like(d, dtype=torch.bool)
    clamped[:, 2:] = cl
    # the decode's error per coordinate
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    cx, cy = p[:, 0] + 0.5 * pw, p[:, 1] + 0.5 * ph
    dx, dy = d[:, 0] / wx, d[:, 1] / wy
    dw, dh = (d[:, 2] / ww).clamp(max=CLAMP), (d[:, 3] / wh).clamp(max=CLAMP)
    bw, bh = b0[:, 2] - b0[:, 0], b0[:, 3] - b0[:, 1]
    e_cx = U * (3 * (dx * pw).abs() + 1.5 * pw + cx.abs() + (dx * pw + cx).abs())
    e_cy = U * (3 * (dy * ph).abs() + 1.5 * ph + cy.abs() + (dy * ph + cy).abs())
    e_w, e_h = (dw.abs() + 5) * U * bw, (dh.abs() + 5) * U * bh
    e_x = e_cx + 0.5 * e_w + U * torch.maximum(b0[:, 0].abs(), b0[:, 2].abs())
    e_y = e_cy + 0.5 * e_h + U * torch.maximum(b0[:, 1].abs(), b0[:, 3].abs())
    e_b = torch.stack((e_x, e_y, e_x, e_y), 1)

    def at(b):
        """loss rows, gb = dL/db and (optionally) |Hessian| e_b at boxes b."""
        b = b.detach().requires_grad_(True)
        rows = refs.iou_loss_rows(kind, b, g)
        (gb,) = torch.autograd.grad(rows.sum(), b, create_graph=True)
        return b, rows, gb

    def to_deltas(gb):
        sx, sy = gb[:, 0] + gb[:, 2], gb[:, 1] + gb[:, 3]
        tx, ty = 0.5 * (gb[:, 2] - gb[:, 0]) * bw / ww, 0.5 * (gb[:, 3] - gb[:, 1]) * bh / wh
        out = torch.stack((sx * pw / wx, sy * ph / wy, tx, ty), 1)
        return torch.where(clamped, torch.zeros_like(out), out)

    b, rows, gb = at(b0)
    e_gb = torch.zeros_like(gb)
    for q in range(4):
        (hq,) = torch.autograd.grad(gb[:, q].sum(), b, retain_graph=True, allow_unused=True)
        if hq is not None:
            e_gb[:, q] = (hq.abs() * e_b).sum(1)
    gb, rows = gb.detach(), rows.detach()
    S = 1 / torch.minimum(bw, bh) + 1 / torch.minimum(g[:, 2] - g[:, 0], g[:, 3] - g[:, 1])
    e_gb = e_gb + 64 * U * S[:, None]
    ax, ay = gb[:, 0].abs() + gb[:, 2].abs(), gb[:, 1].abs() + gb[:, 3].abs()
    e_grad = torch.stack(((e_gb[:, 0] + e_gb[:, 2] + 6 * U * ax) * pw / wx, (e_gb[:, 1] + e_gb[:, 3] + 6 * U * ay) * ph / wy,
                          (e_gb[:, 0] + e_gb[:, 2] + (dw.abs() + 8) * U * ax) * bw / (2 * ww),
                          (e_gb[:, 1] + e_gb[:, 3] + (dh.abs() + 8) * U * ay) * bh / (2 * wh)), 1)
    e_grad = torch.where(clamped, torch.zeros_like(e_grad), e_grad)
    grad = to_deltas(gb)
    e_rows = (gb.abs() * e_b).sum(1) + 24 * U * (1 + rows.abs())
    # ambiguous rows: the hull of the gradients at the 16 corners b0 +- 8 e_b
    amb = refs.branch_margin(b0, g) <= 4 * e_b.amax(1)
    lo, hi = grad.clone(), grad.clone()
    if bool(amb.any()):
        for corner in range(16):
            s = torch.tensor([1.0 if corner >> q & 1 else -1.0 for q in range(4)], dtype=F64, device=d.device)
            _, _, gc = at(b0 + 8 * e_b * s)
            gc = to_deltas(gc.detach())
            lo, hi = torch.minimum(lo, gc), torch.maximum(hi, gc)
    return dict(rows=rows, e_rows=e_rows, grad=grad * gs, e_grad=e_grad * gs + TINY, amb=amb, clamped=clamped,
                lo=lo * gs, hi=hi * gs, box=b0, e_box=e_b, margin=refs.branch_margin(b0, g))


def check_box(name, kind, got_grad, got_loss, pred, prop, gt, lab, weights, norm, planted):
    R = pred.shape[0]
    gs = 1.0 / norm
    fg = (lab >= 0) & (lab < 800)
    gr = got_grad.to(F64)
    assert float(gr[:, 4:].abs().sum()) == 0.0, name + ": columns >= 4"
    if bool((~fg).any()):
        assert float(gr[~fg].abs().max()) == 0.0, name + ": background rows"
    ex = box_expect(kind, pred, prop, gt, fg, weights, gs)
    got = got_grad[fg][:, :4]
    assert float(got.to(F64)[ex["clamped"]].abs().sum()) == 0.0, name + ": a gradient through a clamped size delta"
    chk = Check(name, None)
    sure = ~ex["amb"]
    if bool(sure.any()):
        chk.add(got[sure], ex["grad"][sure], 2 * ex["e_grad"][sure])
    if bool(ex["amb"].any()):
        a = ex["amb"]
        e = 2 * ex["e_grad"][a]
        chk.add_interval(got[a], rnd(ex["lo"][a] - e), rnd(ex["hi"][a] + e), ex["grad"][a])
    chk.done()
    n_fg, n_amb = int(fg.sum()), int(ex["amb"].sum())
    free = ex["amb"].clone()
    free[: min(planted, n_fg)] = False              # the constructed rows come first and are foreground
    for i in torch.nonzero(free).flatten().tolist():
        print("%s: ambiguous row %d: decoded %s +- %s, gt %s, margin %.3g" % (
            name, i, ex["box"][i].tolist(), ex["e_box"][i].tolist(), gt[fg][i].tolist(), float(ex["margin"][i])))
    assert int(free.sum()) <= 0.01 * n_fg, "%s: %d ambiguous rows of %d" % (name, int(free.sum()), n_fg)
    grid = min((R + 255) // 256, 1024)
    depth = -(-R // (grid * 256)) + 8 + 4 + grid
    ref_l = float(ex["rows"].sum()) / norm
    bound = (float(ex["e_rows"].sum()) + depth * U * float(ex["rows"].abs().sum())) / norm + 2 * U * abs(ref_l)
    err = abs(float(got_loss) - ref_l)
    print("%s: %d fg rows, %d ambiguous; gradient worst ratio %.3g; loss %.9g ref %.9g error %.3g of bound %.3g" % (
        name, n_fg, n_amb, chk.worst, float(got_loss), ref_l, err, 2 * bound))
    WORST[kind] = max(WORST.get(kind, 0.0), chk.worst, err / (2 * bound + 1e-300))
    assert err <= 2 * bound, name
    return ex


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_box_reg_loss(F, H, kind, stage):
    weights = STAGE_WEIGHTS[stage]
    beta = BETA if kind == "smooth_l1" else 0.0
    for R in (1, 65, 2049):
        pred, prop, gt, lab = box_inputs(R, weights, kind, 1000 + 10 * stage + R)
        name = "box_reg_loss %s stage %d R=%d" % (kind, stage, R)
        pd = pred.detach().requires_grad_(True)
        loss = F.box_reg_loss(kind, pd, prop, gt, lab, 800, weights, R, beta, CLAMP)
        loss.backward()
        ex = check_box(name, kind, pd.grad, loss.detach(), pred, prop, gt, lab, weights, R, N_PLANTED if R >= 65 else 0)
        if R == 65:
            fg_rows = torch.nonzero((lab >= 0) & (lab < 800)).flatten()
            assert fg_rows[:N_PLANTED].tolist() == list(range(N_PLANTED))
            if kind != "smooth_l1":
                assert bool(ex["clamped"][4, 2]) and float(pd.grad[4, 2]) == 0.0 and float(pd.grad[4, 3]) != 0.0
                assert float(ex["rows"][0]) > 1.0       # disjoint
            # once directly through the C ABI: the same bits as through the autograd function
            d2 = torch.full_like(pred, 7.0)
            l2 = torch.zeros(1, dtype=torch.float32, device=DEV)
            H.call("u2_box_reg_loss", F.BOX_REG_LOSS_KINDS[kind], pred, prop, gt, lab, d2, l2, R, pred.shape[1], 800, *weights,
                   beta, CLAMP, 1.0 / R)
            assert torch.equal(d2, pd.grad) and torch.equal(l2[0] / R, loss.detach())
    if kind == KINDS[-1] and stage == 2:
        print("box_reg_loss: worst ratio to the bound per kind: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


@pytest.mark.parametrize("kind", KINDS)
def test_box_reg_loss_unpadded_rows(F, kind):
    """Rows of exactly four columns: the gradient leaves in 2-byte stores instead of 16-byte ones."""
    weights, R = STAGE_WEIGHTS[0], 65
    pred, prop, gt, lab = box_inputs(R, weights, kind, 1065, LP=4)
    pd = pred.detach().requires_grad_(True)
    loss = F.box_reg_loss(kind, pd, prop, gt, lab, 800, weights, R, BETA if kind == "smooth_l1" else 0.0, CLAMP)
    loss.backward()
    check_box("box_reg_loss %s LP=4" % kind, kind, pd.grad, loss.detach(), pred, prop, gt, lab, weights, R, N_PLANTED)


def test_box_reg_loss_refusals(F, H):
    pred = torch.zeros((4, 32), dtype=BF16, device=DEV)
    box = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 4, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    d = torch.full_like(pred, 7.0)
    loss = torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    args = (pred, box, box, lab, d, loss)
    H.call("u2_box_reg_loss", F.BOX_REG_LOSS_KINDS["giou"], *args, 0, 32, 800, 10.0, 10.0, 5.0, 5.0, 0.0, CLAMP, 1.0)   # R == 0
    assert float(loss) == 3.0 and bool((d == 7.0).all())
    for kind, beta in ((7, 0.0), (F.BOX_REG_LOSS_KINDS["smooth_l1"], 0.0)):          # unknown kind; beta == 0 is u2_box_reg_l1's
        with pytest.raises(RuntimeError):
            H.call("u2_box_reg_loss", kind, *args, 4, 32, 800, 10.0, 10.0, 5.0, 5.0, beta, CLAMP, 1.0)
    with pytest.raises(ValueError, match="eiou"):
        F.box_reg_loss("eiou", pred, box, box, lab, 800, (10.0, 10.0, 5.0, 5.0), 4)


# =================================================================================================
# the ROI heads with the options on: HIP against the torch definitions on the same inputs
# =================================================================================================
def test_heads_with_options_against_torch_definitions(F, monkeypatch):
    """The small configuration of tests/golden/model_small.json with sigmoid CE, the federated loss and GIoU on: one training
    step's three cascade stages, each loss against the torch definition on the inputs the kernels were given (teacher forced)
    within the bounds above; gradients reach cls_score and bbox_pred; at inference the scores are sigmoids."""
    from tests.golden.make_fixtures import det_fill
    from tests.test_box_loss_options_host import small_dataset
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.modeling import box_losses as BL
    from u2seg_amd.modeling import build_model, inference

    with open(os.path.join(ROOT, "tests", "golden", "model_small.json")) as f:
        fx = json.load(f)
    small_dataset("box_loss_options_small")
    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", True, "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", True,
                         "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou", "DATASETS.TRAIN", ("box_loss_options_small",),
                         "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0])
    torch.manual_seed(fx["seed"])
    model = build_model(cfg)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if not k.endswith("fed_loss_cls_weights"):
                v.copy_(det_fill(k, v.cpu()).to(DEV))
    model.train()
    cls_calls, box_calls = [], []
    sig, box = F.sigmoid_cross_entropy, F.box_reg_loss

    def sigmoid_cross_entropy(logits, labels, num_classes, class_weight=None, counters=None):
        out = sig(logits, labels, num_classes, class_weight, counters)
        cls_calls.append((logits.detach().clone(), labels.clone(), num_classes, class_weight.clone(), out.detach().clone()))
        return out

    def box_reg_loss(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0, scale_clamp=CLAMP):
        out = box(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta, scale_clamp)
        box_calls.append((kind, pred.detach().clone(), proposals.clone(), gt_boxes.clone(), labels.clone(), weights, normalizer,
                          out.detach().clone()))
        return out

    monkeypatch.setattr(F, "sigmoid_cross_entropy", sigmoid_cross_entropy)
    monkeypatch.setattr(F, "box_reg_loss", box_reg_loss)
    h, w = fx["image_hw"]
    batch = make_synthetic_batch(fx["num_images"], start_index=0, height=h, width=w, device=DEV)
    losses = model(batch)
    assert sorted(losses) == sorted(fx["losses"])                       # the loss dict's keys are unchanged
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert len(cls_calls) == 3 and len(box_calls) == 3
    for stage, (z, lab, nc, cw, got) in enumerate(cls_calls):
        # (the small dataset gives four classes a weight: the mask holds the present classes and what could be drawn of those)
        assert nc == 801 and cw.shape == (800,) and set(cw.tolist()) <= {0.0, 1.0} and int((cw[lab[lab < 800]] == 0).sum()) == 0
        assert int(cw.sum()) <= int(lab[lab < 800].unique().numel()) + 4
        R, LP = z.shape
        _, _, ref_l, bound = sigmoid_expect(z, lab, nc, LP, cw, 1.0 / R)
        want = float(BL.sigmoid_cross_entropy(z, lab, 800, cw))             # the torch definition, fp32 on the device
        # the definition's own fp32 error obeys the same per-term bound (its sum is no deeper)
        assert abs(float(got) - ref_l) <= 2 * bound and abs(float(got) - want) <= 4 * bound, (stage, float(got), want, ref_l, bound)
        assert float(got) == float(losses["loss_cls_stage%d" % stage].detach())
    for stage, (kind, pred, prop, gtb, lab, weights, norm, got) in enumerate(box_calls):
        assert kind == "giou" and tuple(weights) == STAGE_WEIGHTS[stage] and norm == pred.shape[0]
        fg = (lab >= 0) & (lab < 800)
        ex = box_expect(kind, pred, prop, gtb, fg, weights, 1.0 / norm)
        ref_l = float(ex["rows"].sum()) / norm
        R = pred.shape[0]
        grid = min((R + 255) // 256, 1024)
        bound = (float(ex["e_rows"].sum()) + (-(-R // (grid * 256)) + 12 + grid) * U * float(ex["rows"].abs().sum())) / norm \
            + 2 * U * abs(ref_l)
        want = float(BL.box_reg_loss(kind, pred, prop, gtb, lab, 800, weights, 0.0, CLAMP)) / norm
        assert abs(float(got) - ref_l) <= 2 * bound and abs(float(got) - want) <= 4 * bound, (stage, float(got), want, ref_l, bound)
        print("stage %d: loss_cls %.6g, loss_box_reg %.6g (torch definition %.6g), %d fg rows" % (
            stage, float(cls_calls[stage][4]), float(got), want, int(fg.sum())))
    for stage in range(3):
        p = model.roi_heads.box_predictor[stage]
        for layer in (p.cls_score, p.bbox_pred):
            gsum = float(layer.weight.grad.float().abs().sum())
            assert math.isfinite(gsum) and gsum > 0, (stage, layer)
    # inference: predict_probs hands sigmoids to the tail
    seen = []
    tail = inference.fast_rcnn_inference

    def fast_rcnn_inference(boxes, scores, *a, **k):
        seen.append(scores if isinstance(scores, torch.Tensor) else torch.cat(list(scores)))
        return tail(boxes, scores, *a, **k)

    monkeypatch.setattr(inference, "fast_rcnn_inference", fast_rcnn_inference)
    model.eval()
    with torch.no_grad():
        out = model([{"image": b["image"], "height": h, "width": w} for b in batch])
    (scores,) = seen
    scores = scores.reshape(-1, scores.shape[-1])
    assert scores.shape[1] == 801 and float(scores.min()) >= 0 and float(scores.max()) <= 1
    assert float((scores.sum(1) - 1).abs().min()) > 1e-3                # not a softmax: the rows do not sum to 1
    assert len(out) == fx["num_images"] and all("instances" in o for o in out)
