"""ROIAlign (u2seg_amd/csrc/roi.hip) and the head losses (losses.hip) at the training shapes (batch 16, the 800 x 1344 and
1024 x 1344 canvases, C = 256, 512 ROIs per image and box stage) against a float64 reference computed on the GPU.

At these sizes the kernels take paths the small parity tests never reach: the gather's second item per thread (q = 1, tile rows
4-7 at C = 256), its 48-bin LDS stage overflowing into reads of dout from L2, lists longer than GS_MAXL = 256 ROIs per (set,
image, level), tiles covered by dozens of ROIs (many 4-ROI batches through the parity-double-buffered row / column bits), the
row loop of u2_softmax_ce (R > 2048), the grid-stride loop of u2_rpn_loss_level (B * HW > 524 288), fp32 valid counts above
2^24 in the semantic loss, and thousands of work-groups sending their dW / db atomics to one class of the mask predictor.

Inputs are seeded and rounded to bf16; both sides see the same values.  Tolerances are derived from the kernels' fp32 arithmetic
(u = 2^-24, fp contraction off where the file says so), element by element, and hold for any order of the fp32 atomics and of
the gather's lists:  |got - bf16(ref)| <= e + step(|ref| + e)  (Check of test_gpu_norm_full_size), with e the bound of the
kernel's fp32 error before its last rounding, doubled for the second-order terms the first-order bound leaves out.

Fast intrinsics (derived, not measured): __expf(x) = exp2(x * log2 e) on v_exp_f32 (1 ulp): the product's rounding and the
rounding of log2 e are relative errors u |x| each in the argument, i.e. relative errors u |x| of the result, so
|__expf(x) / e^x - 1| <= (2 |x| + 4) u (+ one u |x| where the argument x = z - max is itself rounded); results below 2^-126 may
flush to 0 (an absolute 2^-126).  __logf(s) = v_log_f32(s) * ln 2 and log1pf: <= 4 u |result| + 2^-126 absolute.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.test_gpu_norm_full_size import Check, check_vec, rnd, step  # noqa: F401  (step: the unit Check bounds in)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -24
TINY = 2.0 ** -126          # fp32 results below this may flush to 0
F32 = np.float32


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


def exp_rel(x):
    """relative error bound of the kernels' __expf at argument x (module docstring)."""
    return (3 * x.abs() + 4) * U


# =================================================================================================
# ROIAlign: the float64 reference
# =================================================================================================
def roi_geom(rois, scale, P):
    """fp32 geometry exactly as oracle/roi_ops.c:44-55 (aligned=True, sampling_ratio=0) forms it, per ROI:
    ((sh, bh, gh), (sw, bw, gw)): start, bin size and samples per bin of each axis.  numpy float32: every operation rounds
    once, no contraction."""
    r = np.ascontiguousarray(rois, dtype=F32)
    sc, half, pf = F32(scale), F32(0.5), F32(P)
    sw, sh = r[:, 1] * sc - half, r[:, 2] * sc - half
    ew, eh = r[:, 3] * sc - half, r[:, 4] * sc - half
    rw, rh = ew - sw, eh - sh
    bh, bw = rh / pf, rw / pf
    gh, gw = np.ceil(rh / pf).astype(np.int64), np.ceil(rw / pf).astype(np.int64)
    return (sh, bh, gh), (sw, bw, gw)


def axis_tables(s0, bs, g, P, n, dev):
    """One axis of the separable ROIAlign (roi.hip:411-416): Wt[r, p, k] = sum over bin p's samples of their bilinear weight on
    pixel k (float64 weights of the fp32 positions `s0 + p*bs + (i + .5)*bs/g`, the oracle's association); Et bounds the
    kernels' deviation from Wt: they form the position as `(i + .5) * (bs/g)` (roi.hip:311, 528-529), which differs by about
    one ulp of the position - the weight is 1-Lipschitz in the position, so each of the <= 4 pixels around the sample gets
    that difference; St counts the samples touching each pixel (the atomic backward's accumulation chain).
    Returns (Wt, Et, St) [R, P, n] and the range of the valid sample positions."""
    R = s0.shape[0]
    G = max(int(g.max()) if R else 0, 1)
    with np.errstate(all="ignore"):
        a = s0[:, None] + np.arange(P, dtype=F32)[None, :] * bs[:, None]                       # sh + ph * bh
        t = ((np.arange(G, dtype=F32)[None, :] + F32(0.5)) * bs[:, None]) / g.astype(F32)[:, None]   # (iy + .5f) * bh / gh
        pos = a[:, :, None] + t[:, None, :]                                                    # [R, P, G] fp32
    ok = np.arange(G)[None, None, :] < g[:, None, None]
    ok = ok & ~((pos < -1) | (pos > n))                  # the skip rule
    rng = (float(pos[ok].min()), float(pos[ok].max())) if ok.any() else (0.0, 0.0)
    Wt = torch.zeros(R * P * n, dtype=F64, device=dev)
    Et = torch.zeros_like(Wt)
    St = torch.zeros_like(Wt)
    if ok.any():
        ri, pi, _ = np.nonzero(ok)
        base = torch.from_numpy((ri * P + pi) * n).to(dev)
        p = torch.from_numpy(pos[ok].astype(np.float64)).to(dev)
        tt = torch.from_numpy(np.broadcast_to(t[:, None, :], pos.shape)[ok].astype(np.float64)).to(dev)
        e_pos = 5 * U * (tt.abs() + p.abs()) + 2.0 ** -140
        p = p.clamp_min(0)
        lo = p.floor().long()
        top = lo >= n - 1
        lo = torch.where(top, torch.full_like(lo, n - 1), lo)
        hi = torch.where(top, lo, lo + 1)
        p = torch.where(top, lo.to(F64), p)
        lw = p - lo.to(F64)
        Wt.index_put_((base + lo,), 1 - lw, accumulate=True)
        Wt.index_put_((base + hi,), lw, accumulate=True)
        St.index_put_((base + lo,), torch.ones_like(lw), accumulate=True)
        St.index_put_((base + hi,), (hi != lo).to(F64), accumulate=True)
        for d in (-1, 0, 1, 2):
            k = lo + d
            m = (k >= 0) & (k < n)
            Et.index_put_(((base + k)[m],), e_pos[m], accumulate=True)
    return Wt.view(R, P, n), Et.view(R, P, n), St.view(R, P, n), rng


class RoiTables:
    """Both axes' tables of a group of ROIs at one level, and their per-ROI counts."""

    def __init__(self, rois, scale, P, Hl, Wl, dev=DEV):
        (sh, bh, gh), (sw, bw, gw) = roi_geom(rois, scale, P)
        self.Wy, self.Ey, self.Sy, ry = axis_tables(sh, bh, gh, P, Hl, dev)
        self.Wx, self.Ex, self.Sx, rx = axis_tables(sw, bw, gw, P, Wl, dev)
        self.gh, self.gw = torch.from_numpy(gh).to(dev), torch.from_numpy(gw).to(dev)
        self.cnt = (self.gh * self.gw).clamp_min(1).to(F64)
        self.prange = (ry, rx)
        self.gmax = int(max(gh.max(), gw.max())) if len(gh) else 0
        self.P = P
        # pixels a bin (or a ROI) reaches, including the position slack
        self.my, self.mx = (self.Wy + self.Ey) > 0, (self.Wx + self.Ex) > 0


def roi_fwd_ref(T, f, fa):
    """out = sum_y sum_x Wy Wx f / cnt and its bound: position term (Wy+Ey)(Wx+Ex)|f| - Wy Wx |f|; fp32 term: the kernel's
    tables sum g weights, wgt = a * b, acc += wgt * v (two roundings per term, roi.hip:171-223 / :324-408; the fall-back for
    bins wider than 16 pixels adds 4 products per sample), acc * inv_cnt."""
    Hl, Wl, C = f.shape
    P = T.P

    def apply(Wy, Wx, x):
        t = (Wy.reshape(-1, Hl) @ x.reshape(Hl, Wl * C)).view(-1, P, Wl, C)
        return torch.einsum("rqx,rpxc->rpqc", Wx, t)

    v = apply(T.Wy, T.Wx, f)
    s0 = apply(T.Wy, T.Wx, fa)
    s1 = apply(T.Wy + T.Ey, T.Wx + T.Ex, fa)
    ny, nx = T.my.sum(2).to(F64), T.mx.sum(2).to(F64)                       # [R, P]
    g4 = (4 * T.gh * T.gw).to(F64)[:, None, None]
    depth = torch.maximum(ny[:, :, None] * nx[:, None, :], g4) + (T.gh + T.gw).to(F64)[:, None, None] + 8
    ic = (1.0 / T.cnt)[:, None, None, None]
    return v * ic, 2 * ic * ((s1 - s0) + depth[..., None] * U * s1)


def roi_bwd_ref(T, d, Hl, Wl):
    """dfeat = sum_r sum_{p,q} Wy[r,p,y] Wx[r,q,x] d[r,p,q,:] (d already times gscale / cnt) and the two abs sums (plain,
    position-widened); the (ROI, bin) term count per pixel (the gather's chain) and the sample count (the atomic scatter's)."""
    P, C = T.P, d.shape[-1]

    def apply(Wy, Wx, x):
        u_ = torch.einsum("rqx,rpqc->rpxc", Wx, x)
        return (Wy.reshape(-1, Hl).t() @ u_.reshape(-1, Wl * C)).view(Hl, Wl, C)

    da = d.abs()
    v = apply(T.Wy, T.Wx, d)
    s0 = apply(T.Wy, T.Wx, da)
    s1 = apply(T.Wy + T.Ey, T.Wx + T.Ex, da)
    nterm = T.my.sum(1).to(F64).t() @ T.mx.sum(1).to(F64)      # [Hl, Wl]
    nsamp = T.Sy.sum(1).t() @ T.Sx.sum(1)
    return v, s0, s1, nterm, nsamp


# =================================================================================================
# 1: the reference itself, pinned to the C oracle on the inputs of test_roi_align_fwd_bwd
def test_roi_reference_matches_c_oracle():
    from oracle import ops as O

    g = torch.Generator().manual_seed(12)
    shapes, scales = [(24, 32), (12, 16), (6, 8), (3, 4)], [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    feats = [torch.randn((2, 64, h, w), generator=g).bfloat16().float() for h, w in shapes]
    xy = torch.rand((40, 2), generator=g) * 90
    wh = 2 + torch.rand((40, 2), generator=g) ** 2 * 120
    boxes = torch.cat([xy, xy + wh], 1)
    boxes[0] = torch.tensor([-20.0, -10.0, 40.0, 30.0])
    boxes[1] = torch.tensor([50.0, 40.0, 50.0, 40.0])
    bidx = torch.randint(0, 2, (40,), generator=g).float()
    rois = torch.cat([bidx[:, None], boxes], 1)
    lv = O.assign_boxes_to_levels(boxes, 2, 5)
    for ps in (7, 14):
        for l, (hl, wl) in enumerate(shapes):
            idx = torch.nonzero(lv == l)[:, 0]
            if not len(idx):
                continue
            fr = feats[l].clone().requires_grad_(True)
            out = O.roi_align(fr, rois[idx], ps, scales[l])                 # [R, C, P, P] fp32
            d = torch.randn(out.shape, generator=g).bfloat16().float()
            out.backward(d)
            r_np = rois[idx].numpy()
            T = RoiTables(r_np, scales[l], ps, hl, wl)
            fd = feats[l].permute(0, 2, 3, 1).to(DEV, F64)                 # [B, H, W, C]
            dd = d.permute(0, 2, 3, 1).to(DEV, F64) / T.cnt[:, None, None, None]
            gref = torch.zeros_like(fd)
            ob = torch.empty((len(idx), ps, ps, 64), dtype=F64, device=DEV)
            for b in range(2):
                m = torch.from_numpy((r_np[:, 0] == b).nonzero()[0]).to(DEV)
                if not len(m):
                    continue
                Tb = RoiTables(r_np[(r_np[:, 0] == b)], scales[l], ps, hl, wl)
                v, _ = roi_fwd_ref(Tb, fd[b], fd[b].abs())
                ob[m] = v
                gref[b] = roi_bwd_ref(Tb, dd[m], hl, wl)[0]
            # the oracle sums in fp32: at most 4 gh gw terms per output, and the scatter: bound 64 u of the abs sums
            got = out.detach().permute(0, 2, 3, 1).to(DEV, F64)
            assert float((got - ob).abs().max()) <= 64 * U * float(ob.abs().max() + 1e-30) + 1e-12, (ps, l)
            gg = fr.grad.permute(0, 2, 3, 1).to(DEV, F64)
            assert float((gg - gref).abs().max()) <= 64 * U * float(gref.abs().max() + 1e-30) + 1e-12, (ps, l)
            assert float(gref.abs().max()) > 0 and float(ob.abs().max()) > 0


# =================================================================================================
# 2: ROIAlign at the training shapes, every route of the training step
B_IMG = 16
EMPTY_IMG, MANY_IMG, CLUSTER_IMG = 15, 1, 2
SCALES = (0.25, 0.125, 0.0625, 0.03125)
GS_MAXL, STAGE_BINS, GS_KB = 256, 24576 // (2 * 256), 4
GS3 = float(F32(1.0 / 3))           # the kernels get the gradient scale as fp32: 0.33333334


def clip_boxes(bx, h, w):
    bx[:, [0, 2]] = np.clip(bx[:, [0, 2]], 0, w)
    bx[:, [1, 3]] = np.clip(bx[:, [1, 3]], 0, h)
    bx[:, 2] = np.maximum(bx[:, 2], bx[:, 0])
    bx[:, 3] = np.maximum(bx[:, 3], bx[:, 1])
    return bx


def roi_sets(Hc, Wc, seed):
    """Per image: 512 stage-1 ROIs (128 jittered around 5-40 gt boxes, the rest log-uniform), stages 2 / 3 moved by small
    deltas (scale 1/3 each), the foreground ROIs as the 14 x 14 mask set (scale 1).  Adversarial rows: empty boxes, boxes on
    the image and canvas edges, elongated boxes; image MANY_IMG with > 256 stage-1 ROIs on p2; image CLUSTER_IMG with 48 small
    ROIs inside one 8 x 8 tile of p2; image EMPTY_IMG without ROIs.  All boxes are clipped to their (ragged) image."""
    rng = np.random.default_rng(seed)
    sizes = [(Hc, Wc)] + [(Hc - 8 * int(rng.integers(0, 40)), Wc - 8 * int(rng.integers(0, 60))) for _ in range(B_IMG - 1)]
    s1, s2, s3, mk = [], [], [], []
    for b, (h, w) in enumerate(sizes):
        if b == EMPTY_IMG:
            continue
        ng = int(rng.integers(5, 41))
        gs = np.exp(rng.uniform(np.log(16), np.log(0.6 * min(h, w)), (ng, 2)))
        gs = np.minimum(gs, 400.0)                     # mask ROIs stay below p5: that level gets none of them
        gc = rng.uniform(0, 1, (ng, 2)) * [w, h]
        gt = np.concatenate([gc - gs / 2, gc + gs / 2], 1)
        gt = clip_boxes(gt, h, w)
        j = rng.integers(0, ng, 128)
        fg = gt[j] + rng.normal(0, 1, (128, 4)) * 0.08 * np.repeat(gs[j], 2, 1)
        fg = clip_boxes(fg, h, w)
        nr = 512 - 128
        lo_s = np.log(4.0)
        hi_s = np.log(100.0) if b == MANY_IMG else np.log(0.9 * min(h, w))
        ws = np.exp(rng.uniform(lo_s, hi_s, (nr, 2)))
        x0 = rng.uniform(0, 1, (nr, 2)) * ([w, h] - ws).clip(0)
        rest = np.concatenate([x0, x0 + ws], 1)
        k = 0
        for e in range(4):   # empty boxes
            rest[k] = [10.0 + e, 20.0, 10.0 + e + (0 if e % 2 else 30), 20.0 + (30 if e % 2 else 0)]
            k += 1
        rest[k] = [0, 0, w, h]; k += 1                                   # the whole image (p5)
        rest[k] = [0, h - 60, 90, h]; k += 1                             # corners / edges of the image
        rest[k] = [w - 40, 0, w, 25]; k += 1
        rest[k] = [w - 17, h - 11, w, h]; k += 1
        rest[k] = [0, 100, 15, 190]; k += 1
        for ew, eh in ((600, 20), (20, 400), (900, 40), (30, 700), (1300, 12)):   # elongated
            rest[k] = [5.5, 33.25, 5.5 + ew, 33.25 + eh]; k += 1
        if b == CLUSTER_IMG:   # one p2 tile: canvas pixels 320 ... 351 x 160 ... 191 (tile 10 x 5 of the 336 x 200 map)
            cw = rng.uniform(5, 28, (48, 2))
            c0 = np.array([320.0, 160.0]) + rng.uniform(0, 1, (48, 2)) * (32 - cw)
            rest[k: k + 48] = np.concatenate([c0, c0 + cw], 1)
            k += 48
        rest = clip_boxes(rest, h, w)
        st1 = np.concatenate([fg, rest])
        sz = np.repeat(np.maximum(st1[:, 2:] - st1[:, :2], 1.0), 2, 1)
        moved = []
        for _ in range(2):
            mv = st1 + rng.normal(0, 1, st1.shape) * 0.05 * sz
            empty = (st1[:, 2] <= st1[:, 0]) | (st1[:, 3] <= st1[:, 1])
            mv[empty] = st1[empty]
            moved.append(clip_boxes(mv, h, w))
        col = np.full((512, 1), float(b))
        s1.append(np.concatenate([col, st1], 1))
        s2.append(np.concatenate([col, moved[0]], 1))
        s3.append(np.concatenate([col, moved[1]], 1))
        mk.append(np.concatenate([col[:128], fg], 1))
    sets = [(np.concatenate(s).astype(F32), p, gsc) for s, p, gsc in ((s1, 7, GS3), (s2, 7, GS3), (s3, 7, GS3), (mk, 14, 1.0))]
    return sets


def level_shapes(Hc, Wc, c=256):
    return [(B_IMG, Hc // s, Wc // s, c) for s in (4, 8, 16, 32)]


class RoiCoverage:
    """The gather paths the inputs must reach, from the levels and the reference's weight tables."""

    def __init__(self):
        self.big_single, self.max_tile = 0, 0

    def add(self, T, Hl, Wl, cover):
        """cover [tiles_y, tiles_x]: ROIs of the (set, image, level) list with weight on each 8 x 8 tile, accumulated."""
        def tiles(Wt, n):
            m = TF.pad((Wt > 0).to(torch.float32), (0, -(-n // 8) * 8 - n))
            return m.view(Wt.shape[0], T.P, -1, 8).amax(3) > 0                      # [R, P, tiles]: bin p on the tile

        def span(m):
            ar = torch.arange(T.P, device=m.device)[None, :, None]
            hi = torch.where(m, ar, -1).amax(1)
            lo = torch.where(m, ar, T.P).amin(1)
            return (hi - lo + 1).clamp_min(0)                                       # [R, tiles]
        sy, sx = span(tiles(T.Wy, Hl)), span(tiles(T.Wx, Wl))
        # the stage holds a ROI's bin rectangle on a tile (rows span x columns span): > 48 bins read dout from L2
        self.big_single += int(((sy.amax(1) * sx.amax(1)) > STAGE_BINS).sum())
        cover += (sy > 0).to(F64).t() @ (sx > 0).to(F64)

    def done_list(self, cover):
        self.max_tile = max(self.max_tile, int(cover.max()))


@pytest.mark.parametrize("Hc", [800, 1024])
def test_roi_align_full_size(F, Hc):
    Wc = 1344
    torch.cuda.reset_peak_memory_stats()
    shapes = level_shapes(Hc, Wc)
    sets = roi_sets(Hc, Wc, seed=Hc)
    g = torch.Generator(device=DEV).manual_seed(Hc + 1)
    base = [torch.randn(s, generator=g, device=DEV, dtype=BF16) for s in shapes]
    w_sem = [torch.randn(s, generator=g, device=DEV, dtype=BF16) for s in shapes]
    w_rpn = [torch.randn(s, generator=g, device=DEV, dtype=BF16) for s in shapes]
    rois = [torch.from_numpy(r).to(DEV) for r, _, _ in sets]
    lvs = [F.assign_levels(r[:, 1:].contiguous(), 2, 5) for r in rois]
    douts = [torch.randn((r.shape[0], p, p, 256), generator=g, device=DEV, dtype=BF16) for r, (_, p, _) in zip(rois, sets)]
    lv_np = [lv.cpu().numpy() for lv in lvs]

    # ---- host-side coverage of the list paths (levels are bit-exact, test_roi_align_fwd_bwd)
    counts = np.stack([np.bincount(r[:, 0].astype(np.int64) * 4 + lv, minlength=B_IMG * 4) for (r, _, _), lv in zip(sets, lv_np)])
    assert counts.max() > GS_MAXL, counts.max()                       # a (set, image, level) list longer than GS_MAXL
    assert counts.reshape(4, B_IMG, 4)[:, EMPTY_IMG].sum() == 0       # an image without ROIs
    assert counts.reshape(4, B_IMG, 4)[3, :, 3].sum() == 0            # a level without ROIs of a set

    def run_route(fold):
        old = F.ROI_SUM_FOLD
        F.ROI_SUM_FOLD = fold
        try:
            feats = [f.detach().requires_grad_(True) for f in base]
            hs = [F.fan_out(f, 3) for f in feats]
            use = F.roi_grad_tap([h[2] for h in hs])
            outs = [F.roi_align(use, r, lv, p, SCALES, gsc) for r, lv, (_, p, gsc) in zip(rois, lvs, sets)]
            torch.autograd.backward(outs + [h[0] for h in hs] + [h[1] for h in hs], douts + w_sem + w_rpn)
            F.assert_no_deferred_gradients()
            return [o.detach() for o in outs], [f.grad for f in feats]
        finally:
            F.ROI_SUM_FOLD = old

    outs, g_fold = run_route(True)          # route 1: u2_roi_align_bwd_gather_sum with the two other readers as addends
    _, g_multi = run_route(False)           # route 2: u2_roi_align_bwd_gather_multi, then u2_add_n
    # route 4: the forward in processing order (ROI_ORDER_MIN = 0) is the same computation
    old = F.ROI_ORDER_MIN
    F.ROI_ORDER_MIN = 0
    try:
        for r, lv, (_, p, gsc), o in zip(rois, lvs, sets, outs):
            assert torch.equal(F.roi_align(base, r, lv, p, SCALES, gsc), o)
    finally:
        F.ROI_ORDER_MIN = old
    # route 3: the fp32-atomic scatter, one set at a time (a 7 x 7 stage at 1/3 and the 14 x 14 mask set)
    atomic_sets = (0, 3)
    g_atomic = {}
    F.ROI_ALIGN_BWD_ATOMIC = True
    try:
        for s in atomic_sets:
            fs = [f.detach().requires_grad_(True) for f in base]
            o = F.roi_align(fs, rois[s], lvs[s], sets[s][1], SCALES, sets[s][2])
            g_atomic[s] = torch.autograd.grad(o, fs, douts[s])
            del o, fs
    finally:
        F.ROI_ALIGN_BWD_ATOMIC = False

    cov = RoiCoverage()
    chk_f = [Check("roi%d fwd set %d" % (Hc, s), 5e-3) for s in range(4)]
    chk_1 = Check("roi%d bwd gather_sum" % Hc, 5e-3)
    chk_2 = Check("roi%d bwd gather_multi + add_n" % Hc, 8e-3)
    chk_3 = {s: Check("roi%d bwd atomic set %d" % (Hc, s), 5e-3) for s in atomic_sets}
    prange = [np.inf, -np.inf]
    chunk = 32
    for l, (_, Hl, Wl, C) in enumerate(shapes):
        for b in range(B_IMG):
            fb = base[l][b].to(F64)
            fa = fb.abs()
            G, S0, S1 = (torch.zeros((Hl, Wl, C), dtype=F64, device=DEV) for _ in range(3))
            NT = torch.zeros((Hl, Wl), dtype=F64, device=DEV)
            gmax = 0
            for s, (r_np, P, gsc) in enumerate(sets):
                sel = np.nonzero((r_np[:, 0] == b) & (lv_np[s] == l))[0]
                Gs, S0s, S1s = (torch.zeros((Hl, Wl, C), dtype=F64, device=DEV) for _ in range(3))
                NSs = torch.zeros((Hl, Wl), dtype=F64, device=DEV)
                cover = torch.zeros((-(-Hl // 8), -(-Wl // 8)), dtype=F64, device=DEV)
                for c0 in range(0, len(sel), chunk):
                    ids = sel[c0: c0 + chunk]
                    T = RoiTables(r_np[ids], SCALES[l], P, Hl, Wl)
                    (ylo, yhi), (xlo, xhi) = T.prange
                    prange = [min(prange[0], ylo, xlo), max(prange[1], yhi - Hl, xhi - Wl)]
                    gmax = max(gmax, T.gmax)
                    cov.add(T, Hl, Wl, cover)
                    it = torch.from_numpy(ids).to(DEV)
                    v, e = roi_fwd_ref(T, fb, fa)
                    chk_f[s].add(outs[s][it], v, e)
                    d = douts[s][it].to(F64) * (gsc / T.cnt)[:, None, None, None]
                    v, s0, s1, nterm, nsamp = roi_bwd_ref(T, d, Hl, Wl)
                    Gs += v; S0s += s0; S1s += s1; NT += nterm; NSs += nsamp
                    del T, v, e, d, s0, s1
                cov.done_list(cover)
                G += Gs; S0 += S0s; S1 += S1s
                if s in atomic_sets:
                    # per term: (d gscale) / cnt, hy hx, w g: 6 roundings; then one atomic per sample reaching the pixel
                    e3 = (S1s - S0s) + (NSs[..., None] + 8) * U * S1s
                    chk_3[s].add(g_atomic[s][l][b], Gs, 2 * e3)
                del Gs, S0s, S1s, NSs
            a0, a1 = w_sem[l][b].to(F64), w_rpn[l][b].to(F64)
            # the gather: per term tabY / tabX sums of g weights, ic = gscale / cnt, ayc, ayc * ax (gh + gw + 5 roundings); one
            # FMA per (ROI, bin) term reaching the pixel; the addends: two more additions
            per_term = (2 * gmax + 6) * U
            eg = (S1 - S0) + (NT[..., None] * U + per_term) * S1
            v1 = G + a0 + a1
            chk_1.add(g_fold[l][b], v1, 2 * (eg + (NT[..., None] + 3) * U * (a0.abs() + a1.abs())))
            # unfolded: the gather's map rounded to bf16, then u2_add_n's fp32 sum of three bf16 maps, rounded again
            m = G.abs() + 2 * eg + a0.abs() + a1.abs()
            lo = rnd(rnd(G - 2 * eg) + a0 + a1 - 2 * U * m)
            hi = rnd(rnd(G + 2 * eg) + a0 + a1 + 2 * U * m)
            chk_2.add_interval(g_multi[l][b], lo, hi, v1)
            del G, S0, S1, NT, fb, fa, a0, a1, eg, v1, lo, hi, m
    for c in chk_f + [chk_1, chk_2] + list(chk_3.values()):
        c.done()
    # empty boxes: zero outputs (the Check above holds them to exactly 0 as well)
    for (r_np, _, _), o in zip(sets, outs):
        empty = torch.from_numpy(np.nonzero((r_np[:, 3] <= r_np[:, 1]) | (r_np[:, 4] <= r_np[:, 2]))[0]).to(DEV)
        assert len(empty) > 0 and float(o[empty].abs().max()) == 0.0
    # the sample positions stay inside [-0.5, n - 0.5] (boxes clipped to images inside the canvas): the skip rule of the kernels
    # and of the reference can never disagree by a rounding
    assert prange[0] >= -0.75 and prange[1] <= -0.25, prange
    # the gather's paths are reached: single ROIs whose bins on one tile overflow the 48-bin stage, a tile under > 40 ROIs
    assert cov.big_single >= 20, cov.big_single
    assert cov.max_tile > 40, cov.max_tile
    print("roi%d: peak device memory %.2f GB; worst ratio to the bound: %s" % (
        Hc, torch.cuda.max_memory_allocated() / 2 ** 30,
        ", ".join("%s %.3g" % (c.name, c.worst) for c in chk_f + [chk_1, chk_2] + list(chk_3.values()))))


# =================================================================================================
# 3: the losses at their training shapes
def test_softmax_ce_full_size(F):
    """R = 8192 rows (the grid is capped at 512 work-groups: each wave walks 4 rows), 801 classes in 832-wide rows (pads hold
    garbage the kernel must ignore), 75 % background; saturated rows (|z| up to 60), uniform rows, ties."""
    R, NC, LP = 8192, 801, 832
    g = torch.Generator(device=DEV).manual_seed(21)
    z = torch.randn((R, LP), generator=g, device=DEV) * 3
    z[:, NC:] = 1e4
    z[0:64, :NC] = (torch.randn((64, NC), generator=g, device=DEV) * 25).clamp(-60, 60)    # saturated
    z[64:96, :NC] = -60.0
    z[64:96, 5] = 60.0                                                                      # p -> 1 (cancellation)
    z[96:128, :NC] = 1.5                                                                    # uniform
    z[128:256, :NC] = z[128:256, :NC].round()                                              # ties
    z[128:256, 7] = z[128:256, :NC].amax(1)
    z = z.to(BF16)
    lab = torch.full((R,), 800, dtype=torch.int64, device=DEV)
    fgr = torch.rand(R, generator=g, device=DEV) < 0.25
    lab[fgr] = torch.randint(0, 800, (int(fgr.sum()),), generator=g, device=DEV)
    lab[64:80] = 5
    zd = z.detach().requires_grad_(True)
    loss = F.softmax_cross_entropy(zd, lab, NC)
    loss.backward()
    zz = z[:, :NC].to(F64)
    mx = zz.amax(1, keepdim=True)
    lse = torch.logsumexp(zz, 1, keepdim=True)
    p = torch.exp(zz - lse)
    oh = TF.one_hot(lab, NC).to(F64)
    de = exp_rel(zz - mx)
    d_se = de.amax(1, keepdim=True) + 22 * U        # 16 terms per lane + the wave's 6 levels
    d_p = de + d_se + 2 * U
    gs = 1.0 / R
    ref = (p - oh) * gs
    e = gs * (d_p * p + U * (p - oh).abs() + TINY)
    chk = Check("softmax_ce: dlogits", 4e-3)
    chk.add(zd.grad[:, :NC], ref, 2 * e)
    chk.done()
    assert float(zd.grad[:, NC:].abs().max()) == 0.0
    # loss: per row mx + __logf(se) - z_t; 4 rows per wave, 2048 wave atomics
    zt = zz.gather(1, lab[:, None])
    Lr = lse - zt
    ln_se = (lse - mx).abs()
    e_row = d_se + 4 * U * ln_se + TINY + 2 * U * (mx.abs() + ln_se + zt.abs())
    bound = (float(e_row.sum()) + (4 + 2048 + 2) * U * float(Lr.abs().sum())) / R
    ref_l = float(Lr.sum()) / R
    assert abs(float(loss.detach()) - ref_l) <= 2 * bound, (float(loss.detach()), ref_l, bound)
    print("softmax_ce: worst ratio %.3g, loss error %.3g of bound %.3g" % (chk.worst, abs(float(loss.detach()) - ref_l), 2 * bound))


def get_deltas64(src, tgt, w):
    """Box2BoxTransform.get_deltas in float64 on the fp32 boxes, and the bound of losses.hip's fp32 get_deltas against it:
    widths, centres and their difference one rounding each (the difference cancels: its bound is absolute), the weight and the
    division one more each; log of a ratio of two rounded widths (3 u) plus logf's error."""
    s, t = src.to(F64), tgt.to(F64)
    sw, sh = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
    scx, scy = s[:, 0] + 0.5 * sw, s[:, 1] + 0.5 * sh
    tw, th = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1]
    tcx, tcy = t[:, 0] + 0.5 * tw, t[:, 1] + 0.5 * th
    wx, wy, ww, wh = w
    lw, lh = torch.log(tw / sw), torch.log(th / sh)
    d = torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * lw, wh * lh), 1)
    ex = abs(wx) / sw * U * (scx.abs() + sw + tcx.abs() + tw + 5 * (tcx - scx).abs())
    ey = abs(wy) / sh * U * (scy.abs() + sh + tcy.abs() + th + 5 * (tcy - scy).abs())
    e = torch.stack((ex, ey, abs(ww) * (4 * U + 5 * U * lw.abs()), abs(wh) * (4 * U + 5 * U * lh.abs())), 1)
    return d, 2 * e + TINY


def check_l1_grad(name, got, pred, d, e, gs, exact_zero=None):
    """sign(pred - d) * gs, exact, except where |pred - d| lies within the fp32 error of get_deltas (either sign, or 0)."""
    got = got.to(F64)
    df = pred.to(F64) - d
    sure = df.abs() > e
    want = torch.sign(df) * gs
    assert bool((got[sure] == want[sure]).all()), "%s: a gradient of the wrong sign" % name
    amb = ~sure
    assert bool(((got[amb] == gs) | (got[amb] == -gs) | (got[amb] == 0)).all()), name
    if exact_zero is not None:
        assert bool((got[exact_zero] == 0).all()), name
    return int(amb.sum())


@pytest.mark.parametrize("stage,weights", [(0, (10.0, 10.0, 5.0, 5.0)), (1, (20.0, 20.0, 10.0, 10.0)), (2, (30.0, 30.0, 15.0, 15.0))])
def test_box_reg_l1_full_size(F, stage, weights):
    """8192 rows, 25 % foreground, the cascade stage's weights; rows whose prediction is the bf16 rounding of the target (the
    sign rests on the fp32 target) and rows with proposal = gt and prediction 0 (exactly 0: no gradient)."""
    R, LP = 8192, 32
    g = torch.Generator(device=DEV).manual_seed(31 + stage)
    xy = torch.rand((R, 2), generator=g, device=DEV) * torch.tensor([1300.0, 780.0], device=DEV)
    wh = 2 + torch.rand((R, 2), generator=g, device=DEV) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((R, 4), generator=g, device=DEV) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    gt[:64] = prop[:64]
    lab = torch.where(torch.rand(R, generator=g, device=DEV) < 0.25,
                      torch.randint(0, 800, (R,), generator=g, device=DEV), torch.full((R,), 800, device=DEV))
    lab[:128] = 3
    d64, e = get_deltas64(prop, gt, weights)
    pred = torch.randn((R, LP), generator=g, device=DEV).to(BF16)
    pred[:64, :4] = 0
    pred[64:128, :4] = d64[64:128].to(BF16)
    pd = pred.detach().requires_grad_(True)
    loss = F.box_reg_l1_loss(pd, prop, gt, lab, 800, weights, R)
    loss.backward()
    fg = (lab < 800)
    gs = 1.0 / R
    gr = pd.grad.to(F64)
    assert float(gr[~fg].abs().max()) == 0.0 and float(gr[:, 4:].abs().max()) == 0.0
    zero_rows = torch.zeros_like(fg)
    zero_rows[:64] = True
    amb = check_l1_grad("box_reg stage %d" % stage, gr[fg][:, :4], pred[fg][:, :4], d64[fg], e[fg], gs,
                        exact_zero=zero_rows[fg][:, None].expand(-1, 4))
    assert amb < 64 * 4 + 16   # near-ties: the exact-zero rows and a handful of others
    # loss: per thread <= 4 terms, block sums over 256 lanes, 32 work-group atomics; the terms carry get_deltas' error
    df = (pred[fg][:, :4].to(F64) - d64[fg]).abs()
    ref = float(df.sum()) / R
    bound = (float(e[fg].sum()) + (4 + 8 + 32 + 2) * U * float(df.sum())) / R + U * ref
    assert abs(float(loss.detach()) - ref) <= 2 * bound, (float(loss.detach()), ref, bound)


@pytest.mark.parametrize("phased", [False, True], ids=["plain", "phased"])
def test_mask_predict_bce_full_size(F, H, phased):
    """N = 2048 ROIs x 784 positions x 256 channels, 800 classes, half the ROIs in one class (8192 work-groups' dW / db
    atomics on one row); |z| > 20, all-0 and all-1 targets.  The logit through logit_out (C ABI): inside the interval of the
    fp32 dot product's bound, i.e. one bf16 step, a second only where the float64 value straddles a rounding midpoint.  The loss
    and the gradients are checked at the kernel's own bf16 logit."""
    N, S, C, K = 2048, 28, 256, 800
    P = S * S
    g = torch.Generator(device=DEV).manual_seed(41)
    x = torch.randn((N, S, S, C), generator=g, device=DEV, dtype=BF16)
    x[::4] *= 8                                                # |z| > 20 on these ROIs
    w = torch.randn((K, C), generator=g, device=DEV) * 0.05
    bias = torch.randn(K, generator=g, device=DEV) * 0.1
    bias[100:110] = 22.0
    bias[110:120] = -22.0
    cls = torch.randint(0, K, (N,), generator=g, device=DEV)
    cls[: N // 2] = 7
    cls[N // 2: N // 2 + 64] = torch.arange(100, 164, device=DEV) % 20 + 100
    tgt = (torch.rand((N, S, S), generator=g, device=DEV) < 0.5).to(torch.uint8)
    tgt[3::16] = 0
    tgt[5::16] = 1
    xin = x.view(N, S // 2, 2, S // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, S // 2, S // 2, 4 * C).contiguous() if phased else x
    wq, bq = w.to(BF16).to(F64), bias.to(BF16).to(F64)
    denom = float(N * P)
    # the kernel's logit, in pixel order
    zk = torch.empty((N, P), dtype=BF16, device=DEV)
    lsum = torch.zeros(1, dtype=torch.float32, device=DEV)
    H.call("u2_mask_predict_bce", xin, w.contiguous(), bias.contiguous(), cls, tgt, None, None, None, lsum, zk, N, P, C,
           1.0 / denom, S if phased else 0, None)
    chk_z = Check("mask_bce%s: logit" % ("_phased" if phased else ""), None)
    xv = x.view(N, P, C)
    for n0 in range(0, N, 128):
        sl = slice(n0, n0 + 128)
        xc = xv[sl].to(F64)
        wc = wq[cls[sl]][:, None, :]
        v = (xc * wc).sum(2) + bq[cls[sl]][:, None]
        e = 2 * (12 * U * (xc * wc).abs().sum(2) + U * v.abs())
        chk_z.add_interval(zk[sl], rnd(v - e), rnd(v + e), v)
        del xc, wc, v, e
    chk_z.done()
    # the production wrapper: loss in forward, dx / dW / db in backward
    xd = xin.detach().requires_grad_(True)
    wd = torch.nn.Parameter(w.clone().view(K, C, 1, 1))
    bd = torch.nn.Parameter(bias.clone())
    loss = F.mask_predict_bce_loss(xd, wd, bd, cls, tgt, phased)
    loss.backward()
    dx = xd.grad
    if phased:
        dx = dx.view(N, S // 2, S // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, S, S, C)
    dx = dx.reshape(N, P, C)
    z = zk.to(F64)
    t = tgt.view(N, P).to(F64)
    sg = torch.sigmoid(z)
    g64 = (sg - t) / denom
    # sg = 1 / (1 + __expf(-z)): sigma (1 - sigma) exp_rel(|z|) + 2 u sigma; (sg - t): u; * fl(1 / denom): 2 u
    e_g = (sg * (1 - sg) * exp_rel(z) + 2 * U * sg) / denom + 3 * U * g64.abs() + 2.0 ** -140
    chk_x = Check("mask_bce%s: dx" % ("_phased" if phased else ""), 5e-3)
    for n0 in range(0, N, 128):
        sl = slice(n0, n0 + 128)
        wc = wq[cls[sl]][:, None, :]
        chk_x.add(dx[sl], g64[sl, :, None] * wc, 2 * (e_g[sl, :, None] * wc.abs() + U * (g64[sl, :, None] * wc).abs()))
    chk_x.done()
    # dW / db: per lane <= 25 positions, 4 waves, then one atomic per work-group (8 per ROI) on the class's row
    Y = torch.zeros((N, C), dtype=F64, device=DEV)
    A = torch.zeros_like(Y)
    Eg = torch.zeros_like(Y)
    for n0 in range(0, N, 128):
        sl = slice(n0, n0 + 128)
        xc = xv[sl].to(F64)
        Y[sl] = torch.einsum("np,npc->nc", g64[sl], xc)
        A[sl] = torch.einsum("np,npc->nc", g64[sl].abs(), xc.abs())
        Eg[sl] = torch.einsum("np,npc->nc", e_g[sl], xc.abs())
        del xc
    nk = torch.bincount(cls, minlength=K).to(F64)
    dw_ref = torch.zeros((K, C), dtype=F64, device=DEV).index_add_(0, cls, Y)
    dw_abs = torch.zeros_like(dw_ref).index_add_(0, cls, A)
    dw_eg = torch.zeros_like(dw_ref).index_add_(0, cls, Eg)
    depth = (25 + 3 + 8 * nk + 2)[:, None]
    check_vec("mask_bce: dW", wd.grad.view(K, C), dw_ref, 2 * (depth * U * dw_abs + dw_eg), 6e-3)
    db_ref = torch.zeros(K, dtype=F64, device=DEV).index_add_(0, cls, g64.sum(1))
    db_abs = torch.zeros(K, dtype=F64, device=DEV).index_add_(0, cls, g64.abs().sum(1))
    db_eg = torch.zeros(K, dtype=F64, device=DEV).index_add_(0, cls, e_g.sum(1))
    check_vec("mask_bce: db", bd.grad, db_ref, 2 * ((25 + 3 + 8 * nk + 2) * U * db_abs + db_eg), 6e-3)
    # loss: max(z, 0) - z t + log1pf(__expf(-|z|)) per position; 25 per lane, 4 waves, 16 384 work-group atomics
    y = torch.exp(-z.abs())
    lp = torch.log1p(y)
    li = z.clamp_min(0) - z * t + lp
    e_l = exp_rel(z) * y / (1 + y) + 4 * U * lp + TINY + 2 * U * (li.abs() + lp)
    ref = float(li.sum()) / denom
    bound = (float(e_l.sum()) + (25 + 3 + N * 8 + 2) * U * float(li.abs().sum())) / denom + U * ref
    assert abs(float(loss.detach()) - ref) <= 2 * bound, (float(loss.detach()), ref, bound)
    assert float(z.abs().max()) > 20
    print("mask_bce%s: worst ratios logit %.3g dx %.3g" % ("_phased" if phased else "", chk_z.worst, chk_x.worst))


RPN_STRIDES = (4, 8, 16, 32, 64)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
def test_rpn_loss_full_size(F, fused):
    """B = 16, five levels of the 800 x 1344 canvas, A = 3, 256 sampled anchors per image (0 ... 128 positives), up to 40 gt
    boxes, normaliser 256 * 16.  p2 has B * HW = 1 075 200 rows: the 2048 work-groups loop three times."""
    from oracle import ops as O

    B, A = 16, 3
    grids = [(-(-800 // s), -(-1344 // s)) for s in RPN_STRIDES]
    cells = [O.generate_cell_anchors([s * 8], (0.5, 1.0, 2.0)).float() for s in RPN_STRIDES]
    anchors = [a.to(DEV) for a in O.grid_anchors(grids, list(RPN_STRIDES), cells, 0.0)]
    acat = torch.cat(anchors)
    atot = acat.shape[0]
    g = torch.Generator(device=DEV).manual_seed(51)
    rng = np.random.default_rng(52)
    labels = torch.full((B, atot), -1, dtype=torch.int8, device=DEV)
    match = torch.zeros((B, atot), dtype=torch.int32, device=DEV)
    G = 40
    gt = torch.zeros((B, G, 4), dtype=torch.float32, device=DEV)
    for b in range(B):
        npos = [0, 128][b] if b < 2 else int(rng.integers(1, 65))
        pick = torch.from_numpy(rng.choice(atot, 256, replace=False)).to(DEV)
        labels[b, pick] = 0
        pos = pick[:npos]
        labels[b, pos] = 1
        ng = int(rng.integers(1, G + 1))
        src = acat[pos[:ng]] if npos else acat[pick[:ng]]
        src = torch.cat([src, acat[pick[: max(0, ng - len(src))]]])
        sz = (src[:, 2:] - src[:, :2]).repeat(1, 2)
        gt[b, :ng] = src + torch.randn(src.shape, generator=g, device=DEV) * 0.15 * sz
        gt[b, :ng, 2:] = torch.maximum(gt[b, :ng, 2:], gt[b, :ng, :2] + 1)
        match[b, pos] = torch.arange(npos, device=DEV, dtype=torch.int32) % ng
    maps = []
    for h, w in grids:
        m = torch.randn((B, h, w, 32), generator=g, device=DEV)
        m[..., :A] *= torch.where(torch.rand((B, h, w, 1), generator=g, device=DEV) < 0.05, 12.0, 2.0)
        maps.append(m.to(BF16))
    if fused:
        objs = [m.detach().requires_grad_(True) for m in maps]
        for o in objs:
            o._u2_rpn_fused = True
        dlts = [o[..., A: 5 * A] for o in objs]
        lc, ll = F.rpn_losses(labels, match, gt, anchors, A, 256.0 * B, objs, dlts)
    else:
        objs = [m[..., :8].contiguous().requires_grad_(True) for m in maps]
        dl = [torch.cat([m[..., A: 5 * A], torch.zeros_like(m[..., :4])], 3).contiguous().requires_grad_(True) for m in maps]
        lc, ll = F.rpn_losses(labels, match, gt, anchors, A, 256.0 * B, objs, dl)
    (lc + ll).backward()
    gs = 1.0 / (256 * B)
    chk = Check("rpn%s: dobj" % ("_fused" if fused else ""), 5e-3)
    off = 0
    l_ref = t_ref = 0.0
    e_lc = e_ll = a_lc = a_ll = 0.0
    amb = 0
    gridsz = 0
    for lvl, (h, w) in enumerate(grids):
        hw = h * w
        gridsz += min(2048, -(-B * hw // 256))
        lab = labels[:, off: off + hw * A].to(torch.int64).view(B, hw, A)
        mt = match[:, off: off + hw * A].to(torch.int64).view(B, hw, A)
        z = maps[lvl][..., :A].to(F64).view(B, hw, A)
        valid = lab >= 0
        t = lab.clamp_min(0).to(F64)
        sg = torch.sigmoid(z)
        ref = torch.where(valid, (sg - t) * gs, torch.zeros_like(z))
        e = torch.where(valid, gs * (sg * (1 - sg) * exp_rel(z) + 2 * U * sg + U * (sg - t).abs()) + 2.0 ** -140, torch.zeros_like(z))
        go = objs[lvl].grad.view(B, hw, -1)
        chk.add(go[..., :A], ref, 2 * e)
        y = torch.exp(-z.abs())
        lp = torch.log1p(y)
        li = torch.where(valid, z.clamp_min(0) - z * t + lp, torch.zeros_like(z))
        l_ref += float(li.sum())
        a_lc += float(li.abs().sum())
        e_lc += float(torch.where(valid, exp_rel(z) * y / (1 + y) + 4 * U * lp + TINY + 2 * U * (li.abs() + lp), torch.zeros_like(z)).sum())
        posm = lab == 1
        bi = torch.arange(B, device=DEV)[:, None, None].expand(B, hw, A)
        an = anchors[lvl].view(hw, A, 4)[None].expand(B, hw, A, 4)
        d64, ed = get_deltas64(an[posm], gt[bi[posm], mt[posm]], (1.0, 1.0, 1.0, 1.0))
        pr = maps[lvl][..., A: 5 * A].view(B, hw, A, 4)[posm]
        gd = (objs[lvl].grad.view(B, hw, -1)[..., A: 5 * A] if fused else dl[lvl].grad.view(B, hw, -1)[..., : 4 * A]).reshape(B, hw, A, 4)
        amb += check_l1_grad("rpn deltas", gd[posm], pr, d64, ed, gs)
        assert float(gd[~posm].abs().max()) == 0.0
        df = (pr.to(F64) - d64).abs()
        t_ref += float(df.sum())
        a_ll += float(df.sum())
        e_ll += float(ed.sum())
        # padding columns are zero
        if fused:
            assert float(go[..., 5 * A:].abs().max()) == 0.0
        else:
            assert float(go[..., A:].abs().max()) == 0.0 and float(dl[lvl].grad[..., 4 * A:].abs().max()) == 0.0
        off += hw * A
    assert off == atot
    chk.done()
    assert amb <= 4
    depth = 3 * 3 + 8 + gridsz + 2    # per thread <= 3 rows x 3 anchors, the block sum, every level's work-group atomics
    for got, ref, e, a, nm in ((lc, l_ref, e_lc, a_lc, "loss_rpn_cls"), (ll, t_ref, e_ll, a_ll, "loss_rpn_loc")):
        r = ref * gs
        bound = (e + depth * U * a) * gs + U * abs(r)
        assert abs(float(got.detach()) - r) <= 2 * bound, (nm, float(got.detach()), r, bound)


def semseg_case(name):
    """(canvas height, ragged image sizes, 255 blobs, one whole image ignored)"""
    return {"ragged800": (800, True, 24, True), "dense800": (800, False, 3, False), "ragged1024": (1024, True, 24, True)}[name]


@pytest.mark.parametrize("case", ["ragged800", "dense800", "ragged1024"])
def test_sem_seg_loss_full_size(F, case):
    """Logits 16 x h x 336 x 32 (28 classes) at stride 4, targets 16 x 4h x 1344 with the canvas padding, 255 blobs and (ragged
    cases) one whole image ignored.  dense800 and ragged1024 have more than 2^24 valid pixels: the kernel counts them with fp32
    atomics of per-work-group counts, exact below 2^24 and off by at most 1 per atomic above it.  This test bounds that error
    (the worst order of the atomics: the smallest counts last) and carries it into the loss and dlogit bounds."""
    Hc, ragged, nblob, drop = semseg_case(case)
    B, NC, LP = 16, 28, 32
    h, w = Hc // 4, 1344 // 4
    g = torch.Generator(device=DEV).manual_seed(Hc + nblob)
    rng = np.random.default_rng(Hc + nblob)
    logits = torch.randn((B, h, w, LP), generator=g, device=DEV) * 2
    logits[..., NC:] = 7.0
    logits = logits.to(BF16)
    tgt = torch.randint(0, NC, (B, 4 * h, 4 * w), generator=g, device=DEV).to(torch.uint8)
    for b in range(B):
        if ragged and b:
            ih, iw = 4 * h - 8 * int(rng.integers(0, 12)), 4 * w - 8 * int(rng.integers(0, 20))
            tgt[b, ih:] = 255
            tgt[b, :, iw:] = 255
        for _ in range(nblob):
            y0, x0 = int(rng.integers(0, 4 * h - 40)), int(rng.integers(0, 4 * w - 60))
            tgt[b, y0: y0 + int(rng.integers(3, 40)), x0: x0 + int(rng.integers(3, 60))] = 255
    if drop:
        tgt[5] = 255
    n_valid = int((tgt != 255).sum())
    if case != "ragged800":
        assert n_valid > 2 ** 24, n_valid
    ld = logits.detach().requires_grad_(True)
    loss = F.sem_seg_loss(ld, tgt, NC, 255)
    acc, sc = loss.grad_fn.saved_tensors
    cnt_k = float(sc[1])
    loss.backward()
    # the count: per-work-group counts are exact integers (owner: the work-group of the pixel's upper-left tap, 15 x 7 taps)
    ys, xs = torch.arange(4 * h, device=DEV), torch.arange(4 * w, device=DEV)
    by = (torch.div(ys - 2, 4, rounding_mode="floor").clamp_min(0) // 7)
    bx = (torch.div(xs - 2, 4, rounding_mode="floor").clamp_min(0) // 15)
    nby, nbx = int(by.max()) + 1, int(bx.max()) + 1
    key = (torch.arange(B, device=DEV)[:, None, None] * nby + by[None, :, None]) * nbx + bx[None, None, :]
    wg = torch.bincount(key[tgt != 255], minlength=B * nby * nbx)
    wg = torch.sort(wg[wg > 0])[0].to(torch.int64)
    cnt_err = 0
    if n_valid > 2 ** 24:
        budget = n_valid - 2 ** 24 + int(wg.max())
        cnt_err = int((torch.cumsum(wg, 0) <= budget).sum()) + 1
    assert cnt_k == int(cnt_k) and abs(cnt_k - n_valid) <= cnt_err, (cnt_k, n_valid, cnt_err)
    n_wg = len(wg)
    chk = Check("semseg %s: dlogits" % case, 4e-3)
    lsum = esum = asum = 0.0
    for b in range(B):
        z = logits[b, :, :, :NC].permute(2, 0, 1)[None].to(F64).requires_grad_(True)
        up = TF.interpolate(z, scale_factor=4.0, mode="bilinear", align_corners=False)
        t = tgt[b].long()[None]
        valid = (t != 255)[:, None]
        ce = TF.cross_entropy(up, t, ignore_index=255, reduction="sum")
        (gref,) = torch.autograd.grad(ce, z)
        with torch.no_grad():
            zabs = TF.interpolate(z.abs(), scale_factor=4.0, mode="bilinear", align_corners=False)
            mx = up.amax(1, keepdim=True)
            lse = torch.logsumexp(up, 1, keepdim=True)
            p = torch.exp(up - lse)
            oh = TF.one_hot(t.clamp_max(NC - 1), NC).permute(0, 3, 1, 2).to(F64)
            de = exp_rel(up - mx)
            dz = 4 * U * zabs.amax(1, keepdim=True)          # the kernel's interpolated logits (fp32, ATen's association)
            d_p = de + de.amax(1, keepdim=True) + 12 * U + 2 * dz
            epix = torch.where(valid, d_p * p + 15 * U * (p - oh).abs() + TINY, torch.zeros_like(p))
        (eg,) = torch.autograd.grad(up, z, epix)             # the transposed interpolation of the per-pixel bounds
        with torch.no_grad():
            gk = ld.grad[b, :, :, :NC].to(F64)
            r = gref[0].permute(1, 2, 0)
            e = eg[0].permute(1, 2, 0)
            ref = r / n_valid
            chk.add(gk, ref, 2 * (e / n_valid + ref.abs() * (cnt_err / n_valid + 3 * U)))
            zt = up.gather(1, t.clamp_max(NC - 1)[:, None])
            ln = (lse - mx)
            li = torch.where(valid, lse - zt, torch.zeros_like(lse))
            lsum += float(li.sum())
            asum += float(torch.where(valid, mx.abs() + ln.abs() + zt.abs(), torch.zeros_like(lse)).sum())
            esum += float(torch.where(valid, 2 * dz + de.amax(1, keepdim=True) + 12 * U + 14 * U * ln.abs() + TINY,
                                      torch.zeros_like(lse)).sum())
        del z, up, gref, eg, p, oh, de, epix
    chk.done()
    assert float(ld.grad[..., NC:].abs().max()) == 0.0
    depth = 3 * 32 + 8 + n_wg + 2
    ref_l = lsum / n_valid
    bound = (esum + depth * U * asum) / n_valid + ref_l * (cnt_err / n_valid + 2 * U)
    assert abs(float(loss.detach()) - ref_l) <= 2 * bound, (float(loss.detach()), ref_l, bound)
    print("semseg %s: %d valid pixels, count %d (bound %d), worst ratio %.3g" % (case, n_valid, int(cnt_k), cnt_err, chk.worst))
