"""The box decision kernels of u2seg_amd/csrc/roi.hip - IoU matching (iou_match_kernel, match_label_kernel), batched NMS
(nms_mask_kernel, nms_scan_kernel), FPN level assignment, delta decoding (apply_deltas_kernel and its copy in rpn_decode_kernel)
and the ground-truth mask crops (mask_crop_kernel, mask_crop_batch_kernel) - at their decision edges against float64.  These
kernels turn boxes into integers (which ground truth, kept or not, which level, which target pixels); random boxes almost never
land where they decide, so the inputs here are built to.

References: tests/float64_refs.py (iou_ref, match_ref, nms_ref, levels_ref, apply_deltas_ref, mask_crop_ref - plain torch in
float64 on the CPU, written from the reference's formulas and held against the oracle's restatements by
tests/test_float64_refs_host.py).  Two kinds of check, as in tests/test_gpu_inference_tails_float64.py:

A. exact inputs, bit for bit, nothing excused.  Integer box corners below 2^11 (every area, intersection and union an fp32 number,
   the IoU the one correctly rounded quotient: iou_ref's docstring) or dyadic ROI corners on binary masks (every sample position,
   weight and bin sum an fp32 number: mask_crop_exact_case's docstring).  Match index, label, matched value, kept positions, level
   and target pixel must equal the reference everywhere.  Decisions that sit exactly on their threshold and ties are built in.

B. random fp32 inputs, measured margin: 4 x the largest deviation of the REFERENCE's own fp32 form (the oracle on the CPU) from
   float64 on the very inputs of the test - the factor pays for the kernel's different, equally valid operation order and another
   expf - never a figure taken from the kernel.  Values seen when this was written stand next to each assert."""
import ctypes

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16


class Env:
    pass


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from oracle import ops
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()
    e = Env()
    e.hip, e.F, e.O = _hip, functional, ops
    return e


def report(name, what, value):
    print("BOX64 %s | %s | %.4g" % (name, what, value))


def first_diff(name, got, want):
    """Every element equal; the message names the first that is not."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            name, int(bad.sum()), bad.numel(), i, got[i].item(), want[i].item()))


# ----------------------------------------------------------------------------------------------------------------------------
# IoU matching (kind A throughout)
# ----------------------------------------------------------------------------------------------------------------------------
def check_match(E, name, cand, gts, g_pad, lo, hi, allow):
    """F.iou_match on candidates [n, 4] (shared) or [B, n, 4] and the per-image ground truths `gts` (list of [g_i, 4]), padded to
    g_pad rows with a box that overlaps everything (it must never be read): match, labels and matched value equal match_ref at
    every element.  Returns the labels [B, n] (CPU)."""
    b = len(gts)
    gt = torch.tensor(R.BOX_BIG).repeat(b, g_pad, 1)
    for i, gi in enumerate(gts):
        gt[i, : gi.shape[0]] = gi
    ngt = torch.tensor([gi.shape[0] for gi in gts], dtype=torch.int32)
    match, labels, mval = E.F.iou_match(cand.to(DEV), gt.to(DEV), ngt.to(DEV), lo, hi, allow)
    assert match.dtype == torch.int32 and labels.dtype == torch.int8 and mval.dtype == torch.float32
    for i, gi in enumerate(gts):
        ci = cand[i] if cand.dim() == 3 else cand
        rm, rl, rv = R.match_ref(gi, ci, lo, hi, allow)
        tag = "%s image %d (ngt %d of %d) thr (%g, %g) low-quality %d" % (name, i, gi.shape[0], g_pad, lo, hi, allow)
        first_diff(tag + " match", match[i].long(), rm)
        first_diff(tag + " value", mval[i], rv)
        first_diff(tag + " label", labels[i], rl)
    return labels.cpu()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_match_sizes_layouts_and_padding(E, n):
    """n at and around the 256-candidate work-group, G in {1, 4, 37}, a batch of three images with ngt = G, 0 and about G / 2 (the
    padding rows hold a box that would match everything), shared [n, 4] and per-image [B, n, 4] candidates, thresholds (0.3, 0.7)
    and (0.5, 0.5), with and without low-quality matches.  Integer boxes: many candidates tie between ground truths, and one ground
    truth is repeated (the first index must win)."""
    g = torch.Generator().manual_seed(100 + n)
    seen = set()
    for g_pad in (1, 4, 37):
        full = R.int_boxes(g_pad, g)
        if g_pad > 1:
            full[g_pad - 1] = full[0]
        gts = [full, full[:0], full[: max(g_pad // 2, 1)]]
        for cand in (R.int_boxes(n, g), torch.stack([R.int_boxes(n, g) for _ in range(3)])):
            for lo, hi in ((0.3, 0.7), (0.5, 0.5)):
                for allow in (False, True):
                    lab = check_match(E, "n %d G %d %s" % (n, g_pad, "per-image" if cand.dim() == 3 else "shared"), cand, gts,
                                      g_pad, lo, hi, allow)
                    seen |= set(lab.flatten().tolist())
                    assert not bool(lab[1].any())           # no ground truth: everything background
    if n >= 255:
        assert seen == {-1, 0, 1}


def test_match_grid_stride_loop(E):
    """n = 262 144 + 300 candidates, G = 3: the launch is capped at 1024 work-groups of 256, so this is the first n at which the
    grid-stride loop takes a second pass (the 800 x 1333 anchor set has 266 994).  Low-quality matches on: the per-ground-truth
    maximum is reduced over all work-groups and both passes."""
    g = torch.Generator().manual_seed(7)
    n = 262144 + 300
    cand = R.int_boxes(n, g, span=1500, side=300)
    gt = R.int_boxes(3, g, span=1200, side=500, min_side=100)
    cand[n - 7] = gt[2]                       # the best candidate of ground truth 2 sits in the second pass
    lab = check_match(E, "grid stride", cand, [gt], 3, 0.3, 0.7, True)
    assert int(lab[0, n - 7]) == 1 and set(lab.flatten().tolist()) == {-1, 0, 1}


def test_match_iou_exactly_on_a_threshold(E):
    """Candidates whose IoU with the ground truth is exactly 1/2, 3/10 and 7/10 (and 1, 0, 2/10 .. 8/10, touching): RN32(3/10) is
    float32(0.3), so `v < lo` is false and the candidate is ignored, not background; RN32(7/10) is float32(0.7): positive; at
    (0.5, 0.5) the 1/2 candidate is positive.  An approximate division or a threshold held in double moves one of them."""
    for lo, hi, want in ((0.3, 0.7, [-1, -1, 1, 1, 0, 0, -1, -1, 1, 0]), (0.5, 0.5, [1, 0, 1, 1, 0, 0, 0, 1, 1, 0])):
        lab = check_match(E, "edge", R.EDGE_CAND, [R.EDGE_GT], 1, lo, hi, False)
        assert lab[0].tolist() == want
        check_match(E, "edge", R.EDGE_CAND.repeat(30, 1), [R.EDGE_GT, R.EDGE_GT], 4, lo, hi, True)


def test_match_ties_and_low_quality_rules(E):
    """- two identical ground truths: the first index everywhere;
    - low-quality matches whose tying best candidates sit in three different work-groups (indices 5, 300 and 900 of 1000; IoU 1/5,
      below lo): the per-ground-truth maximum goes through the LDS atomicMax of three work-groups and the global one, and all three
      must be positive while a candidate with IoU 1/10 stays background;
    - a ground truth that overlaps no candidate: its maximum is 0 and, as in the reference, every candidate it does not overlap -
      all of them - turns positive."""
    g = torch.Generator().manual_seed(9)
    cand = R.int_boxes(1000, g) + 200                       # all inside [200, 360]
    gt = R.int_boxes(4, g) + 200
    gt[2] = gt[0]
    far = torch.tensor([[0.0, 0.0, 10.0, 10.0]])            # overlaps only the candidates planted below
    for i, k in ((5, 2.0), (300, 2.0), (900, 2.0), (600, 1.0)):
        cand[i] = torch.tensor([0.0, 0.0, 10.0, k])         # IoU 2/10 three times, 1/10 once
    gts = torch.cat([gt, far])
    lab = check_match(E, "ties", cand, [gts], 5, 0.3, 0.7, True)
    assert lab[0, [5, 300, 900]].tolist() == [1, 1, 1] and int(lab[0, 600]) == 0
    m = E.F.iou_match(cand.to(DEV), gts[None].to(DEV), torch.tensor([5], dtype=torch.int32, device=DEV), 0.3, 0.7, True)[0]
    assert not bool((m == 2).any()) and bool((m == 0).any()) and m[0, [5, 300, 900, 600]].tolist() == [4] * 4
    assert 0 < int((lab == 0).sum()) and 0 < int((lab == 1).sum()) < 500
    without = check_match(E, "ties, no low-quality", cand, [gts], 5, 0.3, 0.7, False)
    assert without[0, [5, 300, 900]].tolist() == [0, 0, 0]
    lonely = torch.cat([gt, torch.tensor([[1000.0, 1000.0, 1010.0, 1010.0]])])
    lab = check_match(E, "disjoint ground truth", cand, [lonely, gt], 5, 0.3, 0.7, True)
    assert bool((lab[0] == 1).all()) and not bool((lab[1] == 1).all())


def test_match_writes_its_b_n_elements_and_nothing_else(E):
    """Through the ABI with guarded outputs (B = 2, n = 257 and 1, G = 4): match, labels and mval are written for all B n
    elements - no sentinel left - and the 64 elements behind them keep their sentinel."""
    g = torch.Generator().manual_seed(11)
    for n in (257, 1):
        b, g_pad = 2, 4
        cand = torch.stack([R.int_boxes(n, g) for _ in range(b)])
        gts = [R.int_boxes(4, g), R.int_boxes(2, g)]
        gt = torch.tensor(R.BOX_BIG).repeat(b, g_pad, 1)
        gt[0], gt[1, :2] = gts[0], gts[1]
        match = torch.full((b * n + 64,), -77, dtype=torch.int32, device=DEV)
        mval = torch.full((b * n + 64,), -77.0, dtype=torch.float32, device=DEV)
        labels = torch.full((b * n + 64,), -77, dtype=torch.int8, device=DEV)
        gmax = torch.empty((b, g_pad), dtype=torch.int32, device=DEV)
        E.hip.call("u2_iou_match", cand.to(DEV), 1, gt.to(DEV), torch.tensor([4, 2], dtype=torch.int32, device=DEV), match, mval,
                   gmax, labels, b, n, g_pad, 0.3, 0.7, 1)
        torch.cuda.synchronize()
        for t in (match, mval, labels):
            assert bool((t[b * n:] == -77).all()) and not bool((t[: b * n] == -77).any()), n
        for i in range(b):
            rm, rl, rv = R.match_ref(gts[i], cand[i], 0.3, 0.7, True)
            first_diff("guarded match", match[i * n: (i + 1) * n].long(), rm)
            first_diff("guarded label", labels[i * n: (i + 1) * n], rl)
            first_diff("guarded value", mval[i * n: (i + 1) * n], rv)


# ----------------------------------------------------------------------------------------------------------------------------
# batched NMS (kind A throughout)
# ----------------------------------------------------------------------------------------------------------------------------
def check_nms(E, name, boxes, groups, cnt, thr, max_keep, poison=False):
    """F.batched_nms (or, with `poison`, the launcher itself on a workspace pre-filled with 0xFF bytes: the words of column blocks
    before the row's own and of rows beyond cnt are never written, and nothing may read them) on boxes [B, n, 4] in score order,
    groups [B, n], cnt [B]: kept positions and their number equal nms_ref per image, and oracle.ops.nms (the C restatement, given
    strictly descending scores).  Returns the kept lists."""
    b, n = boxes.shape[0], boxes.shape[1]
    bd, gd = boxes.to(DEV), groups.to(torch.int32).to(DEV)
    cd = torch.tensor(cnt, dtype=torch.int32, device=DEV)
    if poison:
        ws = torch.full((E.hip.call_nostream("u2_nms_workspace_bytes", b, n) + 8,), 0xFF, dtype=torch.uint8, device=DEV)
        keep = torch.full((b, max_keep), -5, dtype=torch.int32, device=DEV)
        nkeep = torch.full((b,), -5, dtype=torch.int32, device=DEV)
        E.hip.call("u2_batched_nms", bd, gd, cd, ws, keep, nkeep, b, n, float(thr), max_keep)
        fill = -5
    else:
        keep, nkeep = E.F.batched_nms(bd, gd, cd, thr, max_keep)
        fill = 0
    keep, nkeep = keep.cpu(), nkeep.cpu().tolist()
    out = []
    for i in range(b):
        c = cnt[i]
        want = R.nms_ref(boxes[i, :c], groups[i, :c], thr, max_keep)
        tag = "%s image %d (cnt %d of %d) thr %g max_keep %d" % (name, i, c, n, thr, max_keep)
        assert nkeep[i] == len(want), (tag, nkeep[i], len(want))
        assert keep[i, : nkeep[i]].tolist() == want, tag
        assert bool((keep[i, nkeep[i]:] == fill).all()), tag          # nothing written behind the kept list
        orc = E.O.nms(boxes[i, :c], torch.arange(c, 0, -1).float(), thr, groups[i, :c]).tolist()
        assert want == orc[:max_keep], tag
        out.append(want)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 300])
def test_nms_sizes_counts_and_thresholds(E, n):
    """n at and around the 64-box block, cnt = 0, n and a value inside a block, thresholds 0.5 / 0.65 / 0.7, three groups,
    max_keep = n and a value inside a block: heavily overlapping integer boxes, so chains of suppression run through every block."""
    g = torch.Generator().manual_seed(200 + n)
    kept = 0
    for thr in (0.5, 0.65, 0.7):
        boxes = R.int_boxes(n, g, span=32, min_side=40)[None]
        groups = torch.randint(0, 3, (1, n), generator=g)
        for cnt in sorted({0, n, max(n - 27, 1), (n + 1) // 2}):
            for max_keep in sorted({n, max(n // 3, 1)}):
                kept += len(check_nms(E, "n %d" % n, boxes, groups, [cnt], thr, max_keep)[0])
    assert kept >= 3


def test_nms_ragged_batch(E):
    """B = 3 with per-image counts 300, 0 and 100 of n = 300; the boxes behind an image's count would suppress (they repeat the
    first box) and must not be read."""
    g = torch.Generator().manual_seed(21)
    boxes = torch.stack([R.int_boxes(300, g, span=32, min_side=40) for _ in range(3)])
    boxes[2, 100:] = boxes[2, 0]
    groups = torch.randint(0, 2, (3, 300), generator=g)
    for poison in (False, True):
        out = check_nms(E, "ragged", boxes, groups, [300, 0, 100], 0.5, 300, poison)
        assert len(out[0]) > 5 and out[1] == [] and len(out[2]) > 3


def test_nms_constructions(E):
    """Hand-made cases, each once through the wrapper and once through the launcher on a 0xFF-filled workspace:
    - all boxes identical (n = 129): exactly one kept; the same boxes spread over three groups never interact: three kept;
    - all disjoint (n = 300), max_keep in {1, 64, 100, 256, 300}: positions 0 .. max_keep - 1 in order and nkeep exact, with more
      than 192 kept rows for 256 and 300; 100 ends the scan in the middle of a block;
    - nms_helper_stride_case (n = 400): a victim in block 6 of the 201st kept box, which a helper thread reaches only with its
      second stride of 192 (at n = 300 no helper takes one, whatever is kept);
    - a ladder in which every second box survives, across the 64- and 128-box edges, in both parities;
    - nms_lazy_column_case: a box at position 3 whose only victims sit at 130 .. 140 and 200, and a box at position 5 that is
      itself suppressed and must spare 150 .. 155;
    - pairs with IoU exactly 1/2 at 0.5, 7/10 at 0.7, 13/20 at 0.65: not suppressed; the pair one pixel tighter is;
    - boxes without area: 0 / 0 = NaN suppresses nothing."""
    zero = lambda n: torch.zeros((1, n), dtype=torch.int64)     # noqa: E731
    for poison in (False, True):
        same = torch.tensor([[5.0, 5.0, 25.0, 30.0]]).repeat(129, 1)[None]
        assert check_nms(E, "identical", same, zero(129), [129], 0.5, 129, poison) == [[0]]
        assert check_nms(E, "identical, 3 groups", same, (torch.arange(129) % 3)[None], [129], 0.5, 129, poison) == [[0, 1, 2]]
        grid = R._grid_boxes(300)[None]
        for max_keep in (1, 64, 100, 256, 300):
            assert check_nms(E, "disjoint", grid, zero(300), [300], 0.5, max_keep, poison) == [list(range(max_keep))]
        assert check_nms(E, "ladder", R.nms_ladder(300)[None], zero(300), [300], 0.5, 300, poison) == [list(range(0, 300, 2))]
        assert check_nms(E, "ladder, odd", R.nms_ladder(300, 1)[None], zero(300), [300], 0.5, 300, poison) == [[0] + list(range(1, 300, 2))]
        assert check_nms(E, "ladder, cut", R.nms_ladder(300)[None], zero(300), [300], 0.5, 70, poison) == [list(range(0, 140, 2))]
        lazy, dead = R.nms_lazy_column_case()
        assert check_nms(E, "lazy column", lazy[None], zero(300), [300], 0.5, 300, poison) == [[i for i in range(300) if i not in dead]]
        far, dead = R.nms_helper_stride_case()
        assert check_nms(E, "helper stride", far[None], zero(400), [400], 0.5, 400, poison) == [[i for i in range(400) if i not in dead]]
        for thr in (0.5, 0.7, 0.65):
            assert check_nms(E, "pairs", R.nms_threshold_pairs(thr)[None], zero(4), [4], thr, 4, poison) == [[0, 1, 2]]
        flat = torch.tensor([[10.0, 10.0, 10.0, 20.0]] * 3 + [[5.0, 5.0, 5.0, 5.0]] * 2 + [[8.0, 8.0, 12.0, 22.0]])[None]
        assert check_nms(E, "no area", flat, zero(6), [6], 0.5, 6, poison) == [list(range(6))]


# ----------------------------------------------------------------------------------------------------------------------------
# level assignment (kind A: the decision is compared, and every box is either exactly on a boundary or 2^-10 clear of it)
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(2, 5), (1, 6)])
def test_assign_levels_at_the_boundaries(E, lo, hi):
    """level_boundary_boxes: sqrt(area) exactly 28 .. 896, square and not (56 x 224), lands on the upper side of its boundary -
    levels_ref's docstring derives why s / 224 + 1e-8 rounds back to the power of two in fp32 -; each boundary scaled by
    1 +- 2^-10; boxes without area (level 0).  n = 1 (every box alone) and n = 257 (the boxes repeated past one work-group)."""
    b = R.level_boundary_boxes()
    want = R.levels_ref(b, lo, hi)
    assert int(want.min()) == 0 and int(want.max()) == hi - lo
    many = b.repeat(6, 1)[:257]
    got = E.F.assign_levels(many.to(DEV), lo, hi)
    assert got.dtype == torch.int32
    first_diff("levels n 257", got.long(), want.repeat(6)[:257])
    for i in range(b.shape[0]):
        first_diff("levels n 1, box %d %s" % (i, b[i].tolist()), E.F.assign_levels(b[i: i + 1].to(DEV), lo, hi).long(), want[i: i + 1])


# ----------------------------------------------------------------------------------------------------------------------------
# delta decode
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257])
def test_apply_deltas_exact_inputs_bit_for_bit(E, n):
    """Kind A.  Integer and half-integer source boxes, some sticking out of and some wholly outside the images; deltas
    (k wx, m wy, 0, 0) with k, m in -3 .. 3 (zero deltas among them) for the three cascade weight sets: dx = k exactly, exp(0) = 1,
    so the decoded box is the source moved by (k w, m h) bit for bit, and the clipped one lands on exactly 0 and W or H.  `img`
    selects among three image sizes; img = nullptr with the clip on reads image 0."""
    g = torch.Generator().manual_seed(300 + n)
    xy = torch.randint(-300, 700, (n, 2), generator=g).float() / 2
    src = torch.cat([xy, xy + torch.randint(1, 200, (n, 2), generator=g).float() / 2], dim=1)
    sizes = torch.tensor(R.DELTA_SIZES)
    img = torch.randint(0, 3, (n,), generator=g).to(torch.int32)
    for wt in R.CASCADE_WEIGHTS:
        km = torch.randint(-3, 4, (n, 2), generator=g).float()
        km[0] = 0
        d = torch.cat([km * torch.tensor(wt[:2]), torch.zeros((n, 2))], dim=1)
        raw, clipped = R.apply_deltas_ref(src, d, wt, R.SCALE_CLAMP, sizes, img)
        moved = src + torch.stack([km[:, 0] * (src[:, 2] - src[:, 0]), km[:, 1] * (src[:, 3] - src[:, 1])] * 2, dim=1)
        assert torch.equal(raw, moved.to(F64)) and torch.equal(raw[0], src[0].to(F64))
        got = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, None, None, R.SCALE_CLAMP)
        first_diff("unclipped", got.to(F64), raw)
        got = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, img.to(DEV), sizes.to(DEV), R.SCALE_CLAMP)
        first_diff("clipped, img", got.to(F64), clipped)
        _, clipped0 = R.apply_deltas_ref(src, d, wt, R.SCALE_CLAMP, sizes[:1])
        got = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, None, sizes.to(DEV), R.SCALE_CLAMP)
        first_diff("clipped, no img", got.to(F64), clipped0)
        if n > 1:
            lim = sizes[img.long()]
            assert bool((clipped[:, 0] == 0).any()) and bool((clipped[:, 2] == lim[:, 1]).any()) and bool((clipped[:, 3] == lim[:, 0]).any())
            assert bool(((clipped[:, 2] - clipped[:, 0]) == 0).any())       # a box wholly outside collapses onto the border


def test_apply_deltas_random_inputs_vs_float64(E):
    """Kind B.  delta_random_case: 2000 boxes per cascade weight set, size deltas far above the clamp (decoded sides up to 62.5 x the
    source's) and near -20.  |kernel - apply_deltas_ref| <= margin = 4 x max |oracle.apply_deltas (+ clip_boxes) in fp32 on the
    CPU - apply_deltas_ref| over the same inputs, separately for the unclipped boxes (coordinates up to ~ 2e4, an fp32 ulp of
    2e-3) and the clipped ones (at most 500)."""
    sizes = torch.tensor(R.DELTA_SIZES)
    for seed, wt in enumerate(R.CASCADE_WEIGHTS):
        src, d, img = R.delta_random_case(2000, 40 + seed, wt)
        raw, clipped = R.apply_deltas_ref(src, d, wt, R.SCALE_CLAMP, sizes, img)
        o_raw = E.O.apply_deltas(d, src, wt)
        o_clip = torch.empty_like(o_raw)
        for i in range(3):
            o_clip[img == i] = E.O.clip_boxes(o_raw[img == i], R.DELTA_SIZES[i])
        dev_raw, dev_clip = float((o_raw.to(F64) - raw).abs().max()), float((o_clip.to(F64) - clipped).abs().max())
        # measured on the CPU when written (weights 10/5, 20/10, 30/15): dev_raw 1.45e-3, 1.29e-3, 1.38e-3 -> margins 5.8e-3, 5.1e-3,
        # 5.5e-3; dev_clip 6.50e-5, 7.65e-5, 6.60e-5 -> margins 2.6e-4, 3.1e-4, 2.6e-4
        report("deltas w %g" % wt[0], "max |oracle fp32 - float64| unclipped", dev_raw)
        report("deltas w %g" % wt[0], "max |oracle fp32 - float64| clipped", dev_clip)
        assert 0 < dev_raw < 1e-2 and 0 < dev_clip < 2e-4 and float(raw.abs().max()) > 3000
        got_raw = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, None, None, R.SCALE_CLAMP).cpu().to(F64)
        got_clip = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, img.to(DEV), sizes.to(DEV), R.SCALE_CLAMP).cpu().to(F64)
        err_raw, err_clip = float((got_raw - raw).abs().max()), float((got_clip - clipped).abs().max())
        report("deltas w %g" % wt[0], "max |kernel - float64| / margin, unclipped", err_raw / (4 * dev_raw))
        report("deltas w %g" % wt[0], "max |kernel - float64| / margin, clipped", err_clip / (4 * dev_clip))
        # seen on an MI355X when written: 0.25 of the margin unclipped for all three sets (the kernel's worst element is the
        # oracle's, with the same fp32 value); clipped 0.25, 0.21, 0.25
        assert err_raw <= 4 * dev_raw and err_clip <= 4 * dev_clip


@pytest.mark.parametrize("channel", [0, 1, 2, 3], ids=["dx", "dy", "dw", "dh"])
def test_apply_deltas_keeps_a_nan_delta(E, channel):
    """A NaN in one delta channel: the unclipped output is NaN exactly where the reference's is (torch.clamp(max=) keeps NaN: both
    corners of that axis), for every cascade weight set; every other box is untouched by it."""
    src, d, _ = R.delta_random_case(257, 50, R.CASCADE_WEIGHTS[0])
    for wt in R.CASCADE_WEIGHTS:
        d2 = d.clone()
        d2[[0, 100, 256], channel] = float("nan")
        raw, _ = R.apply_deltas_ref(src, d2, wt, R.SCALE_CLAMP)
        o_raw = E.O.apply_deltas(d2, src, wt)
        assert torch.equal(torch.isnan(raw), torch.isnan(o_raw)) and int(torch.isnan(raw).sum()) == 6
        got = E.F.apply_deltas(src.to(DEV), d2.to(DEV), wt, None, None, R.SCALE_CLAMP).cpu()
        first_diff("NaN pattern, channel %d" % channel, torch.isnan(got), torch.isnan(raw))
        clean = E.F.apply_deltas(src.to(DEV), d.to(DEV), wt, None, None, R.SCALE_CLAMP).cpu()
        keep = ~torch.isnan(raw)
        assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("channel", [0, 1, 2, 3], ids=["dx", "dy", "dw", "dh"])
def test_rpn_decode_counts_a_nan_delta(E, channel):
    """F.rpn_decode on two levels (8 and 4 anchors, kmax = 8) with a NaN in one delta channel of one candidate: the reference's
    decode (oracle.apply_deltas) gives that candidate a non-finite box, so `nonfinite` counts exactly it and its keep flag is
    clear; every other real candidate is kept and its clipped box is the oracle's to fp32 error; the padding of the short level is
    not kept."""
    g = torch.Generator().manual_seed(60)
    weights, kmax, hw = (1.0, 1.0, 1.0, 1.0), 8, (64.0, 80.0)
    sizes = torch.tensor([list(hw)], device=DEV)
    levels, want_boxes, want_finite = [], [], []
    for li, (gh, gw) in enumerate(((2, 4), (1, 4))):
        k = gh * gw
        d = (torch.randn((1, gh, gw, 4), generator=g) * 0.2).to(BF16)
        if li == 0:
            d[0, 0, 2, channel] = float("nan")
        xy = torch.rand((k, 2), generator=g) * 30 + 5
        anc = torch.cat([xy, xy + 8 + torch.rand((k, 2), generator=g) * 8], dim=1)
        idx = torch.arange(k, dtype=torch.int32)[None]
        sc = torch.randn((1, k), generator=g)
        levels.append(dict(deltas=d.to(DEV), anchors=anc.to(DEV), idx=idx.to(DEV), scores=sc.to(DEV)))
        raw = E.O.apply_deltas(d.float().reshape(k, 4), anc, weights)
        want_finite.append(torch.isfinite(raw).all(dim=1))
        want_boxes.append(E.O.clip_boxes(raw, hw))
    assert want_finite[0].tolist() == [True, True, False] + [True] * 5 and bool(want_finite[1].all())
    boxes, scores, keep, nonfinite = E.F.rpn_decode(levels, 1, 1, kmax, sizes, weights, R.SCALE_CLAMP, 0.0)
    torch.cuda.synchronize()
    assert int(nonfinite.item()) == 1, "non-finite candidates counted: %d, the reference has 1" % int(nonfinite.item())
    assert keep.cpu().tolist() == [[1, 1, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0, 0]]
    for li in range(2):
        k = want_boxes[li].shape[0]
        ok = want_finite[li]
        assert float((boxes[li, :k].cpu() - want_boxes[li])[ok].abs().max()) < 1e-4
        assert torch.equal(scores[li, :k].cpu(), levels[li]["scores"][0].cpu())


# ----------------------------------------------------------------------------------------------------------------------------
# mask crops
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 7, 28])
def test_mask_crop_exact_inputs_bit_for_bit(E, p):
    """Kind A.  F.mask_crop on mask_crop_exact_case: binary masks, ROIs of side p, 2 p, 3 p and 1.5 p (and 2 p x 3 p) with dyadic
    corners - every bin sum is an fp32 number (asserted) -, bin averages of exactly 1/4, 2/4, 3/4, 4/9 and 5/9 among them (2/4
    gives 1, 4/9 gives 0, 5/9 gives 1), ROIs hanging over each border, wholly outside, without extent, mask index > 0: every
    target pixel equals mask_crop_ref >= 0.5."""
    masks, rois = R.mask_crop_exact_case(p)
    avg = R.mask_crop_ref(masks, rois, p)
    assert torch.equal(avg * 36 * 64, torch.round(avg * 36 * 64)), "precondition: the bin sums are multiples of 1/64"
    seen = set(avg.flatten().tolist())
    assert all(v in seen for v in (0.25, 0.5, 0.75, 4.0 / 9, 5.0 / 9)) and int(rois[:, 0].max()) > 0
    got = E.F.mask_crop(masks.to(DEV), rois.to(DEV), p)
    assert got.dtype == torch.uint8 and got.shape == avg.shape
    first_diff("mask crop P %d" % p, got, (avg >= 0.5).to(torch.uint8))
    assert not bool(got[-5:].any()) and bool(got[-10:-5].any())     # outside / empty ROIs: all 0; the overhanging ones are not


def test_mask_crop_batch_two_chunks_vs_float64_and_the_single_crop(E):
    """u2_mask_crop_batch on 35 images of two sizes (32 per launch: the second chunk holds images 32 .. 34), ROIs in images 0, 5, 31,
    32 and 34, thirty images without any; `out` pre-filled with 7: every byte is written - no 7 left -, equals mask_crop_ref of its
    image's bitmaps and equals the single-tensor crop of the same ROI.  R = 0 returns 0 and writes nothing."""
    p = 7
    masks, rois, img = R.mask_crop_batch_case(p)
    md = [m.to(DEV) for m in masks]
    n = len(md)
    ptrs = (ctypes.c_void_p * n)(*[m.data_ptr() for m in md])
    hs = (ctypes.c_int * n)(*[m.shape[1] for m in md])
    ws = (ctypes.c_int * n)(*[m.shape[2] for m in md])
    r = rois.shape[0]
    out = torch.full((r * p * p + 64,), 7, dtype=torch.uint8, device=DEV)
    E.hip.call("u2_mask_crop_batch", ptrs, hs, ws, n, rois.to(DEV), img.to(DEV), out, r, p)
    torch.cuda.synchronize()
    assert bool((out[r * p * p:] == 7).all()) and not bool((out[: r * p * p] == 7).any())
    got = out[: r * p * p].view(r, p, p).cpu()
    lit = 0
    for i in sorted(set(img.tolist())):
        sel = img == i
        want = (R.mask_crop_ref(masks[i], rois[sel], p) >= 0.5).to(torch.uint8)
        first_diff("batched crop, image %d" % i, got[sel], want)
        first_diff("single crop, image %d" % i, E.F.mask_crop(md[i], rois[sel].to(DEV), p), want)
        lit += int(want.sum())
    assert lit > 200
    E.hip.call("u2_mask_crop_batch", ptrs, hs, ws, n, rois.to(DEV), img.to(DEV), out, 0, p)
    torch.cuda.synchronize()
    assert torch.equal(out[: r * p * p].view(r, p, p).cpu(), got) and bool((out[r * p * p:] == 7).all())


def test_mask_crop_random_inputs_decide_like_float64_outside_the_margin(E):
    """Kind B.  mask_crop_random_case (45 x 53 noise bitmaps, 24 ROIs with arbitrary fp32 corners, P = 28): a target pixel may
    differ from mask_crop_ref >= 0.5 only where |average - 0.5| < margin = 4 x max |oracle ROIAlign in fp32 - mask_crop_ref| on
    these inputs; such pixels are at most 0.1 %, and the oracle's fp32 form alone is held to the same."""
    masks, rois = R.mask_crop_random_case()
    avg = R.mask_crop_ref(masks, rois, 28)
    v32 = E.O.roi_align(masks[:, None].float(), rois, 28, 1.0)[:, 0].to(F64)
    dev = float((v32 - avg).abs().max())
    margin = 4 * dev       # measured on the CPU when written: dev 5.38e-6 -> margin 2.15e-5; 15 of 18816 pixels (0.08 %) inside it
    report("mask crop random", "max |oracle fp32 - float64|", dev)
    assert 0 < margin < 1e-4
    near = (avg - 0.5).abs() < margin
    share = float(near.double().mean())
    report("mask crop random", "share of pixels inside the margin", share)
    assert share <= 1e-3
    want = avg >= 0.5
    assert torch.equal((v32 >= 0.5)[~near], want[~near])          # the reference's fp32 form alone
    got = E.F.mask_crop(masks.to(DEV), rois.to(DEV), 28).cpu().bool()
    bad = (got != want) & ~near
    report("mask crop random", "pixels differing inside the margin", float(((got != want) & near).sum()))
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())    # seen on an MI355X: no pixel differs, inside the margin or out
    assert 0.2 < float(want.double().mean()) < 0.8
