"""The case tables of tests/loss_cases.py without a GPU: from the constants of the launchers in u2seg_amd/csrc/losses.hip,
restated here, every branch the tables are meant to reach is reached by some case; the generators deliver what their
docstrings promise; and the float64 reference alone has exactly as many L1 elements inside get_deltas' fp32 error bound as the
cases tie on purpose - the number the GPU test allows to take either sign."""
import pytest
import torch

from tests import float64_refs as R
from tests import loss_cases as C
from tests.test_gpu_heads_full_size import get_deltas64

F64 = torch.float64

# losses.hip, restated
REG_MAX_LP, REG_GRID_CAP, PIECE_LP = 1024, 512, 512      # softmax_ce_kernel: register form, its grid cap, columns per piece
SS_OW, SS_OH, SS_MAXC, SS_STAGED = 15, 7, 32, 32         # semseg_ce_kernel: owned taps, classes served, columns staged in LDS
MASK_SLICE_AT = ((512, 8), (128, 4), (0, 1))             # u2_mask_predict_bce: P >= first -> second slices
RPN_BLOCK, BOX_BLOCK, SCALE_BLOCK, SCALE_CAP = 256, 256, 256, 4096


def test_softmax_table_reaches_every_branch():
    cs = C.SOFTMAX_CASES
    assert len(set(cs)) == len(cs) == 11
    reg = [c for c in cs if c[2] <= REG_MAX_LP and c[2] % 8 == 0]
    gen = [c for c in cs if c not in reg]
    for c in cs:
        is_reg, grid, walk, atomics, terms = C.softmax_geometry(*c)
        assert is_reg == (c in reg) and c[1] <= c[2] and c[1] >= 2
        assert grid == (min(REG_GRID_CAP, -(-c[0] // 4)) if is_reg else -(-c[0] // 4))
        assert atomics == (4 * grid if is_reg else c[0]) and terms == (16 if is_reg else -(-c[1] // 64))
    assert any(lp <= PIECE_LP for _, _, lp in reg)                                  # one piece per lane
    assert any(lp == PIECE_LP and nc == lp for _, nc, lp in reg)                    # the second piece empty
    assert any(lp == PIECE_LP + 8 and nc == PIECE_LP + 1 for _, nc, lp in reg)      # one valid column in the second piece
    assert any(lp == REG_MAX_LP and nc % 8 and nc > lp - 8 for _, nc, lp in reg)    # widest row, partly valid last chunk
    assert any(nc == lp for _, nc, lp in reg) and any(lp == 8 for _, _, lp in reg)
    assert any(lp > REG_MAX_LP for _, _, lp in gen) and any(lp % 8 for _, _, lp in gen)
    assert any(r < 4 for r, _, _ in cs)                                             # fewer rows than a work-group
    assert any(-(-r // 4) > REG_GRID_CAP and r % 4 == 3 for r, _, _ in reg)         # capped: waves walk rows, a ragged end
    assert any(C.softmax_geometry(*c)[2] > 1 for c in reg) and any(1 < -(-c[0] // 4) < REG_GRID_CAP for c in reg)
    assert any(-(-r // 4) > REG_GRID_CAP and r % 4 == 2 for r, _, _ in gen)         # uncapped grid, waves past R return early
    assert (81 in [c[1] for c in cs]) and (301 in [c[1] for c in cs])               # the default head and u2seg_R50_300
    assert C.SOFTMAX_THIRD in cs and all(c in cs for c in C.SOFTMAX_WRAPPER)
    assert [C.softmax_geometry(*c)[0] for c in C.SOFTMAX_WRAPPER] == [True, False]


@pytest.mark.parametrize("case", C.SOFTMAX_CASES)
def test_softmax_rows_are_of_every_kind(case):
    r, nc, lp = case
    z, lab = C.softmax_case(*case)
    assert z.dtype == torch.bfloat16 and z.shape == (r, lp) and int(lab.min()) >= 0 and int(lab.max()) < nc
    assert lp == nc or float(z[:, nc:].float().min()) > 9000
    zz = z[:, :nc].to(F64)
    kind = torch.arange(r) % C.SOFTMAX_KINDS
    ref = R.softmax_ce_ref(z, lab, nc)
    p_lab = ref["p"].gather(1, lab[:, None])[:, 0]
    n_max = (zz == zz.amax(1, keepdim=True)).sum(1)
    if r >= C.SOFTMAX_KINDS:
        assert float(zz[kind == 1].abs().max()) > 30 and float(zz.abs().max()) <= 60
        assert bool((p_lab[kind == 2] > 1 - 1e-9).all()) and bool((p_lab[kind == 3] < 1e-9).all())
        assert bool((n_max[kind == 4] == nc).all())
        assert bool((n_max[kind == 5] >= 2).all()) and bool((R.first_argmax(zz)[kind == 5] == 0).all())
        six = kind == 6
        assert bool((zz[six, nc - 1] == zz[six].amax(1)).all()) and bool((n_max[six] >= 2).any())
        assert int(lab[7]) == 0 and (r < 16 or int(lab[15]) == nc - 1)
    pred = R.first_argmax(zz)
    assert torch.equal(zz.gather(1, pred[:, None])[:, 0], zz.amax(1))


def test_semseg_table_reaches_every_branch():
    cs = C.SEM_CASES
    assert len(set(cs)) == len(cs)
    maps = {(h, w) for _, h, w, nc, lp, ig, sat in cs if (nc, lp, ig, sat) == (28, 32, 255, False)}
    assert maps == set(C.SEM_MAPS) and all({b for b, h, w, *_ in cs if (h, w) == m} >= {1, 3} for m in C.SEM_MAPS)
    assert {(nc, lp) for _, h, w, nc, lp, *_ in cs if (h, w) == (8, 16)} == set(C.SEM_CLASSES)
    assert (3, 15, 31, 32, 32, 255, False) in cs
    assert any(h < SS_OH and w < SS_OW for h, w in maps)                             # smaller than a tile
    assert (SS_OH, SS_OW) in maps and (SS_OH + 1, SS_OW + 1) in maps                 # a tile exactly; one tap larger
    assert any(w == 1 and h > SS_OH for h, w in maps) and any(h == 1 and w > SS_OW for h, w in maps) and (1, 1) in maps
    assert any(C.sem_tiles(h, w) == (3, 3) for h, w in maps)                         # a tile with neighbours on every side
    ncs = {nc for nc, _ in C.SEM_CLASSES}
    assert {1, 8, 9, SS_MAXC} <= ncs and all(nc <= SS_MAXC and lp >= nc and lp % 8 == 0 for nc, lp in C.SEM_CLASSES)
    assert any(lp > SS_STAGED for _, lp in C.SEM_CLASSES) and any(lp > SS_STAGED and lp % 16 for _, lp in C.SEM_CLASSES)
    assert any(ig == 0 for *_, ig, _ in cs) and any(sat for *_, sat in cs)
    assert all(c in cs for c in C.SEM_WRAPPER) and {(h, w) for _, h, w, *_ in C.SEM_WRAPPER} == set(C.SEM_MAPS)


@pytest.mark.parametrize("case", C.SEM_CASES)
def test_semseg_targets_keep_the_contract(case):
    b, h, w, nc, lp, ignore, sat = case
    z, t = C.sem_case(*case)
    assert z.shape == (b, h, w, lp) and t.shape == (b, 4 * h, 4 * w) and t.dtype == torch.uint8
    tl = t.long()
    valid = tl != ignore
    assert bool((tl[valid] < nc).all()) and 0 < int(valid.sum()) < valid.numel()
    assert lp == nc or bool((z[..., nc:].float() == C.SEM_PAD).all())
    ny, nx = C.sem_tiles(h, w)
    ty, tx = C.sem_owner(h, w)
    assert int(ty.max()) == ny - 1 and int(tx.max()) == nx - 1
    per_tile = torch.zeros(ny * nx, dtype=torch.long).index_add_(
        0, (ty[:, None] * nx + tx[None, :]).reshape(-1), valid.sum(0).reshape(-1).long())
    if ny * nx > 1:
        assert int(per_tile[-1]) == 0 and bool((per_tile[:-1] > 0).all())             # one tile without a valid pixel
    if sat:
        zz = z[..., :nc].float()
        assert float((zz.amax(-1) - zz.median(-1).values).abs().max()) > 30


def test_mask_table_reaches_every_branch():
    cs = C.MASK_CASES
    slices = lambda p: next(s for at, s in MASK_SLICE_AT if p >= at)   # noqa: E731
    for n, side, phased, k in cs:
        p = side * side
        assert C.mask_slices(p) == slices(p) and (not phased or side % 2 == 0)
    ps = sorted(side * side for _, side, _, _ in cs)
    assert {slices(p) for p in ps} == {1, 4, 8}
    for at in (128, 512):      # the nearest squares on either side of each threshold
        below, above = max(s * s for s in range(1, 40) if s * s < at), min(s * s for s in range(1, 40) if s * s >= at)
        assert below in ps and above in ps
    assert any(p % (4 * slices(p)) for p in ps) and any(side % 2 for _, side, _, _ in cs) and min(ps) == 4
    assert any(ph and side != 28 for _, side, ph, _ in cs) and {slices(s * s) for _, s, ph, _ in cs if ph} == {4, 8}
    assert any(n == 1 for n, *_ in cs) and any(k == 1 for *_, k in cs) and any(n == 1 and ph for n, _, ph, _ in cs)
    all0 = all1 = big = 0
    for case in cs:
        n, side, phased, k = case
        x, w, bias, cls, tgt = C.mask_case(*case)
        assert x.shape == (n, side * side, C.MASK_C) and int(cls.min()) >= 0 and int(cls.max()) < k and w.shape == (k, C.MASK_C)
        assert n < 2 or int(cls[0]) == int(cls[1])
        all0 += int((tgt.sum(1) == 0).sum())
        all1 += int((tgt.sum(1) == side * side).sum())
        ref = R.mask_bce_ref(x, w, bias, cls, tgt)
        big += int((ref["logit"].abs() > 20).sum())
        assert float(ref["logit"][0, 0]) > 20 and float(ref["logit"][0, 1]) < -20 and float(ref["logit"].abs().max()) < 88
    assert all0 >= 2 and all1 >= 2 and big >= 2 * len(cs)


def test_rpn_table_reaches_every_branch():
    sep, fus = C.RPN_SEPARATE, C.RPN_FUSED
    assert {a for _, _, a, _, _ in sep} == {1, 2, 3, 4}
    assert {lpo for *_, lpo, _ in sep} == {8, 16} and {lpd for *_, lpd in sep} == {16, 32}
    assert {lpo for *_, lpo in fus} == {16, 32, 40}
    for group in (sep, fus):
        bhw = [c[0] * c[1] for c in group]
        assert 1 in [c[1] for c in group]                                            # HW = 1
        assert any(n < RPN_BLOCK for n in bhw) and any(n > RPN_BLOCK for n in bhw)   # either side of a work-group
        assert any(n % RPN_BLOCK for n in bhw if n > RPN_BLOCK)
    assert any(C.rpn_grid(c[0], c[1]) == 3 for c in sep + fus)
    no_pos = no_label = ties = 0
    gs = set()
    for case in C.RPN_CASES:
        b, hw, a, lpo, lpd, fused = case
        c = C.rpn_case(*case)
        o, d, lab, mt = C.rpn_views(c)
        assert c["lvl_off"] > 0 and c["atot"] == c["lvl_off"] + hw * a and c["labels"].shape == (b, c["atot"])
        assert bool((c["labels"][:, : c["lvl_off"]] == 1).all())
        assert int(mt.min()) >= 0 and int(mt.max()) < c["G"] and c["gt"].shape == (b, c["G"], 4)
        assert int(lab.min()) >= -1 and int(lab.max()) <= 1 and int((lab == 1).sum()) > 0
        wh = torch.cat([c["anchors"][:, 2:] - c["anchors"][:, :2], (c["gt"][..., 2:] - c["gt"][..., :2]).reshape(-1, 2)])
        assert float(wh.min()) >= 4
        pads = c["obj"][..., (15 if fused else a):].float()
        assert pads.numel() == 0 or float(pads.min()) > 9000
        assert fused or 4 * a == lpd or float(c["dlt"][..., 4 * a:].float().min()) > 9000
        no_pos += int((((lab == 1).sum(1) == 0) & ((lab >= 0).sum(1) > 0)).sum())
        no_label += int(((lab >= 0).sum(1) == 0).sum())
        gs.add(c["G"])
        # the ambiguity cap: the reference alone has exactly the constructed ties inside get_deltas' fp32 error
        ref = R.rpn_level_ref(o, d, lab, mt, c["gt"], c["anchors"], a)
        _, e = get_deltas64(ref["src"], ref["dst"], (1.0, 1.0, 1.0, 1.0))
        assert int((ref["df"].abs() <= e).sum()) == c["ties"], case
        ties += c["ties"]
    assert no_pos >= 2 and no_label >= 2 and gs == {1, 5} and ties >= 8


@pytest.mark.parametrize("weights", C.BOX_WEIGHTS)
def test_box_table_reaches_every_branch_and_holds_its_ties(weights):
    rs = [r for r, _, _ in C.BOX_CASES]
    assert 1 in rs and BOX_BLOCK - 1 in rs and BOX_BLOCK + 1 in rs and {lp for _, lp, _ in C.BOX_CASES} == {8, 32}
    assert any(bg and lp == 8 and r > BOX_BLOCK for r, lp, bg in C.BOX_CASES)
    for r, lp, all_bg in C.BOX_CASES:
        pred, prop, gt, lab, ties = C.box_case(r, lp, all_bg, weights)
        ref = R.box_l1_ref(pred, prop, gt, lab, C.BOX_BG, weights)
        fg = ref["fg"]
        assert int(lab.min()) >= 0 and int(lab.max()) <= C.BOX_BG and float(pred[:, 4:].float().min()) > 9000
        assert (int(fg.sum()) == 0) == all_bg and (all_bg or r == 1 or 0 < int(fg.sum()) < r)
        _, e = get_deltas64(prop, gt, weights)
        assert int((ref["df"].abs() <= e)[fg].sum()) == ties, (r, lp)
        if ties:
            k = C.BOX_TIED_ROWS
            assert ties == 4 * k and bool((ref["df"][:k] == 0).all())
            assert torch.equal(pred[k: 2 * k, :4].to(F64), ref["tgt"][k: 2 * k].to(torch.bfloat16).to(F64))


def test_scale_table():
    ns = C.SCALE_N
    assert 1 in ns and SCALE_BLOCK - 1 in ns and SCALE_BLOCK + 1 in ns
    assert any(-(-n // SCALE_BLOCK) > SCALE_CAP and n % SCALE_BLOCK for n in ns)    # past the cap: the grid-stride loop, ragged
    assert {(a, b) for a, b, _ in C.SCALE_ARGS} == {(True, True), (False, True), (True, False)}
    assert {m for *_, m in C.SCALE_ARGS} == {1.0, 0.5}
