"""u2_rpn_loss_level_opt, u2_box_reg_loss_cls (u2seg_amd/csrc/losses.hip) and u2_apply_deltas_cls (csrc/roi.hip): against the
entries they extend bit for bit where they must agree, per element against the float64 restatements of
tests/box_loss_refs.py with the derived bounds of tests/test_gpu_box_loss_options.py (box_expect / check_box, read there)
elsewhere, and a StandardROIHeads model with class-specific regression and a GIoU RPN loss against the torch definitions of
u2seg_amd/modeling/box_losses.py and a per-image torch restatement of the inference tail.

The inputs are those of tests/box_regression_cases.py; tests/test_box_regression_options_host.py holds their ambiguity cap
on the CPU by the float64 side alone.

Summation depth of the loss words.  check_box allows ceil(R / (grid 256)) + 8 + 4 + grid roundings with grid = ceil(R / 256).
u2_box_reg_loss_cls sums exactly as u2_box_reg_loss does (one thread per row, 256 rows per work-group): the same figure.
u2_rpn_loss_level_opt is called one level at a time into a loss word of its own: a thread adds its position's <= 3 positives,
the wave 6 levels, the work-group 2, one atomic: 11 <= 14 for the levels used here (one work-group each)."""
import json
import math
import os

import pytest
import torch

from tests import box_regression_cases as cases
from tests.test_gpu_box_loss_options import DEV, box_expect, check_box
from tests.test_gpu_heads_full_size import U, get_deltas64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800_standard_heads.yaml")
F64 = torch.float64
BF16 = torch.bfloat16
CLAMP, BETA = cases.CLAMP, cases.BETA
RPN_SEED = 4100
CLS_SHAPES = [(1, 12, 64), (65, 12, 64), (300, 12, 64), (512, 800, 3200)]      # (R, K, LP); the last is the real pitch
FORMS = [("smooth_l1", BETA), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0)]


def cls_seed(R, K):
    return 5001 + R + K   # (5000: one drawn row of R = 300 and of R = 512 falls within four decode errors of a branch)


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
# the RPN level kernel
# =================================================================================================
def run_rpn(H, case, fused, options):
    """Every level through u2_rpn_loss_level (options None) or u2_rpn_loss_level_opt (kind code, beta, weights), each into its
    own loss words, the gradient maps prefilled with NaN.  Returns per level (dobj [B, n], ddeltas [B, n, 4], pads, loss [2])."""
    labels, match, gt = case["labels"].to(DEV), case["match"].to(DEV), case["gt"].to(DEV)
    atot = labels.shape[1]
    out, off = [], 0
    for (h, w, _, _), anc, (o, d) in zip(cases.RPN_LEVELS, case["anchors"], cases.rpn_maps(case, fused, DEV)):
        go = torch.full_like(o, float("nan"))
        gd = None if fused else torch.full_like(d, float("nan"))
        loss = torch.zeros(2, dtype=torch.float32, device=DEV)
        args = (o, d, labels, match, gt, anc.to(DEV), go, gd, loss, cases.RPN_B, h * w, cases.RPN_A, o.shape[3],
                0 if fused else d.shape[3], atot, off, cases.RPN_G, 1.0 / cases.RPN_NORM)
        if options is None:
            H.call("u2_rpn_loss_level", *args)
        else:
            kind, beta, weights = options
            H.call("u2_rpn_loss_level_opt", kind, *args, *weights, beta, CLAMP)
        out.append(cases.rpn_split_grads(go, gd, fused) + (loss,))
        off += anc.shape[0]
    assert off == atot
    return out


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_rpn_default_options_give_the_old_entrys_bits(F, H, fused):
    """smooth_l1, beta 0, unit weights: both loss words and every element of the gradient maps, pads (prefilled with NaN) included."""
    case = cases.rpn_case(cases.RPN_WEIGHTS[0], RPN_SEED)
    old = run_rpn(H, case, fused, None)
    new = run_rpn(H, case, fused, (F.BOX_REG_LOSS_KINDS["smooth_l1"], 0.0, (1.0, 1.0, 1.0, 1.0)))
    for lvl, (a, b) in enumerate(zip(old, new)):
        for x, y, what in zip(a, b, ("dobj", "ddeltas", "pads", "loss")):
            assert not bool(torch.isnan(y.float()).any()), (lvl, what)
            assert torch.equal(x, y), (lvl, what)
        assert float(b[2].float().abs().max()) == 0.0 and float(b[3][1]) > 0.0


@pytest.mark.parametrize("wi", [0, 1], ids=["unit", "w10-10-5-5"])
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("kind,beta", FORMS)
def test_rpn_loss_level_options(F, H, kind, beta, fused, wi):
    """Per element against float64 with the bounds of box_expect / check_box, level by level.  With the second weights the
    second level has no positive anchor; the second image has no ground truth."""
    weights = cases.RPN_WEIGHTS[wi]
    case = cases.rpn_case(weights, RPN_SEED + wi, empty_level=bool(wi))
    got = run_rpn(H, case, fused, (F.BOX_REG_LOSS_KINDS[kind], beta, weights))
    base = run_rpn(H, case, fused, None)
    for lvl, ((dobj, dd, pads, loss), (dobj0, _, _, loss0)) in enumerate(zip(got, base)):
        name = "rpn_loss_level_opt %s %s w%d level %d" % (kind, "fused" if fused else "separate", wi, lvl)
        # the objectness part is the old entry's, bit for bit; the pads are exactly 0
        assert torch.equal(dobj, dobj0) and torch.equal(loss[0], loss0[0]), name
        assert float(pads.float().abs().max()) == 0.0 and not bool(torch.isnan(dd.float()).any()), name
        pred, prop, gtm, lab, planted = cases.rpn_level_rows(case, lvl)
        off = sum(a.shape[0] for a in case["anchors"][:lvl])
        n = case["anchors"][lvl].shape[0]
        not_pos = (case["labels"][:, off:off + n] != 1).to(DEV)
        assert float(dd[not_pos].float().abs().max()) == 0.0, name + ": labels 0 and -1"
        if int((lab < 800).sum()) == 0:
            assert lvl == 1 and wi == 1 and float(loss[1]) == 0.0 and float(dd.float().abs().max()) == 0.0, name
            continue
        grad4 = torch.zeros((pred.shape[0], 8), dtype=BF16, device=DEV)        # (check_box also wants columns >= 4 to be zero)
        grad4[:, :4] = dd.reshape(-1, 4)
        ex = check_box(name, kind, grad4, loss[1] / cases.RPN_NORM, pred.to(DEV), prop.to(DEV), gtm.to(DEV), lab.to(DEV), weights,
                       cases.RPN_NORM, planted)
        if lvl == 0 and kind != "smooth_l1":
            assert bool(ex["clamped"][4, 2]) and float(ex["rows"][0]) > 1.0 and bool(ex["amb"][3])   # clamp, disjoint, pred == gt


def test_rpn_loss_level_opt_refusals(F, H):
    case = cases.rpn_case(cases.RPN_WEIGHTS[0], RPN_SEED)
    giou = F.BOX_REG_LOSS_KINDS["giou"]
    for options in ((7, 0.0, (1.0, 1.0, 1.0, 1.0)), (-1, 0.0, (1.0, 1.0, 1.0, 1.0)), (giou, 0.0, (1.0, 1.0, 0.0, 1.0)),
                    (giou, 0.0, (1.0, -1.0, 1.0, 1.0)), (F.BOX_REG_LOSS_KINDS["smooth_l1"], -0.5, (1.0, 1.0, 1.0, 1.0))):
        with pytest.raises(RuntimeError, match="u2_rpn_loss_level_opt"):
            run_rpn(H, case, False, options)


def test_rpn_losses_routes_by_options(F, H, monkeypatch):
    """layers/losses.py: the default options still call u2_rpn_loss_level, anything else the new entry, and autograd hands the
    kernel's gradient maps on."""
    case = cases.rpn_case(cases.RPN_WEIGHTS[1], RPN_SEED + 1)
    called = []
    real = H.call
    monkeypatch.setattr(H, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    labels, match, gt = case["labels"].to(DEV), case["match"].to(DEV), case["gt"].to(DEV)
    anchors = [a.to(DEV) for a in case["anchors"]]

    def run(**opts):
        maps = cases.rpn_maps(case, False, DEV, pad=0.0)
        objs = [o.requires_grad_(True) for o, _ in maps]
        dlts = [d.requires_grad_(True) for _, d in maps]
        cls, loc = F.rpn_losses(labels, match, gt, anchors, cases.RPN_A, cases.RPN_NORM, objs, dlts, **opts)
        (cls + loc).backward()
        return cls.detach(), loc.detach(), [d.grad for d in dlts]

    c0, l0, _ = run()
    assert set(called) == {"u2_rpn_loss_level"}
    del called[:]
    c1, l1, g1 = run(box_reg_loss_type="giou", weights=cases.RPN_WEIGHTS[1])
    assert set(called) == {"u2_rpn_loss_level_opt"} and torch.equal(c0, c1) and not torch.equal(l0, l1)
    direct = run_rpn(H, case, False, (F.BOX_REG_LOSS_KINDS["giou"], 0.0, cases.RPN_WEIGHTS[1]))
    assert torch.equal(l1, (direct[0][3][1] + direct[1][3][1]) / cases.RPN_NORM)
    for g, (_, dd, _, _) in zip(g1, direct):
        assert torch.equal(g[..., :12].reshape(dd.shape), dd)
    with pytest.raises(ValueError, match="eiou"):
        run(box_reg_loss_type="eiou")
    with pytest.raises(ValueError, match="positive"):
        run(weights=(1.0, 1.0, 0.0, 1.0))


# =================================================================================================
# class-specific regression: loss and decode
# =================================================================================================
def run_cls_loss(H, F, kind, beta, pred, prop, gt, lab, K):
    R, LP = pred.shape
    d = torch.full_like(pred, float("nan"))
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    H.call("u2_box_reg_loss_cls", F.BOX_REG_LOSS_KINDS[kind], pred, prop, gt, lab, d, loss, R, LP, K, *cases.HEAD_WEIGHTS, beta,
           CLAMP, 1.0 / R)
    return d, loss


def run_agnostic(H, F, kind, beta, own, prop, gt, lab800):
    """u2_box_reg_l1 / u2_box_reg_loss on the gathered [R, 4] columns."""
    R = own.shape[0]
    own = own.contiguous()
    d = torch.full_like(own, float("nan"))
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    if kind == "smooth_l1" and beta == 0.0:
        H.call("u2_box_reg_l1", own, prop, gt, lab800, d, loss, R, 4, 800, *cases.HEAD_WEIGHTS, 1.0 / R)
    else:
        H.call("u2_box_reg_loss", F.BOX_REG_LOSS_KINDS[kind], own, prop, gt, lab800, d, loss, R, 4, 800, *cases.HEAD_WEIGHTS, beta,
               CLAMP, 1.0 / R)
    return d, loss


def l1_expect(own, prop, gt, fg, norm):
    """float64 L1 sum over the foreground rows / norm and its bound: box_expect's smooth-L1 bound above beta (value
    1-Lipschitz in df), the summation depth of check_box."""
    tgt, e_t = get_deltas64(prop[fg], gt[fg], cases.HEAD_WEIGHTS)
    df = own[fg].to(F64) - tgt
    rows = df.abs().sum(1)
    e_rows = (e_t + U * df.abs()).sum(1) + 8 * U * rows
    R = own.shape[0]
    grid = min((R + 255) // 256, 1024)
    depth = -(-R // (grid * 256)) + 8 + 4 + grid
    ref = float(rows.sum()) / norm
    return ref, (float(e_rows.sum()) + depth * U * float(rows.sum())) / norm + 2 * U * abs(ref)


def cls_loss_case(F, H, kind, beta, R, K, LP):
    pred, prop, gt, lab = (t.to(DEV) for t in cases.cls_case(R, K, LP, cases.HEAD_WEIGHTS, cls_seed(R, K)))
    name = "box_reg_loss_cls %s beta %g R=%d K=%d" % (kind, beta, R, K)
    d, loss = run_cls_loss(H, F, kind, beta, pred, prop, gt, lab, K)
    own, lab800 = cases.cls_gathered(pred, lab, K)
    d_ag, loss_ag = run_agnostic(H, F, kind, beta, own, prop, gt, lab800)
    fg = lab < K
    cols = cases.cls_columns(lab, K)
    mine = d.gather(1, cols)
    # the labelled class's four columns: the bits of the class-agnostic entries on the gathered columns
    assert torch.equal(mine[fg], d_ag[fg]), name
    # everything else - other classes, pads, background rows - exactly 0 over the NaN prefill
    rest = d.clone()
    rest[fg] = rest[fg].scatter(1, cols[fg], torch.zeros_like(mine[fg]))
    assert float(rest.float().abs().max()) == 0.0 and not bool(torch.isnan(rest.float()).any()), name
    planted = cases.N_PLANTED if R >= 65 else 0
    if beta == 0.0 and kind == "smooth_l1":
        ref, bound = l1_expect(own, prop, gt, fg, R)
        err = abs(float(loss) / R - ref)
        print("%s: loss %.9g ref %.9g error %.3g of bound %.3g" % (name, float(loss) / R, ref, err, 2 * bound))
        assert err <= 2 * bound, name
    else:
        grad4 = torch.zeros((R, 8), dtype=BF16, device=DEV)
        grad4[:, :4] = torch.where(fg[:, None], mine, torch.zeros_like(mine))
        ex = check_box(name, kind, grad4, loss[0] / R, own, prop, gt, lab800, cases.HEAD_WEIGHTS, R, planted)
        if R >= 65 and kind != "smooth_l1":
            assert bool(ex["clamped"][4, 2]) and float(ex["rows"][0]) > 1.0
    assert int(fg.sum()) >= 1 and float(loss) > 0.0
    # through layers/functional.py and autograd: the same bits
    pd = pred.detach().requires_grad_(True)
    out = F.box_reg_loss_cls(kind, pd, prop, gt, lab, K, cases.HEAD_WEIGHTS, R, beta, CLAMP)
    out.backward()
    assert torch.equal(pd.grad, d) and torch.equal(out.detach(), loss[0] / R), name


@pytest.mark.parametrize("R,K,LP", CLS_SHAPES[:3], ids=lambda v: str(v))
@pytest.mark.parametrize("kind,beta", FORMS + [("smooth_l1", 0.0)], ids=["smooth_l1", "giou", "diou", "ciou", "l1"])
def test_box_reg_loss_cls(F, H, kind, beta, R, K, LP):
    """K = 12, LP = 64: R = 65 crosses a wave, R = 300 a work-group's 256 rows."""
    cls_loss_case(F, H, kind, beta, R, K, LP)


def test_box_reg_loss_cls_at_the_real_pitch(F, H):
    """K = 800, LP = 3200, R = 512: rows of 400 16-byte pieces, two work-groups."""
    cls_loss_case(F, H, "giou", 0.0, *CLS_SHAPES[3])


def test_box_reg_loss_cls_refusals(F, H):
    K, LP = 12, 64
    pred = torch.zeros((4, LP), dtype=BF16, device=DEV)
    box = torch.tensor([[0.0, 0.0, 10.0, 10.0]] * 4, device=DEV)
    lab = torch.zeros(4, dtype=torch.int64, device=DEV)
    d = torch.full_like(pred, 7.0)
    loss = torch.full((1,), 3.0, dtype=torch.float32, device=DEV)
    giou = F.BOX_REG_LOSS_KINDS["giou"]
    H.call("u2_box_reg_loss_cls", giou, pred, box, box, lab, d, loss, 0, LP, K, 10.0, 10.0, 5.0, 5.0, 0.0, CLAMP, 1.0)   # R == 0
    assert float(loss) == 3.0 and bool((d == 7.0).all())
    for kind, lp, k, beta in ((giou, 32, K, 0.0), (giou, 47, K, 0.0), (7, LP, K, 0.0), (giou, LP, 0, 0.0),
                              (F.BOX_REG_LOSS_KINDS["smooth_l1"], LP, K, -1.0)):        # LP < 4 K twice, kind, K, beta
        with pytest.raises(RuntimeError, match="u2_box_reg_loss_cls"):
            H.call("u2_box_reg_loss_cls", kind, pred, box, box, lab, d, loss, 4, lp, k, 10.0, 10.0, 5.0, 5.0, beta, CLAMP, 1.0)
    assert float(loss) == 3.0 and bool((d == 7.0).all())
    with pytest.raises(ValueError, match="eiou"):
        F.box_reg_loss_cls("eiou", pred, box, box, lab, K, (10.0, 10.0, 5.0, 5.0), 4)


@pytest.mark.parametrize("R", [1, 65])
@pytest.mark.parametrize("dtype", [BF16, torch.float32], ids=["bf16", "fp32"])
def test_apply_deltas_cls(F, H, R, dtype):
    """[R, 4 K] equals u2_apply_deltas on each class's gathered columns bit for bit; one dw lies above the clamp."""
    K, LP = 12, 64
    pred, prop, _, _ = cases.cls_case(max(R, 2), K, LP, cases.HEAD_WEIGHTS, cls_seed(R, K) + 1)
    pred, prop = pred[:R].clone(), prop[:R].contiguous().to(DEV)
    pred[0, 4 * 5 + 2] = 5.0 * cases.HEAD_WEIGHTS[2] + 1.0          # class 5 of row 0: dw > log(1000 / 16)
    pred[R - 1, 4 * 11 + 3] = float("nan")                          # a NaN size delta stays NaN (the decode keeps it)
    pred = pred.to(dtype).to(DEV)
    got = F.apply_deltas_cls(prop, pred, K, cases.HEAD_WEIGHTS, CLAMP)
    assert got.shape == (R, 4 * K) and got.dtype == torch.float32
    for c in range(K):
        want = F.apply_deltas(prop, pred[:, 4 * c:4 * c + 4].float().contiguous(), cases.HEAD_WEIGHTS, None, None, CLAMP)
        both_nan = torch.isnan(got[:, 4 * c:4 * c + 4]) & torch.isnan(want)
        assert torch.equal(torch.where(both_nan, 0.0, got[:, 4 * c:4 * c + 4]), torch.where(both_nan, 0.0, want)), c
    w0 = float(prop[0, 2] - prop[0, 0])
    assert float(got[0, 22] - got[0, 20]) == pytest.approx(1000.0 / 16 * w0, rel=1e-5)       # the clamped width
    assert bool(torch.isnan(got[R - 1, 4 * 11 + 1])) and bool(torch.isfinite(got[R - 1, 4 * 11]))
    with pytest.raises(RuntimeError, match="u2_apply_deltas_cls"):
        F.apply_deltas_cls(prop, pred, 17, cases.HEAD_WEIGHTS, CLAMP)                         # LP < 4 K


# =================================================================================================
# StandardROIHeads with the options on
# =================================================================================================
HOT_CLASSES = {5: 7.0, 310: 6.25, 777: 5.5}      # class -> bias
MODEL_OPTS = ["MODEL.DEVICE", DEV, "MODEL.RPN.POST_NMS_TOPK_TEST", 40, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.05,
              "TEST.DETECTIONS_PER_IMAGE", 50, "TEST.AUG.MIN_SIZES", (96,), "TEST.AUG.MAX_SIZE", 160]


@pytest.fixture
def standard_model(F):
    """u2seg_R50_800_standard_heads.yaml (StandardROIHeads, class-specific regression, GIoU in the RPN) at the small size of
    tests/golden/model_small.json with det_fill weights.  The class scores are CHOSEN: the classifier's weights are scaled to a
    tenth (logits within about +-0.5 of their bias) and three classes get biases 0.75 apart, so that these three pass the score
    threshold for every proposal (softmax about 0.4, 0.2 and 0.09) and no two logits of a row are equal in bf16: scores tie
    neither within a row nor, their rows' sums differing, across rows.  Built anew for every test: a training step moves the
    running statistics, and the inference test's preconditions are stated for the model as filled."""
    from tests.golden.make_fixtures import det_fill
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model

    with open(os.path.join(ROOT, "tests", "golden", "model_small.json")) as f:
        fx = json.load(f)
    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(MODEL_OPTS)
    torch.manual_seed(fx["seed"])
    model = build_model(cfg)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(det_fill(k, v.cpu()).to(DEV))
        model.roi_heads.box_predictor.cls_score.weight.mul_(0.1)
        for c, b in HOT_CLASSES.items():
            model.roi_heads.box_predictor.cls_score.bias[c] += b
    return cfg, model, fx


def test_standard_heads_with_options_against_torch_definitions(F, standard_model, monkeypatch):
    """One training step: the class-specific box loss and the RPN's GIoU loss against float64 and against the torch definitions
    on the inputs the kernels were given (teacher forced), within the bounds of box_expect; gradients reach bbox_pred and the
    RPN's delta predictor."""
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.modeling import box_losses as BL

    cfg, model, fx = standard_model
    model.train()
    box_calls, rpn_calls = [], []
    box, rpn = F.box_reg_loss_cls, F.rpn_losses

    def box_reg_loss_cls(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0, scale_clamp=CLAMP):
        out = box(kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta, scale_clamp)
        box_calls.append((kind, pred.detach().clone(), proposals.clone(), gt_boxes.clone(), labels.clone(), bg_label, weights,
                          normalizer, beta, out.detach().clone()))
        return out

    def rpn_losses(labels, match, gt, anchors, num_anchors, normalizer, objs, deltas, *options):
        out = rpn(labels, match, gt, anchors, num_anchors, normalizer, objs, deltas, *options)
        fused = all(getattr(o, "_u2_rpn_fused", False) for o in objs)
        b = labels.shape[0]
        a = num_anchors
        dl = [(o[..., a:5 * a] if fused else d[..., :4 * a]).detach().reshape(b, -1, 4) for o, d in zip(objs, deltas)]
        ob = [o[..., :a].detach().reshape(b, -1) for o in objs]
        rpn_calls.append((labels.clone(), match.clone(), gt.clone(), torch.cat(anchors), torch.cat(ob, 1), torch.cat(dl, 1),
                          normalizer, options, [o.shape[1] * o.shape[2] for o in objs], out[0].detach().clone(),
                          out[1].detach().clone()))
        return out

    monkeypatch.setattr(F, "box_reg_loss_cls", box_reg_loss_cls)
    monkeypatch.setattr(F, "rpn_losses", rpn_losses)
    h, w = fx["image_hw"]
    batch = make_synthetic_batch(fx["num_images"], start_index=0, height=h, width=w, device=DEV)
    losses = model(batch)
    assert sorted(losses) == ["loss_box_reg", "loss_cls", "loss_mask", "loss_rpn_cls", "loss_rpn_loc", "loss_sem_seg"]
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert len(box_calls) == 1 and len(rpn_calls) == 1
    # ---- the class-specific box loss
    kind, pred, prop, gtb, lab, bg, weights, norm, beta, got = box_calls[0]
    assert (kind, bg, beta, tuple(weights)) == ("smooth_l1", 800, 0.0, cases.HEAD_WEIGHTS) and pred.shape[1] == 3200
    assert norm == pred.shape[0] and float(got) == float(losses["loss_box_reg"].detach())
    own, lab800 = cases.cls_gathered(pred, lab, 800)
    fg = lab < 800
    ref, bound = l1_expect(own, prop, gtb, fg, norm)
    want = float(BL.box_reg_loss(kind, pred, prop, gtb, lab, 800, weights, beta, CLAMP, cls_agnostic=False)) / norm
    print("loss_box_reg %.6g (torch definition %.6g, float64 %.6g), %d fg rows" % (float(got), want, ref, int(fg.sum())))
    assert int(fg.sum()) >= 1 and abs(float(got) - ref) <= 2 * bound and abs(float(got) - want) <= 4 * bound
    # ---- the RPN's GIoU loss
    labels, match, gt, anchors, obj, deltas, norm, options, hws, got_cls, got_loc = rpn_calls[0]
    assert options[0] == "giou" and tuple(options[2]) == (1.0, 1.0, 1.0, 1.0) and norm == 256 * fx["num_images"]
    assert float(got_loc) == float(losses["loss_rpn_loc"].detach())
    b_idx, a_idx = torch.nonzero(labels == 1, as_tuple=True)
    n_pos = b_idx.numel()
    rows_pred, rows_src = deltas[b_idx, a_idx], anchors[a_idx]
    rows_gt = gt[b_idx, match[b_idx, a_idx].long()]
    ex = box_expect("giou", rows_pred, rows_src, rows_gt, torch.ones(n_pos, dtype=torch.bool, device=DEV), options[2], 1.0 / norm)
    ref = float(ex["rows"].sum()) / norm
    grids = sum(min(-(-labels.shape[0] * hw // 256), 2048) for hw in hws)
    bound = (float(ex["e_rows"].sum()) + (3 + 10 + grids) * U * float(ex["rows"].abs().sum())) / norm + 2 * U * abs(ref)
    want = float(BL.rpn_box_reg_loss("giou", labels, match, gt, anchors, deltas, options[2], 0.0, CLAMP)) / norm
    want_cls = float(BL.rpn_objectness_loss(labels, obj)) / norm
    print("loss_rpn_loc %.6g (torch definition %.6g, float64 %.6g), %d positives; loss_rpn_cls %.6g (%.6g)" % (
        float(got_loc), want, ref, n_pos, float(got_cls), want_cls))
    assert n_pos >= 4 and abs(float(got_loc) - ref) <= 2 * bound and abs(float(got_loc) - want) <= 4 * bound
    assert float(got_cls) == pytest.approx(want_cls, rel=1e-4)
    # ---- gradients reach the predictors
    p = model.roi_heads.box_predictor
    for layer in (p.cls_score, p.bbox_pred, model.proposal_generator.rpn_head.anchor_deltas):
        gsum = float(layer.weight.grad.float().abs().sum())
        assert math.isfinite(gsum) and gsum > 0, layer
    # only the labelled classes' rows of bbox_pred receive a gradient
    rows = p.bbox_pred.weight.grad.float().abs().sum(1).reshape(800, 4).sum(1)
    seen = torch.zeros(800, dtype=torch.bool, device=DEV)
    seen[lab[fg]] = True
    assert float(rows[~seen].max()) == 0.0 and bool((rows[seen] > 0).all())
    model.zero_grad(set_to_none=True)


def iou64(a, b):
    lt, rb = torch.maximum(a[:, None, :2], b[None, :, :2]), torch.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = (rb - lt).clamp(min=0).prod(2)
    area_a, area_b = (a[:, 2:] - a[:, :2]).prod(1), (b[:, 2:] - b[:, :2]).prod(1)
    return inter / (area_a[:, None] + area_b[None] - inter)


def inference_single_image(boxes, scores, shape, score_thresh, nms_thresh, topk):
    """fast_rcnn_inference_single_image (fast_rcnn.py:117-171) restated: pick the box by class, clip, threshold, batched NMS by
    class (greedy, in score order), top-k.  Also returns the preconditions' figures: (distinct scores, smallest distance of a
    same-class IoU from the NMS threshold)."""
    k = scores.shape[1] - 1
    valid = torch.isfinite(boxes).all(1) & torch.isfinite(scores).all(1)
    boxes, scores = boxes[valid].float().reshape(-1, k, 4), scores[valid][:, :k]
    h, w = shape
    boxes = torch.stack((boxes[..., 0].clamp(0, w), boxes[..., 1].clamp(0, h), boxes[..., 2].clamp(0, w), boxes[..., 3].clamp(0, h)), -1)
    roi, cls = torch.nonzero(scores > score_thresh, as_tuple=True)
    cb, cs = boxes[roi, cls], scores[roi, cls]
    order = torch.sort(cs, descending=True, stable=True)[1]
    cb, cs, cls = cb[order].cpu(), cs[order].cpu(), cls[order].cpu()
    keep, margin = [], float("inf")
    for c in cls.unique().tolist():
        idx = torch.nonzero(cls == c).flatten()
        iou = iou64(cb[idx].to(F64), cb[idx].to(F64))
        off_diag = ~torch.eye(len(idx), dtype=torch.bool)
        if bool(off_diag.any()):
            margin = min(margin, float((iou[off_diag] - nms_thresh).abs().min()))
        alive = torch.ones(len(idx), dtype=torch.bool)
        for i in range(len(idx)):
            if alive[i]:
                keep.append(int(idx[i]))
                alive &= ~(iou[i] > nms_thresh) | (torch.arange(len(idx)) <= i)
    keep = sorted(keep)[:topk] if topk >= 0 else sorted(keep)                # candidate index = score rank
    keep = torch.tensor(keep, dtype=torch.int64)
    return cb[keep], cs[keep], cls[keep], (int(cs.unique().numel()) == int(cs.numel()), margin, int(cs.numel()))


def test_standard_heads_inference_equals_the_per_image_restatement(F, standard_model, monkeypatch):
    """Eval mode on two images of different size: the instances are those of the restatement above on the [R_i, 4 K] boxes and
    [R_i, K + 1] scores the heads handed to the tail, image by image.  (Measured for these two images: 120 candidates each, NMS
    alone keeps 111 and 113, the top-k cut 50; the nearest same-class IoU lies 0.014 and 0.005 from the threshold.)"""
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.modeling import inference

    cfg, model, fx = standard_model
    model.eval()
    seen = []
    tail = inference.fast_rcnn_inference

    def fast_rcnn_inference(boxes, scores, image_shapes, *a):
        out = tail(boxes, scores, image_shapes, *a)
        seen.append(([b.clone() for b in boxes], [s.clone() for s in scores], list(image_shapes), a, out[0]))
        return out

    monkeypatch.setattr(inference, "fast_rcnn_inference", fast_rcnn_inference)
    batch = []
    for i, (h, w) in enumerate([(160, 224), (192, 256)]):
        x = make_synthetic_batch(1, start_index=i, height=h, width=w, device=DEV)[0]
        batch.append({"image": x["image"], "height": h, "width": w})
    with torch.no_grad():
        out = model(batch)
    (boxes, scores, shapes, (score_thresh, nms_thresh, topk), results), = seen
    assert (score_thresh, nms_thresh, topk) == (0.05, 0.5, 50) and len(boxes) == 2 and shapes[0] != shapes[1]
    want = [inference_single_image(b, s, shape, score_thresh, nms_thresh, topk) for b, s, shape in zip(boxes, scores, shapes)]
    for i, (b, (_, ws, _, (distinct, margin, ncand))) in enumerate(zip(boxes, want)):
        print("image %d: %d proposals, %d candidates, %d kept, scores distinct: %s; smallest |IoU - thr| %.3g" % (
            i, b.shape[0], ncand, len(ws), distinct, margin))
    for b, s, res, (wb, ws, wc, (distinct, margin, ncand)) in zip(boxes, scores, results, want):
        assert b.shape[1] == 3200 and s.shape[1] == 801 and b.shape[0] == s.shape[0] >= 1
        assert distinct and margin > 1e-4, "precondition: no tied scores, no IoU within 1e-4 of the threshold"
        assert 1 <= len(ws) < ncand                                            # something is kept and something suppressed or cut
        assert set(wc.tolist()) <= set(HOT_CLASSES)
        assert torch.equal(res.pred_classes.cpu(), wc) and torch.equal(res.scores.cpu(), ws)
        assert torch.equal(res.pred_boxes.tensor.cpu(), wb)
    assert len(out) == 2 and all(o["instances"].image_size == (x["height"], x["width"]) for o, x in zip(out, batch))


def test_tta_with_a_class_specific_head(F, standard_model):
    """One two-view case (one size, with its mirror image): impl="device" == impl="host" bit for bit through the same calls."""
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.modeling import GeneralizedRCNNWithTTA

    cfg, model, _ = standard_model
    model.eval()
    x = make_synthetic_batch(1, start_index=0, height=96, width=128, device=DEV)[0]
    batch = [{"image": x["image"], "height": 144, "width": 192}]
    with torch.no_grad():
        host = GeneralizedRCNNWithTTA(cfg, model, impl="host")
        assert len(host.tta_mapper(batch[0])) == 2
        want = host(batch)
        got = GeneralizedRCNNWithTTA(cfg, model, impl="device", batch_size=2)(batch)
    a, b = want[0]["instances"], got[0]["instances"]
    assert len(a) >= 1 and a.image_size == b.image_size == (144, 192)
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores)
    assert torch.equal(a.pred_classes, b.pred_classes) and torch.equal(a.pred_masks, b.pred_masks)
