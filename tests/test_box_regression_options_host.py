"""The RPN's localisation loss options and class-specific box regression on the host: the torch definitions of
u2seg_amd/modeling/box_losses.py against what the reference itself computed (tests/golden/box_regression_golden.npz,
generator: tests/golden/make_box_regression_fixture.py), the options through from_config, the state-dict shapes of the shipped
configs and of a class-specific head, the checkpointer on both layouts of bbox_pred, and the float64 side of
tests/test_gpu_box_regression_options.py on the CPU: the drawn inputs of tests/box_regression_cases.py must stay within the
GPU test's ambiguity cap by the reference alone.  No GPU."""
import json
import math
import os
import zlib

import numpy as np
import pytest
import torch

from tests import box_loss_refs as refs
from tests import box_regression_cases as cases
from tests.test_box_loss_options_host import close, small_dataset   # (close: the fixture tolerance RTOL of that file)
from u2seg_amd.modeling import box_losses as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG_DIR = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation")
FORMS = [("diou", 0.0, "diou"), ("ciou", 0.0, "ciou"), ("smooth_l1", None, "smooth_l1"), ("smooth_l1", 0.0, "l1")]


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(GOLDEN, "box_regression_golden.npz")).items()}


def cfg_with(opts=(), name="u2seg_R50_800.yaml"):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CFG_DIR, name))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


# ---- the definitions against the reference's arrays ----------------------------------------------------------
@pytest.mark.parametrize("wi", [0, 1])
@pytest.mark.parametrize("kind,beta,name", FORMS)
def test_rpn_definition_reproduces_the_reference(gold, kind, beta, name, wi):
    a = gold
    beta = float(a["beta"]) if beta is None else beta
    weights = tuple(a["rpn_weights"][wi].tolist())
    norm = float(a["rpn_batch_per_image"]) * a["rpn_labels"].shape[0]
    o = a["rpn_obj"].clone().requires_grad_(True)
    d = a["rpn_deltas"].clone().requires_grad_(True)
    loc = BL.rpn_box_reg_loss(kind, a["rpn_labels"], a["rpn_match"], a["rpn_gt"], a["rpn_anchors"], d, weights, beta,
                              float(a["scale_clamp"])) / norm
    cls = BL.rpn_objectness_loss(a["rpn_labels"], o) / norm
    loc.backward()
    cls.backward()
    key = "rpn_w%d_%s" % (wi, name)
    assert close(loc.detach(), a[key + "_loc"]) and close(d.grad, a[key + "_ddeltas"])
    assert close(cls.detach(), a[key + "_cls"]) and close(o.grad, a[key + "_dobj"])
    assert float(d.grad[a["rpn_labels"] != 1].abs().max()) == 0.0     # labels 0 and -1, the whole image without ground truth
    assert int((a["rpn_labels"][1] == 1).sum()) == 0 and float(a["rpn_gt"][1].abs().max()) == 0.0
    if kind != "smooth_l1":                                            # a dw above the clamp passes no gradient
        over = (a["rpn_deltas"][..., 2] / weights[2] > float(a["scale_clamp"])) & (a["rpn_labels"] == 1)
        assert int(over.sum()) >= 1 and float(d.grad[..., 2][over].abs().max()) == 0.0


@pytest.mark.parametrize("kind,beta,name", FORMS)
def test_class_specific_definition_reproduces_the_reference(gold, kind, beta, name):
    a = gold
    beta = float(a["beta"]) if beta is None else beta
    k, weights = int(a["head_num_classes"]), tuple(a["head_weights"].tolist())
    d = a["head_deltas"].clone().requires_grad_(True)
    loss = BL.box_reg_loss(kind, d, a["head_prop"], a["head_gtb"], a["head_classes"], k, weights, beta, float(a["scale_clamp"]),
                           cls_agnostic=False) / d.shape[0]
    loss.backward()
    assert close(loss.detach(), a["head_%s_loss" % name]) and close(d.grad, a["head_%s_grad" % name])
    own = torch.zeros_like(d, dtype=torch.bool)
    fg = a["head_classes"] < k
    own[fg] = own[fg].scatter(1, cases.cls_columns(a["head_classes"], k)[fg], True)
    assert float(d.grad[~own].abs().max()) == 0.0 and int(own.sum()) == 4 * int(fg.sum())


def test_class_specific_decode_reproduces_the_reference(gold):
    a = gold
    k, weights = int(a["head_num_classes"]), tuple(a["head_weights"].tolist())
    got = BL.predict_boxes_cls(a["head_deltas"], a["head_prop"], k, weights, float(a["scale_clamp"]))
    assert got.shape == (a["head_prop"].shape[0], 4 * k) and close(got, a["head_pred_boxes"])


def test_golden_file_holds_arrays_only():
    with np.load(os.path.join(GOLDEN, "box_regression_golden.npz"), allow_pickle=False) as f:
        assert all(f[k].dtype.kind in "fiu" for k in f.files)


# ---- options and construction ------------------------------------------------------------------------------
def rpn_with(opts):
    from u2seg_amd.layers import ShapeSpec
    from u2seg_amd.modeling.rpn import RPN

    shapes = {"p%d" % (i + 2): ShapeSpec(channels=256, stride=4 << i) for i in range(5)}
    return RPN(cfg_with(opts), shapes)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_every_rpn_option_builds(kind):
    rpn = rpn_with(["MODEL.RPN.BBOX_REG_LOSS_TYPE", kind, "MODEL.RPN.SMOOTH_L1_BETA", "0.5",
                    "MODEL.RPN.BBOX_REG_WEIGHTS", "(10.0, 10.0, 5.0, 5.0)"])
    assert rpn.box_reg_loss_type == kind and rpn.smooth_l1_beta == 0.5 and rpn.bbox_reg_weights == (10.0, 10.0, 5.0, 5.0)


def test_rpn_refuses_what_it_cannot_serve():
    with pytest.raises(ValueError, match="eiou"):
        rpn_with(["MODEL.RPN.BBOX_REG_LOSS_TYPE", "eiou"])
    for bad in ("(1.0, 1.0, 0.0, 1.0)", "(1.0, -2.0, 1.0, 1.0)", "(1.0, 1.0, 1.0)"):
        with pytest.raises(ValueError, match="BBOX_REG_WEIGHTS"):
            rpn_with(["MODEL.RPN.BBOX_REG_WEIGHTS", bad])
    with pytest.raises(ValueError, match="SMOOTH_L1_BETA"):
        rpn_with(["MODEL.RPN.SMOOTH_L1_BETA", "-0.5"])
    d = rpn_with([])
    assert (d.box_reg_loss_type, d.smooth_l1_beta, d.bbox_reg_weights) == ("smooth_l1", 0.0, (1.0, 1.0, 1.0, 1.0))


def test_rpn_options_reach_the_loss_call(monkeypatch):
    """RPN.losses hands its options to F.rpn_losses; the defaults are what it has always been called with."""
    from u2seg_amd.modeling import rpn as rpn_mod

    seen = []

    class Stand:
        def rpn_losses(self, *a):
            seen.append(a[8:])
            return torch.zeros(()), torch.zeros(())

    monkeypatch.setattr(rpn_mod, "F", Stand())
    monkeypatch.setattr(rpn_mod, "step_counters", lambda: None)
    labels = torch.zeros((2, 5), dtype=torch.int8)
    rpn_with(["MODEL.RPN.BBOX_REG_LOSS_TYPE", "ciou", "MODEL.RPN.BBOX_REG_WEIGHTS", "(2.0, 2.0, 1.0, 1.0)"]).losses(
        [], [], [], labels, None, None)
    rpn_with([]).losses([], [], [], labels, None, None)
    assert seen[0] == ("ciou", 0.0, (2.0, 2.0, 1.0, 1.0), math.log(1000.0 / 16))
    assert seen[1][:3] == ("smooth_l1", 0.0, (1.0, 1.0, 1.0, 1.0))


def test_shipped_configs_keep_their_state_dicts():
    from u2seg_amd.modeling import build_model

    with open(os.path.join(GOLDEN, "model_small.json")) as f:
        fx = json.load(f)
    sd = build_model(cfg_with()).state_dict()
    assert len(sd) == fx["num_state_entries"] and zlib.crc32("\n".join(sd.keys()).encode()) == fx["state_dict_keys_crc32"]
    assert sum(v.numel() for k, v in build_model(cfg_with()).named_parameters()) == fx["num_params"]
    for stage in range(3):
        assert tuple(sd["roi_heads.box_predictor.%d.bbox_pred.weight" % stage].shape) == (4, 1024)
    assert sum(p.numel() for p in build_model(cfg_with(name="u2seg_R50_300.yaml")).parameters()) == 74400554
    small_dataset("box_loss_options_small")
    fed = build_model(cfg_with(["DATASETS.TRAIN", "('box_loss_options_small',)"], "u2seg_R50_800_fedloss.yaml")).state_dict()
    assert len(fed) == 434 and [k for k in fed if k not in sd] == [
        "roi_heads.box_predictor.%d.fed_loss_cls_weights" % s for s in range(3)]
    assert all(tuple(fed[k].shape) == tuple(sd[k].shape) for k in sd)


@pytest.fixture(scope="module")
def standard_model():
    from u2seg_amd.modeling import build_model

    return build_model(cfg_with(name="u2seg_R50_800_standard_heads.yaml"))


def test_standard_heads_config_builds(standard_model):
    cfg = cfg_with(name="u2seg_R50_800_standard_heads.yaml")
    assert cfg.MODEL.ROI_HEADS.NAME == "StandardROIHeads" and not cfg.MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG
    assert cfg.MODEL.RPN.BBOX_REG_LOSS_TYPE == "giou" and cfg.MODEL.ROI_HEADS.NUM_CLASSES == 800
    sd = standard_model.state_dict()
    assert tuple(sd["roi_heads.box_predictor.bbox_pred.weight"].shape) == (3200, 1024)      # the reference's key, 4 K rows
    assert tuple(sd["roi_heads.box_predictor.bbox_pred.bias"].shape) == (3200,)
    assert tuple(sd["roi_heads.box_predictor.cls_score.weight"].shape) == (801, 1024)
    assert standard_model.proposal_generator.box_reg_loss_type == "giou"
    assert not standard_model.roi_heads.box_predictor.cls_agnostic_bbox_reg


def test_cascade_and_pred_box_training_stay_refused():
    from u2seg_amd.modeling import build_model

    with pytest.raises(AssertionError, match="class-agnostic"):
        build_model(cfg_with(["MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG", "False"]))
    with pytest.raises(AssertionError):
        build_model(cfg_with(["MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES", "True"], "u2seg_R50_800_standard_heads.yaml"))


class HostFunctional(refs.TorchLossFunctional):
    """TorchLossFunctional with the two calls a class-specific head adds."""

    def box_reg_loss_cls(self, kind, pred, proposals, gt_boxes, labels, bg_label, weights, normalizer, beta=0.0,
                         scale_clamp=cases.CLAMP):
        self.calls.append("box_reg_loss_cls:" + kind)
        return BL.box_reg_loss(kind, pred, proposals, gt_boxes, labels, bg_label, weights, beta, scale_clamp, False) / normalizer

    def apply_deltas_cls(self, src, deltas, num_classes, weights, clamp=cases.CLAMP):
        self.calls.append("apply_deltas_cls")
        return BL.predict_boxes_cls(deltas, src, num_classes, weights, clamp)


@pytest.mark.parametrize("kind,beta", [("smooth_l1", 0.0), ("smooth_l1", 0.5), ("giou", 0.0), ("ciou", 0.0)])
def test_class_specific_head_on_the_host(monkeypatch, kind, beta):
    """cls_agnostic_bbox_reg=False through FastRCNNOutputLayers: the loss reads the label's columns and predict_boxes returns
    [R_i, 4 K] per image and [B, S, 4 K] stacked."""
    from u2seg_amd.layers import ShapeSpec
    from u2seg_amd.modeling import roi_heads
    from u2seg_amd.modeling.roi_heads import FastRCNNOutputLayers
    from u2seg_amd.structures import Boxes, Instances

    k, r = 12, 24
    layer = FastRCNNOutputLayers(ShapeSpec(channels=16), box2box_weights=cases.HEAD_WEIGHTS, num_classes=k,
                                 cls_agnostic_bbox_reg=False, box_reg_loss_type=kind, smooth_l1_beta=beta)
    assert tuple(layer.bbox_pred.weight.shape) == (4 * k, 16)
    pred, prop, gt, lab = cases.cls_case(r, k, 64, cases.HEAD_WEIGHTS, 5)
    lab[::2] = torch.arange(r // 2) % k
    scores = torch.zeros(r, 32)
    halves = []
    for i in range(2):
        inst = Instances((900, 1400))
        sl = slice(i * r // 2, (i + 1) * r // 2)
        inst.proposal_boxes, inst.gt_boxes, inst.gt_classes = Boxes(prop[sl]), Boxes(gt[sl]), lab[sl]
        halves.append(inst)
    stand = HostFunctional()
    monkeypatch.setattr(roi_heads, "F", stand)
    out = layer.losses((scores, pred.float()), halves)
    want = BL.box_reg_loss(kind, pred.float(), prop, gt, lab, k, cases.HEAD_WEIGHTS, beta, cases.CLAMP, cls_agnostic=False) / r
    assert close(out["loss_box_reg"], want) and stand.calls == ["softmax_cross_entropy", "box_reg_loss_cls:" + kind]
    boxes = layer.predict_boxes((scores, pred.float()), halves)
    assert [tuple(b.shape) for b in boxes] == [(r // 2, 4 * k)] * 2
    stacked = layer.predict_boxes((scores, pred.float()), halves, stacked=True)
    assert tuple(stacked.shape) == (2, r // 2, 4 * k) and torch.equal(stacked.reshape(r, -1), torch.cat(boxes))
    # class c of row i is apply_deltas of that class's four columns
    c = 7
    one = BL.apply_deltas(pred.float()[:, 4 * c:4 * c + 4], prop, cases.HEAD_WEIGHTS, cases.CLAMP)
    assert torch.equal(torch.cat(boxes)[:, 4 * c:4 * c + 4], one)
    empty = Instances((900, 1400))
    empty.proposal_boxes = Boxes(torch.zeros(0, 4))
    assert tuple(layer.predict_boxes((scores[:0], pred[:0].float()), [empty])[0].shape) == (0, 4 * k)


# ---- checkpoints ----------------------------------------------------------------------------------------------
def test_checkpoints_of_both_layouts(standard_model, tmp_path):
    from u2seg_amd.checkpoint import DetectionCheckpointer

    key = "roi_heads.box_predictor.bbox_pred."
    g = torch.Generator().manual_seed(3)
    specific = {key + "weight": torch.randn(3200, 1024, generator=g), key + "bias": torch.randn(3200, generator=g)}
    path = str(tmp_path / "specific.pth")
    torch.save({"model": specific}, path)
    ck = DetectionCheckpointer(standard_model, save_to_disk=False)
    ck.load(path)
    assert ck.last_incompatible.incorrect_shapes == []
    sd = standard_model.state_dict()
    assert torch.equal(sd[key + "weight"], specific[key + "weight"]) and torch.equal(sd[key + "bias"], specific[key + "bias"])
    # a class-agnostic file into the class-specific model: reported as a shape mismatch and skipped
    agnostic = {key + "weight": torch.ones(4, 1024), key + "bias": torch.ones(4)}
    path = str(tmp_path / "agnostic.pth")
    torch.save({"model": agnostic}, path)
    ck.load(path)
    assert sorted(ck.last_incompatible.incorrect_shapes) == [(key + "bias", (4,), (3200,)), (key + "weight", (4, 1024), (3200, 1024))]
    assert torch.equal(standard_model.state_dict()[key + "weight"], specific[key + "weight"])        # untouched


# ---- the ambiguity cap by the reference alone ---------------------------------------------------------------------
def ambiguous_free_rows(pred, prop, gt, lab, weights, planted):
    """(free ambiguous rows, foreground rows) as check_box of tests/test_gpu_box_loss_options.py counts them."""
    from tests.test_gpu_box_loss_options import box_expect

    fg = (lab >= 0) & (lab < 800)
    n_fg = int(fg.sum())
    if n_fg == 0:
        return 0, 0
    worst = 0
    for kind in ("giou", "diou", "ciou"):
        free = box_expect(kind, pred, prop, gt, fg, weights, 1.0)["amb"].clone()
        free[: min(planted, n_fg)] = False
        worst = max(worst, int(free.sum()))
    return worst, n_fg


@pytest.mark.parametrize("wi", [0, 1])
def test_rpn_inputs_stay_within_the_ambiguity_cap(wi):
    """At most 1 % of the non-planted positives of every level may be ambiguous (branch_margin within four decode errors)."""
    from tests.test_gpu_box_regression_options import RPN_SEED

    case = cases.rpn_case(cases.RPN_WEIGHTS[wi], RPN_SEED + wi, empty_level=bool(wi))
    for lvl in range(len(cases.RPN_LEVELS)):
        pred, prop, gt, lab, planted = cases.rpn_level_rows(case, lvl)
        free, n_fg = ambiguous_free_rows(pred, prop, gt, lab, case["weights"], planted)
        assert free <= 0.01 * n_fg, (lvl, free, n_fg)
        assert (n_fg == 0) == (lvl == 1 and bool(wi))                # the level without a positive


def test_head_inputs_stay_within_the_ambiguity_cap():
    from tests.test_gpu_box_regression_options import CLS_SHAPES, cls_seed

    for R, K, LP in CLS_SHAPES:
        pred, prop, gt, lab = cases.cls_case(R, K, LP, cases.HEAD_WEIGHTS, cls_seed(R, K))
        own, lab800 = cases.cls_gathered(pred, lab, K)
        free, n_fg = ambiguous_free_rows(own, prop, gt, lab800, cases.HEAD_WEIGHTS, cases.N_PLANTED if R >= 65 else 0)
        assert free <= 0.01 * n_fg and n_fg >= 1, (R, K, free, n_fg)
