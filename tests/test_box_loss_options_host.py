"""The box heads' loss options on the host: the torch definitions of u2seg_amd/modeling/box_losses.py against what the
reference itself computed (tests/golden/box_loss_golden.*, generator: tests/golden/make_box_loss_fixture.py), the pinned GIoU
against its formula in float64, the federated class mask by its properties, the class weights against a hand count of
tests/golden/data_small, and the six config keys through from_config.  No GPU: where the ROI heads would launch a kernel the
tests put the torch definitions in its place (tests/box_loss_refs.py:TorchLossFunctional)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import box_loss_refs as refs
from u2seg_amd.modeling import box_losses as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
RTOL = 1e-6   # fp32 outputs of fp32 inputs through the same op sequence


@pytest.fixture(scope="module")
def gold():
    arrays = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "box_loss_golden.npz")).items()}
    with open(os.path.join(GOLDEN, "box_loss_golden.json")) as f:
        return arrays, json.load(f)


def close(got, want):
    return torch.allclose(got, want, rtol=RTOL)


# ---- the definitions against the reference's arrays ----------------------------------------------------
@pytest.mark.parametrize("kind", ["diou", "ciou"])
def test_iou_losses_reproduce_the_reference(gold, kind):
    a, _ = gold
    b1 = a["b1"].clone().requires_grad_(True)
    rows = {"diou": BL.diou_loss, "ciou": BL.ciou_loss}[kind](b1, a["b2"])
    rows.sum().backward()
    assert close(rows.detach(), a[kind + "_rows"]) and close(b1.grad, a[kind + "_rows_grad"])
    assert float(a[kind + "_rows"][0]) > 1.0            # the disjoint pair: no intersection, a distance term


def test_sigmoid_ce_reproduces_the_reference(gold):
    a, meta = gold
    k = meta["num_classes"]
    z = a["logits"].clone().requires_grad_(True)
    loss = BL.sigmoid_cross_entropy(z, a["gt_classes"], k)
    loss.backward()
    assert close(loss.detach(), a["sigmoid_loss"]) and close(z.grad, a["sigmoid_grad"])
    assert float(z.grad[:, k].abs().max()) == 0.0       # the background column takes no part
    # pad columns are ignored, an empty input gives 0
    padded = torch.cat([a["logits"], torch.full((a["logits"].shape[0], 3), 1e4)], 1)
    assert close(BL.sigmoid_cross_entropy(padded, a["gt_classes"], k), a["sigmoid_loss"])
    assert float(BL.sigmoid_cross_entropy(torch.zeros(0, k + 1), torch.zeros(0, dtype=torch.int64), k)) == 0.0


def test_fed_mask_and_loss_reproduce_the_reference(gold):
    a, meta = gold
    k, nf = meta["num_classes"], meta["fed_loss_num_classes"]
    mask = BL.fed_loss_classes_mask(a["gt_classes"], nf, k, a["fed_weight"], extra_classes=a["fed_extra"])
    assert torch.equal(mask, a["fed_mask"])
    z = a["logits"].clone().requires_grad_(True)
    loss = BL.sigmoid_cross_entropy(z, a["gt_classes"], k, mask)
    loss.backward()
    assert close(loss.detach(), a["fed_loss"]) and close(z.grad, a["fed_grad"])
    assert float(a["fed_loss"]) < float(a["sigmoid_loss"])


@pytest.mark.parametrize("kind", ["diou", "ciou", "smooth_l1"])
def test_box_reg_loss_reproduces_the_reference(gold, kind):
    a, meta = gold
    d = a["deltas"].clone().requires_grad_(True)
    beta = meta["smooth_l1_beta"] if kind == "smooth_l1" else 0.0
    loss = BL.box_reg_loss(kind, d, a["prop"], a["gtb"], a["gt_classes"], meta["num_classes"], meta["weights"], beta,
                           meta["scale_clamp"]) / max(meta["rows"], 1)
    loss.backward()
    assert close(loss.detach(), a["box_%s_loss" % kind]) and close(d.grad, a["box_%s_grad" % kind])
    bg = a["gt_classes"] == meta["num_classes"]
    assert float(d.grad[bg].abs().max()) == 0.0
    if kind != "smooth_l1":                             # the planted row: dw above the clamp passes no gradient
        row = int(torch.nonzero(~bg)[0])
        assert float(a["deltas"][row, 2]) / meta["weights"][2] > meta["scale_clamp"] and float(d.grad[row, 2]) == 0.0


def test_smooth_l1_beta_zero_is_l1(gold):
    a, meta = gold
    k, w = meta["num_classes"], meta["weights"]
    fg = a["gt_classes"] < k
    want = (a["deltas"][fg] - BL.get_deltas(a["prop"][fg], a["gtb"][fg], w)).abs().sum()
    assert close(BL.box_reg_loss("smooth_l1", a["deltas"], a["prop"], a["gtb"], a["gt_classes"], k, w, 0.0), want)


def test_unknown_box_loss_type_is_a_value_error(gold):
    a, meta = gold
    with pytest.raises(ValueError, match="eiou"):
        BL.box_reg_loss("eiou", a["deltas"], a["prop"], a["gtb"], a["gt_classes"], meta["num_classes"], meta["weights"])


# ---- GIoU: the pinned formula ----------------------------------------------------------------------------
def test_giou_is_the_pinned_formula(gold):
    a, _ = gold
    b1, b2 = a["b1"].to(torch.float64), a["b2"].to(torch.float64)
    x1, y1, x2, y2 = b1.unbind(1)
    x1g, y1g, x2g, y2g = b2.unbind(1)
    iw = (torch.minimum(x2, x2g) - torch.maximum(x1, x1g))
    ih = (torch.minimum(y2, y2g) - torch.maximum(y1, y1g))
    inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
    union = (x2 - x1) * (y2 - y1) + (x2g - x1g) * (y2g - y1g) - inter
    c = (torch.maximum(x2, x2g) - torch.minimum(x1, x1g)) * (torch.maximum(y2, y2g) - torch.minimum(y1, y1g))
    want = 1 - inter / (union + 1e-7) + (c - union) / (c + 1e-7)
    got = BL.giou_loss(b1, b2)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-12, atol=0)
    assert torch.allclose(refs.iou_loss_rows("giou", b1, b2), want, rtol=1e-12, atol=0)
    assert 1.0 < float(got[0]) <= 2.0                   # disjoint: no intersection, most of the enclosing box empty
    # coinciding boxes: C == U, what is left is DIoU's IoU term (centres coincide as well)
    same = BL.giou_loss(b2, b2)
    assert torch.equal(same, BL.diou_loss(b2, b2)) and float(same.abs().max()) < 1e-6
    # fp32, as the heads use it
    assert torch.allclose(BL.giou_loss(a["b1"], a["b2"]).double(), want, rtol=1e-4, atol=1e-6)


# ---- the federated class mask ----------------------------------------------------------------------------
def test_fed_mask_properties():
    k = 40
    g = torch.Generator().manual_seed(3)
    weight = torch.rand(k, generator=g) + 0.1
    weight[[1, 7, 30]] = 0
    for trial in range(20):
        torch.manual_seed(100 + trial)
        n_present = 1 + trial % 9
        classes = torch.randperm(k, generator=g)[:n_present]
        gt = classes[torch.randint(0, n_present, (50,), generator=g)]
        gt[:n_present] = classes
        with_bg = trial % 2 == 0
        if with_bg:
            gt[-5:] = k
        for num_fed in (3, 8, 20):
            mask = BL.fed_loss_classes_mask(gt, num_fed, k, weight)
            assert mask.shape == (k,) and mask.dtype == torch.float32 and set(mask.tolist()) <= {0.0, 1.0}
            assert bool((mask[classes] == 1).all())                                   # every present class
            # the reference's count: max(num_fed, distinct labels), the background being one of them where it occurs
            assert int(mask.sum()) + with_bg == max(num_fed, n_present + with_bg)
            drawn = mask.clone()
            drawn[classes] = 0
            assert float((drawn * (weight == 0)).sum()) == 0.0                        # never a zero-weight class
    # no class is drawn twice and the draw follows the weights: one heavy class is (almost) always among two extras
    weight = torch.full((k,), 1e-3)
    weight[11] = 1.0
    hits = sum(int(BL.fed_loss_classes_mask(torch.tensor([0, 1, k]), 5, k, weight)[11]) for _ in range(50))
    assert hits >= 45


def test_fed_mask_where_the_reference_would_raise():
    k = 6
    gt = torch.tensor([0, 0, 2, k])
    weight = torch.tensor([1.0, 0.0, 1.0, 0.5, 0.0, 0.0])                             # one candidate (class 3) for two places
    assert BL.fed_loss_classes_mask(gt, 5, k, weight).tolist() == [1, 0, 1, 1, 0, 0]
    assert BL.fed_loss_classes_mask(gt, 50, k, torch.ones(k)).tolist() == [1] * k     # num_fed > K: every class
    assert BL.fed_loss_classes_mask(gt, 5, k, torch.zeros(k)).tolist() == [1, 0, 1, 0, 0, 0]
    assert BL.fed_loss_classes_mask(gt, 2, k, torch.ones(k)).tolist() == [1, 0, 1, 0, 0, 0]   # enough present: nothing added


# ---- class weights from the dataset ----------------------------------------------------------------------
def small_dataset(name):
    from u2seg_amd.data.catalog import DatasetCatalog
    from u2seg_amd.data.datasets import load_coco_json

    root = os.path.join(GOLDEN, "data_small")
    js = os.path.join(root, "prepare_ours", "u2seg_annotations", "ins_annotations", "cocotrain_800.json")
    if name not in DatasetCatalog:
        DatasetCatalog.register(name, lambda: load_coco_json(js, os.path.join(root, "coco", "train2017"), name))
    return js


def test_fed_loss_cls_weights_count_images_per_class():
    from u2seg_amd.data.catalog import MetadataCatalog
    from u2seg_amd.data.detection_utils import get_fed_loss_cls_weights

    js = small_dataset("box_loss_options_small")
    # the hand count of that json: (image, category, iscrowd) = (10, 5, 0) (10, 17, 0) (10, 800, 1) (20, 17, 0) (20, 800, 0)
    # (30, 800, 1) (40, 333, 0) (40, 5, 0): categories 5 and 17 in two images each, 333 and 800 (not a crowd) in one
    with open(js) as f:
        anns = json.load(f)["annotations"]
    assert sorted((a["image_id"], a["category_id"], a["iscrowd"]) for a in anns) == [
        (10, 5, 0), (10, 17, 0), (10, 800, 1), (20, 17, 0), (20, 800, 0), (30, 800, 1), (40, 5, 0), (40, 333, 0)]
    want = torch.zeros(800)
    want[[4, 16]] = 2.0
    want[[332, 799]] = 1.0
    assert torch.equal(get_fed_loss_cls_weights("box_loss_options_small", 1.0), want)
    assert torch.equal(get_fed_loss_cls_weights(["box_loss_options_small"], 0.5), want ** 0.5)
    stored = MetadataCatalog.get("box_loss_options_small").class_image_count
    assert [c["id"] for c in stored] == list(range(1, 801)) and stored[4] == {"id": 5, "image_count": 2}
    # a field that is there is used as it is (the reference's behaviour)
    MetadataCatalog.get("box_loss_options_given").class_image_count = [{"id": 2, "image_count": 9}, {"id": 1, "image_count": 4}]
    assert get_fed_loss_cls_weights("box_loss_options_given", 0.5).tolist() == [2.0, 3.0]


# ---- from_config ---------------------------------------------------------------------------------------
def cfg_with(opts=()):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def predictor(opts=()):
    from u2seg_amd.layers import ShapeSpec
    from u2seg_amd.modeling.roi_heads import FastRCNNOutputLayers

    return FastRCNNOutputLayers(cfg_with(opts), ShapeSpec(channels=16))


def fixed_predictions(k=800, r=24, lp=832):
    g = torch.Generator().manual_seed(11)
    scores = torch.randn(r, lp, generator=g) * 2
    scores[:, k + 1:] = 1e4
    deltas = torch.zeros(r, 32)
    deltas[:, :4] = torch.randn(r, 4, generator=g) * 0.5
    xy = torch.rand(r, 2, generator=g) * 200
    prop = torch.cat([xy, xy + 10 + torch.rand(r, 2, generator=g) * 80], 1)
    gtb = prop + torch.randn(r, 4, generator=g) * 3
    gt = torch.randint(0, k, (r,), generator=g)
    gt[::2] = k
    from u2seg_amd.structures import Boxes, Instances

    inst = Instances((300, 300))
    inst.proposal_boxes, inst.gt_boxes, inst.gt_classes = Boxes(prop), Boxes(gtb), gt
    return (scores, deltas), [inst], (prop, gtb, gt)


def losses_on_host(pred, monkeypatch, predictions, proposals):
    from u2seg_amd.modeling import roi_heads

    stand_in = refs.TorchLossFunctional()
    monkeypatch.setattr(roi_heads, "F", stand_in)
    return pred.losses(predictions, proposals), stand_in.calls


def test_use_sigmoid_ce_reaches_the_loss(monkeypatch):
    """MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE True: loss_cls on fixed predictions is the sigmoid definition, not softmax."""
    predictions, proposals, (_, _, gt) = fixed_predictions()
    out, calls = losses_on_host(predictor(["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"]), monkeypatch, predictions, proposals)
    want = BL.sigmoid_cross_entropy(predictions[0], gt, 800)
    softmax = TF.cross_entropy(predictions[0][:, :801], gt)
    assert sorted(out) == ["loss_box_reg", "loss_cls"]
    assert close(out["loss_cls"], want) and not torch.allclose(out["loss_cls"], softmax, rtol=1e-2)
    assert calls == ["sigmoid_cross_entropy", "box_reg_l1_loss"]
    # the default keeps softmax and L1
    out, calls = losses_on_host(predictor(), monkeypatch, predictions, proposals)
    assert close(out["loss_cls"], softmax) and calls == ["softmax_cross_entropy", "box_reg_l1_loss"]


def test_predict_probs_follow_the_loss():
    predictions, proposals, _ = fixed_predictions()
    sig = predictor(["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"]).predict_probs(predictions, proposals, split=False)
    assert sig.shape == (24, 801) and torch.equal(sig, predictions[0][:, :801].sigmoid())
    soft = predictor().predict_probs(predictions, proposals, split=False)
    assert torch.equal(soft, torch.softmax(predictions[0][:, :801], dim=-1))


@pytest.mark.parametrize("kind,beta", [("giou", 0.0), ("diou", 0.0), ("ciou", 0.0), ("smooth_l1", 0.25)])
def test_box_reg_loss_type_reaches_the_loss(monkeypatch, kind, beta):
    predictions, proposals, (prop, gtb, gt) = fixed_predictions()
    pred = predictor(["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", kind, "MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA", str(beta),
                      "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT", "2.0"])
    out, calls = losses_on_host(pred, monkeypatch, predictions, proposals)
    want = 2.0 * BL.box_reg_loss(kind, predictions[1], prop, gtb, gt, 800, (10.0, 10.0, 5.0, 5.0), beta) / 24
    assert close(out["loss_box_reg"], want) and calls == ["softmax_cross_entropy", "box_reg_loss:" + kind]


def test_unknown_loss_type_raises_value_error():
    with pytest.raises(ValueError, match="eiou"):
        predictor(["MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "eiou"])


def test_fed_loss_needs_sigmoid_ce():
    with pytest.raises(AssertionError, match="sigmoid"):
        predictor(["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", "True"])


def test_state_dict_keys_and_cascade_stages(monkeypatch):
    from u2seg_amd.modeling import build_model

    assert len(build_model(cfg_with()).state_dict()) == 431
    small_dataset("box_loss_options_small")
    opts = ["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True", "MODEL.ROI_BOX_HEAD.USE_FED_LOSS", "True",
            "MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE", "giou", "MODEL.ROI_BOX_HEAD.FED_LOSS_NUM_CLASSES", "7",
            "DATASETS.TRAIN", "('box_loss_options_small',)"]
    model = build_model(cfg_with(opts))
    sd = model.state_dict()
    new = sorted(k for k in sd if k.endswith("fed_loss_cls_weights"))
    assert len(sd) == 434 and new == ["roi_heads.box_predictor.%d.fed_loss_cls_weights" % s for s in range(3)]
    stages = model.roi_heads.box_predictor
    assert [p.box2box_weights for p in stages] == [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)]
    for p in stages:
        assert p.use_sigmoid_ce and p.use_fed_loss and p.box_reg_loss_type == "giou" and p.fed_loss_num_classes == 7
        assert p.fed_loss_cls_weights.nonzero().flatten().tolist() == [4, 16, 332, 799]      # image_count ** 0.5
    # the federated mask reaches the loss: with 7 federated classes most of the 800 columns drop out
    predictions, proposals, (_, _, gt) = fixed_predictions()
    out, calls = losses_on_host(stages[1], monkeypatch, predictions, proposals)
    assert calls == ["sigmoid_cross_entropy", "box_reg_loss:giou"]
    assert float(out["loss_cls"]) < 0.1 * float(BL.sigmoid_cross_entropy(predictions[0], gt, 800))


def test_fedloss_config_file():
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(os.path.dirname(CFG), "u2seg_R50_800_fedloss.yaml"))
    head = cfg.MODEL.ROI_BOX_HEAD
    assert head.USE_SIGMOID_CE and head.USE_FED_LOSS and head.BBOX_REG_LOSS_TYPE == "giou"
    assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == 800 and cfg.MODEL.ROI_HEADS.NAME == "CascadeROIHeads"
