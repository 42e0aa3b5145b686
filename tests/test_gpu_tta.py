"""Test-time augmentation on the device (csrc/tta.hip, modeling/test_time_augmentation.py): the three
kernels against their host definitions bit for bit, the views of one source, inference on given boxes, the merge on hand-made
detections (here and not on the CPU: fast_rcnn_inference ends in the HIP NMS kernel), impl="device" against impl="host" end to
end, and the wiring in tools/train_net.py."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import tta_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tta():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.modeling import test_time_augmentation

    _hip.load()
    return test_time_augmentation


def _descriptors(tta, inverse):
    views = C.box_views()
    d = [tta.view_descriptor(t, inverse=inverse) for _, t in views]
    desc = torch.from_numpy(np.stack([x for x, _ in d])).to(DEV)
    flip = torch.tensor([f for _, f in d], dtype=torch.int32, device=DEV)
    image = torch.tensor([im for im, _ in views], dtype=torch.int32, device=DEV)
    return desc, flip, image


# ---- 1. the box kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257])
def test_boxes_to_original_equals_the_float32_definition(tta, n):
    """u2_tta_boxes_to_original == apply_box_f32(inverse) + Boxes.clip + the candidate rule, torch.equal (NaNs in the same
    places): five views of two images with different clip sizes, flips with and without a pre-resize, a view without rows,
    boxes beyond the canvas, a NaN and an inf row, scores at float32(1e-8) exactly (dropped) and the next float (kept)."""
    boxes, scores = C.detections_case(n)
    counts = [len(b) for b in boxes]
    assert sum(counts) == n and counts[2] == 0
    want_b, want_c = C.to_original_expected(boxes, scores)
    desc, flip, image = _descriptors(tta, inverse=True)
    clip = torch.tensor([[w, h] for h, w in C.BOX_CLIP], dtype=torch.float32, device=DEV)
    row_view = torch.from_numpy(np.repeat(np.arange(5), counts).astype(np.int32)).to(DEV)
    got_b, got_c = tta.tta_boxes_to_original(torch.from_numpy(np.concatenate(boxes)).to(DEV),
                                             torch.from_numpy(np.concatenate(scores)).to(DEV), row_view, desc, flip, image, clip)
    torch.cuda.synchronize()
    assert got_b.shape == (n, 4) and got_c.shape == (n,) and got_c.dtype == torch.uint8
    assert C.nan_equal(got_b.cpu(), torch.from_numpy(want_b).reshape(n, 4))
    assert torch.equal(got_c.cpu().bool(), torch.from_numpy(want_c))
    if n == 257:
        s = np.concatenate(scores)
        at, above = np.flatnonzero(s == C.THRESH), np.flatnonzero(s == np.nextafter(C.THRESH, np.float32(1)))
        assert len(at) >= 3 and len(above) >= 3 and not want_c[at].any()
        assert want_c[above].sum() >= 1 and 0 < want_c.sum() < n
        assert np.isnan(want_b).any() and (want_b[~np.isnan(want_b)] == 0).any()   # a NaN row survives the clip, the clip bites


@pytest.mark.parametrize("n", [0, 1, 257])
def test_boxes_to_views_equals_the_float32_definition(tta, n):
    """u2_tta_boxes_to_views == apply_box_f32 per view, torch.equal, not clipped: image 0 with n rows, image 1 with 5."""
    rs = np.random.RandomState(20 + n)
    per_image = [C.random_boxes(rs, r, h, w) for r, (h, w) in zip((n, 5), C.BOX_CLIP)]
    want = C.to_views_expected(per_image)
    desc, flip, image = _descriptors(tta, inverse=False)
    rows = [n, 5]
    image_rows = torch.tensor([0, n, n + 5], dtype=torch.int32, device=DEV)
    out_row, cursor = [], 0
    for im, _ in C.box_views():
        out_row.append(cursor)
        cursor += rows[im]
    got = tta.tta_boxes_to_views(torch.from_numpy(np.concatenate(per_image)).to(DEV), image_rows, desc, flip, image,
                                 torch.tensor(out_row, dtype=torch.int64, device=DEV), cursor, max(rows))
    torch.cuda.synchronize()
    assert got.shape == (3 * n + 10, 4)
    assert C.nan_equal(got.cpu(), torch.from_numpy(np.concatenate(want)))
    if n == 257:
        w = np.concatenate(want)
        assert (w[~np.isnan(w)] < 0).any() and np.isinf(w).any()   # nothing was clipped


def test_box_kernels_refuse_bad_arguments(tta):
    from u2seg_amd import _hip

    desc, flip, image = _descriptors(tta, inverse=True)
    z = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_tta_boxes_to_original", z, z, flip, desc, flip, image, z, z, z, -1, 5, 2, 1e-8)
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_tta_boxes_to_original", z, None, flip, desc, flip, image, z, z, z, 4, 5, 2, 1e-8)
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_tta_boxes_to_views", z, flip, desc, flip, image, None, z, 4, 5, 2)
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_tta_reduce_masks", z, flip, flip, flip, z, 4, 0, 2, 28)
    _hip.call("u2_tta_reduce_masks", None, None, None, None, None, 0, 1, 2, 28)   # no rows: valid, nothing launched


# ---- 2. the mask mean -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [28, 7])
@pytest.mark.parametrize("images", C.REDUCE_CASES, ids=lambda c: "-".join("v%dr%d" % vr for vr in c))
def test_reduce_masks_equals_the_sequential_sum(tta, images, side):
    """u2_tta_reduce_masks == the sequential float32 loop (flipped views mirrored, one division by float(V)), torch.equal, and
    within V * 2^-24 of the float64 mean: V in {1, 2, 3, 18}, R in {0, 1, 37}, two images of different R and V in a launch, the
    odd centre column with P = 7."""
    probs, flips = C.reduce_case(images, side)
    want = C.reduce_expected(probs, flips)
    dev_probs = [p.to(DEV) for views in probs for p in views]
    vs, rs = [v for v, _ in images], [r for _, r in images]
    flip = torch.tensor([f for fl in flips for f in fl], dtype=torch.int32, device=DEV)
    image_views = torch.tensor(np.concatenate([[0], np.cumsum(vs)]), dtype=torch.int32, device=DEV)
    image_rows = torch.tensor(np.concatenate([[0], np.cumsum(rs)]), dtype=torch.int32, device=DEV)
    got = tta.tta_reduce_masks(dev_probs, flip, image_views, image_rows, rs, vs, side)
    torch.cuda.synchronize()
    assert got.shape == (sum(rs), 1, side, side)
    assert torch.equal(got.cpu(), want)
    if got.numel():
        exact = C.reduce_exact_mean(probs, flips)
        per_row_v = torch.tensor([v for v, r in images for _ in range(r)], dtype=torch.float64).view(-1, 1, 1, 1)
        assert bool(((got.cpu().double() - exact).abs() <= per_row_v * 2.0 ** -24).all())
        # the same loop on the device, as impl="host" runs it
        host = torch.cat([tta.mean_in_view_order([(p.flip(dims=[3]) if f else p).to(DEV) for p, f in zip(views, fl)])
                          for views, fl in zip(probs, flips) if views[0].shape[0]])
        assert torch.equal(host, got)


# ---- 3. the views of one source ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre_resize", [True, False])
def test_device_views_equal_the_host_views(tta, pre_resize):
    """V descriptors on one source in one call of u2_aug_resize_bilinear_u8 == the mapper's PIL views, bit for bit (6 views)."""
    inp = C.image_input(pre_resize)
    host = C.mapper()(inp)
    geometry = [(h, w, k % 2) for k, (h, w) in enumerate(C.VIEW_SHAPES)]
    views = tta.device_views(inp["image"].to(DEV), geometry)
    torch.cuda.synchronize()
    assert len(views) == 6
    for k, (v, h) in enumerate(zip(views, host)):
        assert v.dtype == torch.uint8 and torch.equal(v.cpu(), h["image"]), k


# ---- 4. the model ---------------------------------------------------------------------------------------------------------------
E2E_OPTS = ["TEST.AUG.MIN_SIZES", (64, 96, 128), "TEST.AUG.MAX_SIZE", 160, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0]


@pytest.fixture(scope="module")
def small_model(tta):
    """The small configuration of the GPU tests (u2seg_R50_800 with det_fill weights), eval mode, every detection let through."""
    from tests.golden.make_fixtures import det_fill
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model

    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(["MODEL.DEVICE", DEV] + E2E_OPTS)
    model = build_model(cfg)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(det_fill(k, v.cpu()).to(DEV))
    model.eval()
    return cfg, model


def _inputs():
    from u2seg_amd.data import make_synthetic_batch

    out = []
    for i, (h, w, oh, ow) in enumerate([(96, 128, 144, 192), (80, 112, 80, 112)]):
        x = make_synthetic_batch(1, start_index=i, height=h, width=w, device=DEV)[0]
        out.append({"image": x["image"], "height": oh, "width": ow})
    return out


def test_inference_with_detected_instances(small_model):
    """Feeding an image's own predicted boxes and classes back returns the same pred_masks as the plain call; the plain call is
    what it was (PanopticFPN's own inference reports the same instances)."""
    from u2seg_amd.modeling import GeneralizedRCNN
    from u2seg_amd.structures import Boxes, Instances

    cfg, model = small_model
    batch = _inputs()
    with torch.no_grad():
        plain = GeneralizedRCNN.inference(model, batch, do_postprocess=False)
        given = [Instances(p.image_size, pred_boxes=Boxes(p.pred_boxes.tensor.clone()), pred_classes=p.pred_classes.clone())
                 for p in plain]
        again = GeneralizedRCNN.inference(model, batch, given, do_postprocess=False)
        post = GeneralizedRCNN.inference(model, batch)
        full = model(batch)
    for p, a, x in zip(plain, again, batch):
        assert len(p) > 0 and p.pred_masks.shape == (len(p), 1, 28, 28)
        assert torch.equal(a.pred_masks, p.pred_masks) and torch.equal(a.pred_boxes.tensor, p.pred_boxes.tensor)
        assert not a.has("scores")   # nothing but the masks was added
    for q, f, x in zip(post, full, batch):
        qi, fi = q["instances"], f["instances"]
        assert qi.image_size == (x["height"], x["width"]) and set(q) == {"instances"} and "panoptic_seg" in f
        assert torch.equal(qi.pred_boxes.tensor, fi.pred_boxes.tensor) and torch.equal(qi.scores, fi.scores)
        assert torch.equal(qi.pred_classes, fi.pred_classes) and torch.equal(qi.pred_masks, fi.pred_masks)


def _hand_made(tta):
    """Two identity views of one 400 x 400 image: the same object seen twice (the lower score goes), the same box as another
    class (stays), two equal scores (view order), a NaN box, a score of 0, and enough left for a top-k cut."""
    from u2seg_amd.structures import Boxes, Instances

    v0 = ([[10, 10, 50, 50], [100, 100, 150, 150], [200, 10, 240, 50], [float("nan"), 10, 90, 90], [10, 100, 40, 140]],
          [0.9, 0.5, 0.7, 0.8, 0.0], [1, 2, 3, 6, 4])
    v1 = ([[11, 11, 50, 50], [10, 10, 50, 50], [300, 10, 340, 50]], [0.8, 0.85, 0.7], [1, 5, 3])
    dets = []
    for b, s, c in (v0, v1):
        dets.append(Instances((400, 400), pred_boxes=Boxes(torch.tensor(b, dtype=torch.float32, device=DEV)),
                              scores=torch.tensor(s, dtype=torch.float32, device=DEV),
                              pred_classes=torch.tensor(c, dtype=torch.int64, device=DEV)))
    want = [([10, 10, 50, 50], 0.9, 1), ([10, 10, 50, 50], 0.85, 5), ([200, 10, 240, 50], 0.7, 3), ([300, 10, 340, 50], 0.7, 3),
            ([100, 100, 150, 150], 0.5, 2)]
    return dets, want


@pytest.mark.parametrize("topk", [100, 3])
def test_merge_on_hand_made_detections(tta, topk):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import transforms as T
    from u2seg_amd.modeling import GeneralizedRCNN, GeneralizedRCNNWithTTA

    cfg = get_cfg()
    cfg.merge_from_list(["TEST.DETECTIONS_PER_IMAGE", topk, "MODEL.ROI_HEADS.NMS_THRESH_TEST", 0.5])
    blank = GeneralizedRCNN.__new__(GeneralizedRCNN)
    torch.nn.Module.__init__(blank)
    w = GeneralizedRCNNWithTTA(cfg, blank)
    dets, want = _hand_made(tta)
    want = want[:topk]
    host = w._merge_detections(torch.cat([d.pred_boxes.tensor for d in dets]), torch.cat([d.scores for d in dets]),
                               torch.cat([d.pred_classes for d in dets]), (400, 400))
    ident = [tta.view_descriptor(T.TransformList([])) for _ in dets]
    desc = torch.from_numpy(np.stack([d for d, _ in ident])).to(DEV)
    clip = torch.tensor([[400.0, 400.0]], device=DEV)
    # the same image twice in one call: ragged bookkeeping over images
    device = w._merge_device(dets + dets[:1], [2, 1], torch.cat([desc, desc[:1]]), torch.zeros(3, dtype=torch.int32, device=DEV),
                             torch.tensor([0, 0, 1], dtype=torch.int32, device=DEV), torch.cat([clip, clip]), [(400, 400)] * 2)
    for got in (host, device[0]):
        assert got.image_size == (400, 400) and len(got) == len(want)
        assert got.pred_boxes.tensor.cpu().tolist() == [list(map(float, b)) for b, _, _ in want]
        assert torch.equal(got.scores.cpu(), torch.tensor([s for _, s, _ in want], dtype=torch.float32))
        assert got.pred_classes.cpu().tolist() == [c for _, _, c in want] and got.pred_classes.dtype == torch.int64
    alone = [([10, 10, 50, 50], 0.9, 1), ([200, 10, 240, 50], 0.7, 3), ([100, 100, 150, 150], 0.5, 2)][:topk]
    assert device[1].pred_boxes.tensor.cpu().tolist() == [list(map(float, b)) for b, _, _ in alone]
    assert device[1].pred_classes.cpu().tolist() == [c for _, _, c in alone]


def _same_instances(a, b):
    return (a.image_size == b.image_size and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
            and torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
            and a.pred_masks.dtype == torch.bool and torch.equal(a.pred_masks, b.pred_masks))


def test_device_path_equals_host_path_end_to_end(small_model, tta):
    """Two images of different size (one asked for at another size), 6 views, batch_size 3: impl="device" == impl="host" in
    boxes, scores, classes and pasted masks, bit for bit, with keep_features on and off.  Not empty: every view yields
    detections, the merge keeps >= 5 instances per image and suppresses at least one candidate (the top-k cut is out of the
    way: DETECTIONS_PER_IMAGE above the number of candidates)."""
    from u2seg_amd.modeling import GeneralizedRCNN, GeneralizedRCNNWithTTA

    cfg, model = small_model
    cfg = cfg.clone()
    cfg.merge_from_list(["TEST.DETECTIONS_PER_IMAGE", 1000])
    batch = _inputs()
    host = GeneralizedRCNNWithTTA(cfg, model, impl="host")
    with torch.no_grad():
        # the premise: the same view batch twice through the model gives the same bits (no statistics atomics in eval mode)
        views = host.tta_mapper(batch[0])[:3]
        for v in views:
            v.pop("transforms")
        with host._turn_off_roi_heads(["mask_on"]):
            a = GeneralizedRCNN.inference(model, views, do_postprocess=False)
            b = GeneralizedRCNN.inference(model, views, do_postprocess=False)
        assert not a[0].has("pred_masks")
        for x, y in zip(a, b):
            assert torch.equal(x.pred_boxes.tensor, y.pred_boxes.tensor) and torch.equal(x.scores, y.scores)
            assert torch.equal(x.pred_classes, y.pred_classes)
        # not empty
        for x in batch:
            views = host.tta_mapper(x)
            tfms = [v.pop("transforms") for v in views]
            assert len(views) == 6
            with host._turn_off_roi_heads(["mask_on"]):
                outs = host._batch_inference(views)
                boxes, scores, classes = host._get_augmented_boxes(views, tfms)
            assert all(len(o) > 0 for o in outs)
            cands = int((torch.isfinite(boxes).all(dim=1) & torch.isfinite(scores) & (scores > 1e-8)).sum())
            kept = len(host._merge_detections(boxes, scores, classes, (x["height"], x["width"])))
            print("views %s -> %d candidates, %d kept" % ([len(o) for o in outs], cands, kept))
            assert 5 <= kept < cands < 1000
        want = host(batch)
        on = GeneralizedRCNNWithTTA(cfg, model, impl="device", batch_size=3, keep_features=True)(batch)
        off = GeneralizedRCNNWithTTA(cfg, model, impl="device", batch_size=3, keep_features=False)(batch)
        one = GeneralizedRCNNWithTTA(cfg, model, impl="device")(batch[1:])
    assert model.roi_heads.mask_on
    for x, h, d, e in zip(batch, want, on, off):
        hi = h["instances"]
        assert set(h) == set(d) == {"instances"} and hi.image_size == (x["height"], x["width"])
        assert hi.pred_masks.shape == (len(hi), x["height"], x["width"]) and len(hi) >= 5
        assert _same_instances(d["instances"], hi), "impl='device' differs from impl='host'"
        assert _same_instances(e["instances"], hi), "keep_features=False differs"
    assert _same_instances(one[0]["instances"], want[1]["instances"])   # an image alone == the image in a list


# ---- 5. tools/train_net.py ------------------------------------------------------------------------------------------------------
def _same_results(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_results(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return True
    return a == b


def test_train_net_reports_tta_results_beside_the_plain_ones(small_model, tmp_path, monkeypatch):
    """tools/train_net.py --eval-only on tests/golden/data_small (the shared small model handed to main() in place of a freshly
    built one): TEST.AUG.ENABLED True adds bbox_TTA / segm_TTA beside the unchanged plain keys and writes under
    OUTPUT_DIR/inference_TTA; False adds none; the hungarian_matching pass, which writes the mapping, is never repeated with
    augmentation."""
    from u2seg_amd.data import DatasetCatalog, MetadataCatalog
    from u2seg_amd.engine import default_argument_parser
    from u2seg_amd.evaluation import hungarian

    monkeypatch.setenv("DETECTRON2_DATASETS", os.path.join(ROOT, "tests", "golden", "data_small"))
    monkeypatch.setenv("CLUSTER_NUM", "800")
    monkeypatch.chdir(tmp_path)
    for cat in (DatasetCatalog, MetadataCatalog):
        for name in list(cat.keys()):
            cat.remove(name)
    spec = importlib.util.spec_from_file_location("u2seg_train_net_tta", os.path.join(ROOT, "tools", "train_net.py"))
    train_net = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_net)
    monkeypatch.setattr(train_net, "build_model", lambda cfg: small_model[1])
    name = "coco_2017_train"

    def run(mode, aug):
        opts = ["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "DATASETS.TEST", (name,), "DATALOADER.NUM_WORKERS", 0,
                "INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 160, "TEST.AUG.ENABLED", aug, "TEST.AUG.MIN_SIZES", (64, 96),
                "TEST.AUG.MAX_SIZE", 160, "OUTPUT_DIR", str(tmp_path / "out")]
        args = default_argument_parser().parse_args(["--config-file", CFG, "--eval-only", "--eval-mode", mode, "--eval-tasks",
                                                     "bbox,segm"] + [str(o) for o in opts])
        return train_net.main(args)[name]

    first = run("hungarian_matching", True)
    assert set(first) == {"instance_mapping"} and not os.path.exists(tmp_path / "out" / "inference_TTA")
    # every cluster onto a category, so that detections reach the scoring whatever the matching of this tiny set found
    hungarian.save_mapping({c: c for c in range(800)}, "./hungarian_matching/instance_mapping.json")
    plain = run("eval", False)
    assert set(plain) == {"bbox", "segm"} and plain["bbox"]["num_results"] > 0
    assert not os.path.exists(tmp_path / "out" / "inference_TTA")
    both = run("eval", True)
    assert set(both) == {"bbox", "segm", "bbox_TTA", "segm_TTA"}
    assert _same_results({k: v for k, v in both.items() if not k.endswith("_TTA")}, plain)
    assert os.path.isfile(tmp_path / "out" / "inference_TTA" / "coco_instances_results.json")
    assert set(both["bbox_TTA"]) == set(plain["bbox"]) and set(both["segm_TTA"]) == set(plain["segm"])
    assert both["bbox_TTA"]["num_results"] > 0
