"""Semantic / panoptic test-time augmentation on the device (csrc/tta.hip: u2_tta_accumulate_sem_seg,
modeling/tta_panoptic.py: PanopticFPNWithTTA): the accumulate kernel against the existing
kernels bit for bit and against float64, padded storage, calls split in every way, ties, bad arguments, impl="device" against
impl="host" end to end, the anchor to the plain model, and the wiring in tools/train_net.py."""
import ctypes
import functools
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import tta_panoptic_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def tta():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.modeling import tta_panoptic

    _hip.load()
    return tta_panoptic


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's padded NaN-filled blocks on the device and its reference, computed once: u2_bilinear_resize_f32 per view (read
    in place through the block's strides), flip(-1) where flipped, mean_in_view_order.  Nothing here is written again."""
    from u2seg_amd import _hip
    from u2seg_amd.modeling.test_time_augmentation import mean_in_view_order

    c, H, W, _ = P.CASES[name]
    blocks, windows, flips = P.make_views(name, seed=3)
    dev = [torch.from_numpy(b).to(DEV) for b in blocks]
    terms = []
    for block, (h, w), flipped in zip(dev, windows, flips):
        out = torch.empty((c, H, W), dtype=torch.float32, device=DEV)
        _hip.call("u2_bilinear_resize_f32", block, out, c, h, w, block.stride(0), block.stride(1), H, W)
        terms.append(out.flip(-1) if flipped else out)
    want = mean_in_view_order(terms)
    torch.cuda.synchronize()
    return blocks, dev, windows, flips, want.cpu()


def _accumulate(tta, dev, windows, flips, shape, groups):
    """The views in calls of the given group sizes; the accumulator and the arg-max start poisoned."""
    acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    amax = torch.full(shape[1:], -7, dtype=torch.int64, device=DEV)
    assert sum(groups) == len(dev)
    v = 0
    for g in groups:
        last = v + g == len(dev)
        tta.tta_accumulate_sem_seg(dev[v:v + g], windows[v:v + g], flips[v:v + g], acc, v == 0, len(dev) if last else 0,
                                   amax if last else None)
        v += g
    torch.cuda.synchronize()
    return acc.cpu(), amax.cpu()


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_accumulate_equals_the_existing_kernels(tta, name):
    """One call == u2_bilinear_resize_f32 per view + flip + mean_in_view_order, torch.equal; the arg-max == numpy.argmax of it
    (first maximum).  Every view sits in a larger block whose padding is NaN: a NaN-free result shows that the window bounds
    and the strides are honoured.  Float64, independent of the old kernel: within (V + 8) * 2^-24 * max |logit|."""
    c, H, W, views = P.CASES[name]
    blocks, dev, windows, flips, want = _case(name)
    got, amax = _accumulate(tta, dev, windows, flips, (c, H, W), [len(views)])
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(want).any())
    assert torch.equal(got, want)
    assert np.array_equal(amax.numpy(), np.argmax(want.numpy(), axis=0))
    exact = P.mean_logits_f64(blocks, windows, flips, H, W)
    magnitude = max(float(np.abs(b[:, :h, :w]).max()) for b, (h, w) in zip(blocks, windows))
    err = float(np.abs(got.numpy().astype(np.float64) - exact).max())
    print("%s: max error against float64 %.3e, bound %.3e" % (name, err, P.bound(len(views), magnitude)))
    assert err <= P.bound(len(views), magnitude)


@pytest.mark.parametrize("groups", [(3,) * 6, (4, 14), (1,) * 18, (17, 1)], ids=lambda g: "+".join(map(str, g)))
def test_split_calls_give_the_bits_of_one_call(tta, groups):
    """18 views in calls of 3 + 3 + ..., 4 + 14 (first and divisor on different calls), one by one, 17 + 1."""
    name = "c28_33x257_v18"
    c, H, W, _ = P.CASES[name]
    _, dev, windows, flips, want = _case(name)
    got, amax = _accumulate(tta, dev, windows, flips, (c, H, W), list(groups))
    assert torch.equal(got, want)
    assert np.array_equal(amax.numpy(), np.argmax(want.numpy(), axis=0))


def test_split_of_four_views_as_three_and_one(tta):
    from u2seg_amd.modeling.test_time_augmentation import mean_in_view_order

    name = "c28_37x53_v6"
    c, H, W, _ = P.CASES[name]
    _, dev, windows, flips, _ = _case(name)
    dev, windows, flips = dev[:4], windows[:4], flips[:4]
    one, amax_one = _accumulate(tta, dev, windows, flips, (c, H, W), [4])
    two, amax_two = _accumulate(tta, dev, windows, flips, (c, H, W), [3, 1])
    assert torch.equal(one, two) and torch.equal(amax_one, amax_two)
    from u2seg_amd.modeling.inference import sem_seg_postprocess

    terms = [sem_seg_postprocess(b, win, H, W) for b, win in zip(dev, windows)]
    want = mean_in_view_order([t.flip(-1) if f else t for t, f in zip(terms, flips)])
    assert torch.equal(one, want.cpu())


def test_ties_take_the_lower_class_and_an_inf_passes_through(tta):
    """Classes 1 and 2 carry the same logits in both views (an identity view and its flipped twin), above class 0 on the left
    half: the arg-max is 1 there, 0 elsewhere.  A +Inf in the identity view arrives as +Inf and makes no NaN beside it (the
    bilinear expression would: 0 * inf)."""
    from u2seg_amd.modeling.inference import sem_seg_postprocess
    from u2seg_amd.modeling.test_time_augmentation import mean_in_view_order

    H, W = 4, 6
    rs = np.random.RandomState(1)
    views = []
    for _ in range(2):
        v = np.zeros((3, H, W), dtype=np.float32)
        v[0] = rs.uniform(-1, 1, size=(H, W))
        v[1] = v[2] = rs.uniform(-1, 1, size=(H, W))
        views.append(v)
    # symmetric offsets, so that the mean of a view and a mirrored view keeps the pattern: classes 1, 2 win in columns 0, 1, 4, 5
    for v in views:
        v[1:, :, [0, 1, 4, 5]] += 4.0
        v[0, :, [2, 3]] += 4.0
    views[0][0, 2, 3] = np.inf
    dev = [torch.from_numpy(v).to(DEV) for v in views]
    windows, flips = [(H, W)] * 2, [False, True]
    got, amax = _accumulate(tta, dev, windows, flips, (3, H, W), [2])
    want = mean_in_view_order([sem_seg_postprocess(d, (H, W), H, W).flip(-1) if f else sem_seg_postprocess(d, (H, W), H, W)
                               for d, f in zip(dev, flips)]).cpu()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, want) and got[0, 2, 3] == float("inf") and int(torch.isinf(got).sum()) == 1
    assert torch.equal(got[1], got[2])
    expect = np.zeros((H, W), dtype=np.int64)
    expect[:, [0, 1, 4, 5]] = 1
    assert np.array_equal(amax.numpy(), expect) and np.array_equal(amax.numpy(), np.argmax(got.numpy(), axis=0))


def test_accumulate_refuses_bad_arguments(tta):
    """C = 65, n = 0, a zero window side, a null pointer: a negative status, the accumulator untouched."""
    from u2seg_amd import _hip

    src = torch.zeros((65, 4, 4), dtype=torch.float32, device=DEV)
    acc = torch.full((65, 4, 4), 5.0, dtype=torch.float32, device=DEV)
    ptrs = torch.tensor([src.data_ptr()], dtype=torch.int64, device=DEV)

    def desc(h, w):
        return (ctypes.c_longlong * 5)(h, w, 4, 16, 0)

    for args in [(ptrs, desc(4, 4), 1, acc, 1, 1, None, 65, 4, 4),      # C = 65
                 (ptrs, desc(4, 4), 0, acc, 1, 1, None, 3, 4, 4),       # n = 0
                 (ptrs, desc(0, 4), 1, acc, 1, 1, None, 3, 4, 4),       # a zero window side
                 (ptrs, desc(4, 0), 1, acc, 1, 1, None, 3, 4, 4),
                 (ptrs, desc(4, 4), 1, acc, 1, 1, None, 0, 4, 4),       # C = 0
                 (ptrs, desc(4, 4), 1, acc, 1, 1, None, 3, 0, 4),       # H = 0
                 (None, desc(4, 4), 1, acc, 1, 1, None, 3, 4, 4),       # null pointers
                 (ptrs, desc(4, 4), 1, None, 1, 1, None, 3, 4, 4)]:
        with pytest.raises(RuntimeError, match="status -1"):
            _hip.call("u2_tta_accumulate_sem_seg", *args)
    torch.cuda.synchronize()
    assert bool((acc == 5.0).all())
    _hip.call("u2_tta_accumulate_sem_seg", ptrs, desc(4, 4), 1, acc, 1, 1, None, 64, 4, 4)   # the register limit itself is served
    torch.cuda.synchronize()
    assert bool((acc[:64] == 0.0).all()) and bool((acc[64] == 5.0).all())


# ---- 1b. GroupNorm statistics in a fixed order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b,hw,c", [(2, 37 * 53, 128), (1, 1, 8), (3, 700, 24), (1, 256 * 256 + 5, 64)])
def test_ordered_column_statistics(tta, b, hw, c):
    """u2_colstats_ordered (the GroupNorm statistics of a pass without a graph): twice the same bits, within the recursive
    summation bound n * 2^-24 * sum |x| of the float64 sums (any order of additions meets it); chunk counts above and below
    the number of rows, a channel count that does not divide the work-group (24), more chunks than rows (hw = 1)."""
    from u2seg_amd import _hip

    gen = torch.Generator(device=DEV).manual_seed(b * 1000 + c)
    x = (torch.randn((b, hw, c), device=DEV, generator=gen) * 2 + 0.5).to(torch.bfloat16)
    nchunk = max(1, min(256, (hw + 255) // 256))
    outs = []
    for fill in (float("nan"), 7.0):   # neither the scratch nor the result is read before it is written
        part = torch.full((b, nchunk, 2, c), fill, dtype=torch.float32, device=DEV)
        out = torch.full((b, 2, c), fill, dtype=torch.float32, device=DEV)
        _hip.call("u2_colstats_ordered", x, part, out, b, hw, c, c, nchunk)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    xd = x.double()
    want = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=1)
    bound = hw * 2.0 ** -24 * torch.stack([xd.abs().sum(1), (xd * xd).sum(1)], dim=1)
    assert bool(((outs[0].double() - want).abs() <= bound).all())
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_colstats_ordered", x, part, out, b, hw, 4, 4, nchunk)
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_colstats_ordered", x, part, out, b, hw, c, c, 0)


def test_group_norm_without_a_graph_repeats_its_bits(tta):
    """group_norm_act under torch.no_grad(): the same bits twice, and the values of the recorded pass (atomic statistics) up
    to one bf16 step of the output."""
    from u2seg_amd.layers import functional as F

    gen = torch.Generator(device=DEV).manual_seed(4)
    y = torch.randn((3, 67, 113, 128), device=DEV, generator=gen).to(torch.bfloat16)
    gamma = torch.rand(128, device=DEV, generator=gen) + 0.5
    beta = torch.randn(128, device=DEV, generator=gen)
    with torch.no_grad():
        a = F.group_norm_act(y, gamma, beta, 32, relu=True)
        b = F.group_norm_act(y, gamma, beta, 32, relu=True)
    recorded = F.group_norm_act(y, gamma.requires_grad_(), beta.requires_grad_(), 32, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    diff = (a.float() - recorded.detach().float()).abs()
    assert bool((diff <= 2.0 ** -7 * recorded.detach().float().abs().clamp_min(2.0 ** -7)).all())


# ---- 2. the model ---------------------------------------------------------------------------------------------------------------
E2E_OPTS = ["TEST.AUG.MIN_SIZES", (64, 96, 128), "TEST.AUG.MAX_SIZE", 160, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0]


@pytest.fixture(scope="module")
def small_model(tta):
    """The small configuration of tests/test_gpu_tta.py (u2seg_R50_800 with det_fill weights), eval mode."""
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


def _same_instances(a, b):
    return (a.image_size == b.image_size and torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor)
            and torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
            and a.pred_masks.dtype == torch.bool and torch.equal(a.pred_masks, b.pred_masks))


def test_device_path_equals_host_path_end_to_end(small_model):
    """Two images of different size (one asked for at another size), 6 views, batch_size 3: impl="device" == impl="host" in
    sem_seg (torch.equal), the panoptic id map and segments_info; the instances are those of GeneralizedRCNNWithTTA."""
    from u2seg_amd.modeling import GeneralizedRCNNWithTTA, PanopticFPNWithTTA

    cfg, model = small_model
    cfg = cfg.clone()
    cfg.merge_from_list(["TEST.DETECTIONS_PER_IMAGE", 1000])
    batch = _inputs()
    with torch.no_grad():
        host = PanopticFPNWithTTA(cfg, model, impl="host")(batch)
        device = PanopticFPNWithTTA(cfg, model, impl="device", batch_size=3)(batch)
        instances = GeneralizedRCNNWithTTA(cfg, model, impl="device", batch_size=3)(batch)
    torch.cuda.synchronize()
    assert "_detect_from_features" not in vars(model)   # the wrapper stood in front of the model's method only during its calls
    classes = model.sem_seg_head.num_classes
    for x, h, d, i in zip(batch, host, device, instances):
        size = (x["height"], x["width"])
        assert set(h) == set(d) == {"instances", "sem_seg", "panoptic_seg"}
        assert d["sem_seg"].dtype == torch.float32 and tuple(d["sem_seg"].shape) == (classes,) + size
        assert bool(torch.isfinite(d["sem_seg"]).all()) and float(d["sem_seg"].std()) > 0
        assert torch.equal(d["sem_seg"], h["sem_seg"]), "the mean logits of impl='device' differ from impl='host'"
        (d_ids, d_info), (h_ids, h_info) = d["panoptic_seg"], h["panoptic_seg"]
        assert tuple(d_ids.shape) == size and torch.equal(d_ids, h_ids) and d_info == h_info
        assert _same_instances(d["instances"], i["instances"]) and _same_instances(h["instances"], i["instances"])
        assert len(d["instances"]) >= 5
        # the merge was fed the arg-max of the mean: every stuff segment's pixels carry its class there
        argmax = d["sem_seg"].argmax(dim=0)
        for seg in d_info:
            if not seg["isthing"]:
                assert bool((argmax[d_ids == seg["id"]] == seg["category_id"]).all())


def test_one_identity_view_gives_the_plain_models_sem_seg(small_model):
    """Anchor to tested behaviour: with one unflipped view of the input's own size the wrapper's sem_seg equals the plain
    model's, bit for bit, on both implementations; one image per call, so that the batch shapes match."""
    from u2seg_amd.modeling import PanopticFPNWithTTA

    cfg, model = small_model
    for x in _inputs():
        c = cfg.clone()
        h, w = x["image"].shape[1:]
        c.merge_from_list(["TEST.AUG.MIN_SIZES", (min(h, w),), "TEST.AUG.MAX_SIZE", max(h, w), "TEST.AUG.FLIP", False])
        with torch.no_grad():
            plain = model([x])[0]
            device = PanopticFPNWithTTA(c, model, impl="device")([x])[0]
            host = PanopticFPNWithTTA(c, model, impl="host")([x])[0]
        assert tuple(plain["sem_seg"].shape[1:]) == (x["height"], x["width"])
        assert torch.equal(device["sem_seg"], plain["sem_seg"])
        assert torch.equal(host["sem_seg"], plain["sem_seg"])


def test_more_than_64_classes_are_refused_on_the_device_path(small_model, monkeypatch):
    from u2seg_amd.modeling import PanopticFPNWithTTA

    cfg, model = small_model
    monkeypatch.setattr(model.sem_seg_head, "num_classes", 65)
    with pytest.raises(NotImplementedError, match="64 classes"):
        PanopticFPNWithTTA(cfg, model, impl="device")
    PanopticFPNWithTTA(cfg, model, impl="host")


# ---- 3. tools/train_net.py ------------------------------------------------------------------------------------------------------
def _same_finiteness(a, b):
    """Every float of b is finite or NaN exactly where its counterpart in a is; the structure is the same."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_finiteness(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same_finiteness(x, y) for x, y in zip(a, b))
    if isinstance(a, float) or isinstance(b, float):
        return (isinstance(a, (int, float)) and isinstance(b, (int, float))
                and math.isnan(a) == math.isnan(b) and math.isinf(a) == math.isinf(b))
    return type(a) is type(b)


def test_train_net_reports_semantic_and_panoptic_tta_results(small_model, tmp_path, monkeypatch):
    """tools/train_net.py --eval-only on tests/golden/data_small as the panoptic dataset (the shared small model handed to
    main()): --tta-outputs panoptic adds _TTA copies of the semantic, instance and panoptic keys and writes under
    OUTPUT_DIR/inference_TTA; without the flag only the instance keys get a copy, as before."""
    from u2seg_amd.data import DatasetCatalog, MetadataCatalog
    from u2seg_amd.engine import default_argument_parser
    from u2seg_amd.evaluation import hungarian

    monkeypatch.setenv("DETECTRON2_DATASETS", os.path.join(ROOT, "tests", "golden", "data_small"))
    monkeypatch.setenv("CLUSTER_NUM", "800")
    monkeypatch.chdir(tmp_path)
    for cat in (DatasetCatalog, MetadataCatalog):
        for name in list(cat.keys()):
            cat.remove(name)
    spec = importlib.util.spec_from_file_location("u2seg_train_net_tta_panoptic", os.path.join(ROOT, "tools", "train_net.py"))
    train_net = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_net)
    monkeypatch.setattr(train_net, "build_model", lambda cfg: small_model[1])
    name = "coco_2017_train_panoptic_separated"

    def run(mode, extra=()):
        opts = ["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "DATASETS.TEST", (name,), "DATALOADER.NUM_WORKERS", 0,
                "INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 160, "TEST.AUG.ENABLED", True, "TEST.AUG.MIN_SIZES", (64, 96),
                "TEST.AUG.MAX_SIZE", 160, "OUTPUT_DIR", str(tmp_path / "out")]
        args = default_argument_parser().parse_args(["--config-file", CFG, "--eval-only", "--eval-mode", mode, "--eval-tasks",
                                                     "bbox,segm"] + list(extra) + [str(o) for o in opts])
        return train_net.main(args)[name]

    first = run("hungarian_matching", ["--tta-outputs", "panoptic"])
    assert not any(k.endswith("_TTA") for k in first) and not os.path.exists(tmp_path / "out" / "inference_TTA")
    # every cluster onto a category, so that predictions reach the scoring whatever the matching of this tiny set found
    hungarian.save_mapping({c: c for c in range(800)}, "./hungarian_matching/instance_mapping.json")
    hungarian.save_mapping({c: (c - 1) % 15 + 1 if c else 0 for c in range(28)}, "./hungarian_matching/semantic_mapping.json")
    as_before = run("eval")
    plain_keys = {"sem_seg", "bbox", "segm", "panoptic_seg"}
    assert set(as_before) == plain_keys | {"bbox_TTA", "segm_TTA"}
    assert not os.path.exists(tmp_path / "out" / "inference_TTA" / "predictions.json")
    both = run("eval", ["--tta-outputs", "panoptic"])
    assert set(both) == plain_keys | {k + "_TTA" for k in plain_keys}
    for k in plain_keys:
        assert _same_finiteness(both[k], both[k + "_TTA"]), k
    assert _same_finiteness({k: as_before[k] for k in plain_keys}, {k: both[k] for k in plain_keys})
    assert both["bbox_TTA"]["num_results"] > 0 and both["panoptic_seg_TTA"]["num_images"] == both["panoptic_seg"]["num_images"] > 0
    assert os.path.isfile(tmp_path / "out" / "inference_TTA" / "predictions.json")
    assert os.path.isfile(tmp_path / "out" / "inference_TTA" / "coco_instances_results.json")
    assert both["panoptic_seg_TTA"]["predictions_json"] != both["panoptic_seg"]["predictions_json"]
