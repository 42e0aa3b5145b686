"""Boundary IoU of the semantic evaluator on the host (evaluation/semseg_ops.py, evaluation/sem_seg_evaluation.py with
boundary_iou=True) against a literal numpy restatement of the reference's _mask_to_boundary and of the lines of its process()
and evaluate() that use it (detectron2/evaluation/sem_seg_evaluation.py:269-276, 344-360, 396-407).  Parity with the cv2
binary itself is not pinned: cv2 is not available; where scipy is, scipy.ndimage.minimum_filter is a second witness.
Integers throughout: the matrices are compared with ==.  CPU only."""
import math

import numpy as np
import pytest
import torch

from tests import semseg_boundary_cases as cases
from u2seg_amd.data import MetadataCatalog
from u2seg_amd.evaluation import SemSegEvaluator, hungarian, semseg_ops
from u2seg_amd.evaluation import sem_seg_evaluation as sse

N = cases.N


def host(pred, gt, lut, d, n=N):
    c, b = semseg_ops.boundary_confusion_host(torch.from_numpy(pred), torch.from_numpy(gt),
                                              None if lut is None else torch.from_numpy(lut), d, n)
    assert c.dtype == torch.int64 and b.dtype == torch.int64 and c.shape == b.shape == (n, n)
    return c.numpy(), b.numpy()


@pytest.mark.parametrize("h,w,d", cases.SHAPES)
def test_host_definition_equals_the_literal_restatement(h, w, d):
    for name, (pred, gt) in cases.label_maps(h, w, seed=h * 1000 + w + d).items():
        eroded = semseg_ops.erode_host(torch.from_numpy(pred), d).numpy()
        assert np.array_equal(pred - eroded, cases.literal_boundary(pred, d)), name  # every pixel, not only the counts
        want_c, want_b = cases.literal_confusion(pred, gt, None, d)
        got_c, got_b = host(pred, gt, None, d)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_b, want_b), name
        assert got_b.sum() == h * w == got_c.sum()


def test_window_larger_than_the_image_leaves_the_map_itself():
    pred, _ = cases.label_maps(7, 9, seed=1)["blobs"]
    assert np.array_equal(cases.literal_boundary(pred, 4), pred)
    assert not semseg_ops.erode_host(torch.from_numpy(pred), 4).any()
    assert not semseg_ops.erode_host(torch.from_numpy(pred), 4000).any()  # far beyond any padding torch would accept


def test_lut_is_applied_before_the_erosion():
    rs = np.random.RandomState(5)
    lut = cases.chained_lut()
    pred = np.repeat(np.repeat(rs.randint(0, 28, size=(9, 17)), 8, axis=0), 8, axis=1)[:70, :131].astype(np.uint8)
    gt = cases.blobs(rs, 70, 131)
    want_c, want_b = cases.literal_confusion(pred, gt, lut, 7)
    got_c, got_b = host(pred, gt, lut, 7)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_b, want_b)
    mapped_after = lut[cases.literal_boundary(pred, 7)]  # the wrong order gives another matrix on this input
    assert not np.array_equal(mapped_after, cases.literal_boundary(lut[pred], 7))


@pytest.mark.parametrize("h,w,d", cases.SHAPES)
def test_scipy_minimum_filter_agrees(h, w, d):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, (pred, _) in cases.label_maps(h, w, seed=h + w + d).items():
        eroded = ndimage.minimum_filter(pred, size=2 * d + 1, mode="constant", cval=0)
        assert np.array_equal(pred - eroded, cases.literal_boundary(pred, d)), name
        assert np.array_equal(semseg_ops.erode_host(torch.from_numpy(pred), d).numpy(), eroded), name


def test_known_answer_by_hand():
    """5 x 5, all label 3, d = 1: the 3 x 3 interior erodes to 3 (boundary 0), the 16 border pixels to 0 (boundary 3)."""
    m = np.full((5, 5), 3, dtype=np.uint8)
    conf, bconf = host(m, m, None, 1)
    want = np.zeros((N, N), dtype=np.int64)
    want[3, 3], want[0, 0] = 16, 9
    assert np.array_equal(bconf, want)
    assert conf[3, 3] == 25 and conf.sum() == 25
    assert np.array_equal(cases.literal_confusion(m, m, None, 1)[1], want)


def test_arguments_are_checked():
    m = torch.zeros((4, 4), dtype=torch.uint8)
    for bad in (dict(d=0), dict(n=33), dict(n=0)):
        with pytest.raises(ValueError):
            semseg_ops.boundary_confusion_host(m, m, None, **dict(dict(d=1, n=N), **bad))
    with pytest.raises(ValueError):
        semseg_ops.boundary_confusion_host(m, m.long(), None, 1, N)
    with pytest.raises(ValueError):
        semseg_ops.boundary_confusion_host(m + 17, m, None, 1, N)  # a label >= n


def test_dilation_rule():
    """max(1, round(0.02 * diagonal)) with Python's round: half to even."""
    for (h, w), d in (((480, 640), 16), ((800, 1333), 31), ((427, 640), 15), ((5000, 5000), 141), ((1, 1), 1)):
        assert semseg_ops.boundary_dilation(h, w) == d, (h, w)
    assert 0.02 * math.sqrt(75 * 75 + 100 * 100) == 2.5  # the product lands on .5 exactly
    assert semseg_ops.boundary_dilation(75, 100) == 2    # half to even; half up would give 3
    assert 0.02 * math.sqrt(105 * 105 + 140 * 140) == 3.5
    assert semseg_ops.boundary_dilation(105, 140) == 4
    for h, w, d in cases.SHAPES[:4]:
        assert semseg_ops.boundary_dilation(h, w) == 1


def test_cpu_maps_take_the_host_route_and_accumulate():
    pred, gt = cases.label_maps(40, 33, seed=3)["blobs"]
    conf = torch.full((N, N), 2, dtype=torch.int64)
    bconf = torch.full((N, N), 5, dtype=torch.int64)
    want_c, want_b = cases.literal_confusion(pred, gt, None, 2)
    semseg_ops.boundary_confusion(torch.from_numpy(pred), torch.from_numpy(gt), None, 2, N, conf, bconf)
    assert np.array_equal(conf.numpy(), want_c + 2) and np.array_equal(bconf.numpy(), want_b + 5)
    semseg_ops.boundary_confusion(torch.from_numpy(pred), torch.from_numpy(gt), None, 2, N, None, bconf)
    assert np.array_equal(bconf.numpy(), 2 * want_b + 5)


# ---- the evaluator on the tiny validation set of tests/golden/eval_golden (the reference's own evaluators made it)


@pytest.fixture()
def tiny_val_sem(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # the mapping file is read from ./hungarian_matching like in the reference
    return cases.tiny_val_sem(tmp_path)


def literal_matrices(outputs, gts):
    """The reference's process(), restated: the in-place chained remapping, ignore -> 16, both bincounts."""
    conf, bconf = np.zeros((N, N), dtype=np.int64), np.zeros((N, N), dtype=np.int64)
    mapping = hungarian.load_mapping("./hungarian_matching/semantic_mapping.json")
    for out, gt in zip(outputs, gts):
        pred = out["sem_seg"].argmax(dim=0).numpy().astype(int)
        gt = sse.to_supercategories(gt.astype(int))
        gt[gt == 255] = 16
        for cls, tgt in mapping.items():
            pred[pred == int(cls)] = 16 if tgt == -1 else tgt
        h, w = pred.shape
        d = max(1, int(round(0.02 * np.sqrt(h ** 2 + w ** 2))))
        c, b = cases.literal_confusion(pred.astype(np.uint8), gt.astype(np.uint8), None, d)
        conf += c
        bconf += b
    return conf, bconf


def literal_results(conf, bconf, names):
    """The reference's evaluate(), the lines that make IoU, BoundaryIoU and their minimum."""
    tp = conf.diagonal()[:-1].astype(float)
    pos_gt = np.sum(conf[:-1, :-1], axis=0).astype(float)
    pos_pred = np.sum(conf[:-1, :-1], axis=1).astype(float)
    union = pos_gt + pos_pred - tp
    iou = np.full(16, np.nan)
    valid = np.logical_and(pos_gt > 0, union > 0)
    iou[valid] = tp[valid] / union[valid]
    b_iou = np.full(16, np.nan)
    b_tp = bconf.diagonal()[:-1].astype(float)
    b_union = np.sum(bconf[:-1, :-1], axis=0).astype(float) + np.sum(bconf[:-1, :-1], axis=1).astype(float) - b_tp
    b_iou[b_union > 0] = b_tp[b_union > 0] / b_union[b_union > 0]
    res = {}
    for i, name in enumerate(names):
        res["BoundaryIoU-" + name] = 100 * b_iou[i]
        res["min(IoU, B-Iou)-" + name] = 100 * min(iou[i], b_iou[i])
    return res


def same(a, b):
    return (a != a and b != b) or a == pytest.approx(b, rel=1e-12, abs=0)


def test_evaluator_reports_boundary_iou(tiny_val_sem):
    fx, inputs, outputs, gts = tiny_val_sem
    ev = SemSegEvaluator("tiny_val_sem", output_dir="out", mode="eval", boundary_iou=True)
    ev.process(inputs, outputs)
    want_c, want_b = literal_matrices(outputs, gts)
    assert ev._conf_matrix.tolist() == fx["conf_matrix"] == want_c.tolist()
    assert ev._b_conf_matrix.tolist() == want_b.tolist()
    assert ev._b_conf_matrix.device == ev._conf_matrix.device
    res = ev.evaluate()["sem_seg"]
    names = ["things"] + list(sse.SUPERCATEGORIES)
    order = []
    for k in fx["sem_seg_results"]:
        order.append(k)
        if k.startswith("IoU-"):
            order += ["BoundaryIoU-" + k[4:], "min(IoU, B-Iou)-" + k[4:]]
    assert list(res) == order
    for k, v in fx["sem_seg_results"].items():  # every old key has its old value
        assert (res[k] != res[k]) if v is None else (res[k] == pytest.approx(v, rel=1e-12)), k
    want = literal_results(want_c, want_b, names)
    assert len(want) == 32
    for k, v in want.items():
        assert same(res[k], v), (k, res[k], v)
    assert any(v == v and v > 0 for k, v in want.items() if k.startswith("BoundaryIoU-"))  # the set exercises the numbers
    saved = torch.load("out/sem_seg_evaluation.pth", weights_only=False)
    assert list(saved) == order and all(same(saved[k], res[k]) for k in order)


def test_default_output_is_unchanged(tiny_val_sem):
    fx, inputs, outputs, _ = tiny_val_sem
    ev = SemSegEvaluator("tiny_val_sem", mode="eval")
    sent = []
    real = sse.gather_to_rank0
    try:
        sse.gather_to_rank0 = lambda obj: sent.append(obj) or real(obj)
        ev.process(inputs, outputs)
        res = ev.evaluate()["sem_seg"]
    finally:
        sse.gather_to_rank0 = real
    assert list(res) == list(fx["sem_seg_results"])
    assert len(sent) == 1 and sent[0].shape == (N, N) and sent[0].tolist() == fx["conf_matrix"]  # the gather payload as before
    assert not ev._b_conf_matrix.any()
    ev_h = SemSegEvaluator("tiny_val_sem", mode="hungarian_matching", boundary_iou=True)  # untouched by the option
    ev_h.process(inputs, outputs)
    assert sorted(zip(ev_h.pred_det_cate, ev_h.pseudo_gt_cate)) == [tuple(v) for v in fx["semantic_votes"]]
    assert not ev_h._b_conf_matrix.any()


def test_min_with_a_nan_on_either_side(tiny_val_sem):
    """Python's min(iou, b_iou): a NaN first stays (nothing is smaller than it), a NaN second is never picked."""
    ev = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    conf, bconf = torch.zeros((N, N), dtype=torch.int64), torch.zeros((N, N), dtype=torch.int64)
    conf[1, 1], conf[1, 2], conf[2, 2] = 6, 2, 4  # classes 1 and 2 occur; class 3 never does: IoU-3 is NaN
    bconf[1, 1], bconf[3, 1], bconf[3, 3] = 1, 3, 5  # classes 1 and 3 have boundary counts; class 2 has none: BoundaryIoU-2 is NaN
    ev._conf_matrix, ev._b_conf_matrix = conf, bconf
    res = ev.evaluate()["sem_seg"]
    n1, n2, n3 = sse.SUPERCATEGORIES[0], sse.SUPERCATEGORIES[1], sse.SUPERCATEGORIES[2]
    assert res["IoU-" + n1] == pytest.approx(100 * 6 / 8) and res["BoundaryIoU-" + n1] == pytest.approx(100 * 1 / 4)
    assert res["min(IoU, B-Iou)-" + n1] == pytest.approx(25.0)
    assert res["IoU-" + n2] == pytest.approx(100 * 4 / 6) and res["BoundaryIoU-" + n2] != res["BoundaryIoU-" + n2]
    assert res["min(IoU, B-Iou)-" + n2] == res["IoU-" + n2]                  # min(x, nan) = x
    assert res["IoU-" + n3] != res["IoU-" + n3] and res["BoundaryIoU-" + n3] == pytest.approx(100 * 5 / 8)
    assert res["min(IoU, B-Iou)-" + n3] != res["min(IoU, B-Iou)-" + n3]      # min(nan, x) = nan
    assert res["BoundaryIoU-things"] != res["BoundaryIoU-things"]            # no boundary counts at all: NaN, not 0


def test_rank_sum(tiny_val_sem, monkeypatch):
    """Across ranks the boundary matrix is summed like the plain one."""
    fx, inputs, outputs, gts = tiny_val_sem
    half = len(inputs) // 2
    parts = []
    for sl in (slice(0, half), slice(half, None)):
        ev = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
        ev.process(inputs[sl], outputs[sl])
        parts.append(np.stack([ev._conf_matrix.numpy(), ev._b_conf_matrix.numpy()]))
    whole = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    whole.process(inputs, outputs)
    want = whole.evaluate()["sem_seg"]
    sent = []
    monkeypatch.setattr(sse, "gather_to_rank0", lambda obj: sent.append(obj) or [p.copy() for p in parts])
    ev = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    ev.process(inputs[:half], outputs[:half])
    res = ev.evaluate()["sem_seg"]
    assert len(sent) == 1 and sent[0].shape == (2, N, N) and np.array_equal(sent[0], parts[0])
    want_c, want_b = literal_matrices(outputs, gts)
    assert np.array_equal(ev._conf_matrix, want_c) and np.array_equal(ev._b_conf_matrix, want_b)
    assert list(res) == list(want) and all(same(res[k], want[k]) for k in want)
    monkeypatch.setattr(sse, "gather_to_rank0", lambda obj: None)  # every other rank
    other = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    other.process(inputs[half:], outputs[half:])
    assert other.evaluate() is None


def test_entry_point_flag():
    from u2seg_amd.engine.trainer import default_argument_parser

    assert default_argument_parser().parse_args([]).sem_seg_boundary_iou is False
    assert default_argument_parser().parse_args(["--sem-seg-boundary-iou"]).sem_seg_boundary_iou is True


def test_build_evaluator_passes_the_option(tiny_val_sem, tmp_path):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.evaluation import build_evaluator

    MetadataCatalog.get("tiny_val_sem").set(evaluator_type="sem_seg")
    cfg = get_cfg()
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path / "out")])
    assert build_evaluator(cfg, "tiny_val_sem")._boundary_iou is False
    assert build_evaluator(cfg, "tiny_val_sem", sem_seg_boundary_iou=True)._boundary_iou is True


def test_header_declares_and_library_exports_the_entry_points():
    import ctypes

    from u2seg_amd import _hip

    decl = _hip.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert decl["u2_semseg_boundary_confusion"] == (I, [P, P, P, I, I, I, I, P, P, P, LL, P])
    assert decl["u2_semseg_boundary_fused_cap"] == (I, [])
    assert decl["u2_semseg_boundary_scratch_bytes"] == (LL, [I, I, I])
    lib = ctypes.CDLL(_hip.lib_path())
    lib.u2_semseg_boundary_scratch_bytes.restype = LL
    cap = lib.u2_semseg_boundary_fused_cap()
    assert cap >= 31  # 800 x 1333 stays on the fused path
    assert lib.u2_semseg_boundary_scratch_bytes(150, 200, cap) == 0
    assert lib.u2_semseg_boundary_scratch_bytes(150, 200, cap + 1) == 2 * 150 * 200
    assert lib.u2_semseg_boundary_scratch_bytes(150, 200, 0) == -1
