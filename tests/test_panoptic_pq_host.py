"""Panoptic quality from segment-pair count tables (evaluation/panoptic_ops.py + pq.accumulate_counts) against the path it
has to reproduce exactly, pq.accumulate_image on the id maps: host side.  The PQStat dicts - counts and the float64 IoU sums -
are compared with ==."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import panoptic_pq_cases as cases
from u2seg_amd.evaluation import pq
from u2seg_amd.evaluation import panoptic_ops as ops

NINE = ("PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st")


def both_stats(samples, cats, table_from=ops.host_pair_counts):
    want, got = pq.PQStat(), pq.PQStat()
    for gt, gt_segs, pred, pred_segs in samples:
        pq.accumulate_image(want, gt, gt_segs, pred, pred_segs, cats)
        table = cases.gt_table_of(gt_segs)
        counts = table_from(pred, gt, table, cases.num_pred_cols(pred_segs))
        assert counts.dtype == np.int32 and counts.shape == (len(table) + 2, cases.num_pred_cols(pred_segs))
        assert int(counts.sum()) == pred.size
        pq.accumulate_counts(got, counts, table, gt_segs, pred_segs, cats)
    return want, got


def check_family(samples, cats):
    want, got = both_stats(samples, cats)
    assert cases.stat_dicts(got) == cases.stat_dicts(want)
    tp, fp, fn, excused = cases.outcome_counts(want, samples)
    assert tp >= 1 and fp >= 1 and fn >= 1 and excused >= 1, (tp, fp, fn, excused)  # not the equality of empty tables
    assert sum(want.iou.values()) > 0
    a = pq.pq_compute_arrays(samples, cats)
    b = pq.pq_compute_counts([(ops.host_pair_counts(p, g, cases.gt_table_of(gs), cases.num_pred_cols(ps)), cases.gt_table_of(gs), gs, ps)
                              for g, gs, p, ps in samples], cats)
    assert a == b


def test_hand_cases():
    samples, cats = cases.hand_cases()
    check_family(samples, cats)
    for s in samples:  # and one by one
        want, got = both_stats([s], cats)
        assert cases.stat_dicts(got) == cases.stat_dicts(want)
    res = pq.pq_compute_counts([(ops.host_pair_counts(samples[0][2], samples[0][0], [1, 2, 3], 31), [1, 2, 3], samples[0][1],
                                 samples[0][3])], cats)
    assert res["All"] == {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": 3}


def test_golden_maps_against_derived_ground_truth():
    samples, cats = cases.golden_cases()
    assert all(min(cases.gt_table_of(s[1])) > 65535 for s in samples)
    assert all(cases.big_id(9) in np.unique(s[0]) and cases.big_id(9) not in cases.gt_table_of(s[1]) for s in samples)
    check_family(samples, cats)
    for s in samples:
        want, got = both_stats([s], cats)
        assert cases.stat_dicts(got) == cases.stat_dicts(want)
        assert min(cases.outcome_counts(want, [s])) >= 1


@pytest.mark.parametrize("with_area", [False, True])
@pytest.mark.parametrize("h,w,cell", [(480, 640, 40), (200, 333, 30)])
def test_random_blocky_maps(h, w, cell, with_area):
    sample, cats = cases.blocky_case(h, w, cell, seed=h + int(with_area), with_area=with_area)
    check_family([sample], cats)


def test_png_pixels_and_id_maps_give_the_same_table():
    from u2seg_amd.data.pseudo_panoptic import id2rgb

    (gt, gt_segs, pred, pred_segs), _ = cases.blocky_case(50, 37, 7, seed=1, with_area=False)
    table, P = cases.gt_table_of(gt_segs), cases.num_pred_cols(pred_segs)
    a = ops.host_pair_counts(pred, gt, table, P)
    assert np.array_equal(a, ops.host_pair_counts(torch.from_numpy(pred), id2rgb(gt), table, P))
    assert np.array_equal(a, ops.host_pair_counts(pred.astype(np.int32), gt.astype(np.int32), table, P))
    assert a[0].sum() == (gt == 0).sum() and a[-1].sum() == (~np.isin(gt, [0] + table)).sum() > 0
    empty = ops.host_pair_counts(pred, gt, [], P)  # G = 0: void and "other"
    assert empty.shape == (2, P) and empty[0].sum() == (gt == 0).sum() and empty.sum() == gt.size


def test_erased_columns_equal_zeroed_pixels():
    """Dropping an erased segment on the table (its column moved into column 0) == zeroing its pixels in the map."""
    (gt, gt_segs, pred, pred_segs), cats = cases.blocky_case(120, 90, 15, seed=2, with_area=False)
    table, P = cases.gt_table_of(gt_segs), cases.num_pred_cols(pred_segs)
    counts = ops.host_pair_counts(pred, gt, table, P)
    erased = [1, 7]
    counts[:, 0] += counts[:, erased].sum(axis=1)
    counts[:, erased] = 0
    zeroed = np.where(np.isin(pred, erased), 0, pred)
    assert np.array_equal(counts, ops.host_pair_counts(zeroed, gt, table, P))
    kept = [s for s in pred_segs if s["id"] not in erased]
    want, got = pq.PQStat(), pq.PQStat()
    pq.accumulate_image(want, gt, gt_segs, zeroed, kept, cats)
    pq.accumulate_counts(got, counts, table, gt_segs, kept, cats)
    assert cases.stat_dicts(got) == cases.stat_dicts(want)


def test_key_errors_and_value_errors():
    samples, cats = cases.hand_cases()
    gt, gt_segs, pred, pred_segs = samples[1]
    table, P = [1, 2, 3], 41
    counts = ops.host_pair_counts(pred, gt, table, P)
    for segs, categories, match in ((pred_segs[:2], cats, "not in segments_info"),          # pixels without an entry
                                    (pred_segs, {1: cats[1], 7: cats[7]}, "unknown category"),
                                    (pred_segs + [{"id": 35, "category_id": 1}], cats, "not in the predicted png")):
        with pytest.raises(KeyError, match=match):
            pq.accumulate_counts(pq.PQStat(), counts, table, gt_segs, segs, categories)
        with pytest.raises(KeyError, match=match):
            pq.accumulate_image(pq.PQStat(), gt, gt_segs, pred, segs, categories)
    with pytest.raises(KeyError, match="segment id 40 is in the predicted png but not in segments_info"):
        ops.host_pair_counts(pred, gt, table, 40)  # a predicted id outside the table's columns
    with pytest.raises(ValueError, match="my image.*size"):
        ops.host_pair_counts(pred, gt[:, :9], table, P, name="my image")
    with pytest.raises(ValueError, match="my image.*type"):
        ops.host_pair_counts(pred, gt.astype(np.float32), table, P, name="my image")
    with pytest.raises(ValueError, match="my image.*shape"):
        ops.host_pair_counts(pred, np.zeros((10, 10, 4), dtype=np.uint8), table, P, name="my image")
    # the device wrapper's checks of the ground truth (host code: no device needed)
    with pytest.raises(ValueError, match="img 3.*size"):
        ops._checked_gt(np.zeros((10, 9, 3), dtype=np.uint8), (10, 10), "img 3")
    with pytest.raises(ValueError, match="img 3.*type"):
        ops._checked_gt(np.zeros((10, 10), dtype=np.int64), (10, 10), "img 3")
    with pytest.raises(ValueError, match="img 3.*shape"):
        ops._checked_gt(np.zeros((10, 10, 4), dtype=np.uint8), (10, 10), "img 3")
    with pytest.raises(ValueError):
        pq.accumulate_counts(pq.PQStat(), counts[:-1], table, gt_segs, pred_segs, cats)


def run_evaluator(name, inputs, outputs, out_dir, mode_pq):
    from u2seg_amd.evaluation import COCOPanopticEvaluator

    ev = COCOPanopticEvaluator(name, str(out_dir), pq=mode_pq)
    ev.process(inputs[:2], outputs[:2])
    ev.process(inputs[2:], outputs[2:])
    return ev, ev.evaluate()["panoptic_seg"]


@pytest.mark.parametrize("mode", ["eval", "hungarian_matching"])
def test_evaluator_counts_equals_files(tmp_path, monkeypatch, mode):
    name = "pq_tiny_" + tmp_path.name + mode
    inputs, outputs, fx = cases.write_tiny_dataset(str(tmp_path), name)
    monkeypatch.chdir(tmp_path)
    if mode == "eval":
        cases.write_mapping_files(fx)
    ev_f, files = run_evaluator(name, inputs, outputs(), tmp_path / "files", "files")
    ev_c, counts = run_evaluator(name, inputs, outputs(), tmp_path / "counts", "counts")
    assert ev_f.mode == ev_c.mode == mode
    try:
        import panopticapi  # noqa: F401
        extra = set()
    except ImportError:
        extra = {"pq_implementation"}
        assert files["pq_implementation"] == "u2seg_amd.evaluation.pq"
    assert set(files) == {"predictions_json", "num_images"} | set(NINE) | extra  # what it returned before: no new keys
    for key in NINE:
        assert counts[key] == files[key], key
    assert files["num_images"] == counts["num_images"] == 3
    assert cases.read_tree(tmp_path / "files") == cases.read_tree(tmp_path / "counts")
    assert sorted(os.listdir(tmp_path / "counts")) == ["000001.png", "000002.png", "000003.png", "predictions.json"]
    if mode == "eval":
        assert counts["pq_implementation"] == "u2seg_amd.evaluation.pq (device counts)"
        # a segment was erased (cluster 298 has no mapping) and the comparison is not one of empty tables
        assert all(len(p["segments_info"]) == 3 for p in json.load(open(counts["predictions_json"]))["annotations"])
        assert 0 < files["PQ"] < 100 and files["RQ"] > 0


def test_evaluator_counts_errors(tmp_path, monkeypatch):
    from u2seg_amd.data import MetadataCatalog
    from u2seg_amd.evaluation import COCOPanopticEvaluator

    name = "pq_tiny_" + tmp_path.name
    inputs, outputs, fx = cases.write_tiny_dataset(str(tmp_path), name)
    monkeypatch.chdir(tmp_path)
    cases.write_mapping_files(fx)
    ev = COCOPanopticEvaluator(name, None, pq="counts")
    ev.process(inputs[:2], outputs()[:2])
    assert all("pq_counts" in p and "pq_gt_table" in p for p in ev._predictions)
    with pytest.raises(KeyError, match="no prediction for the image with id 3"):
        ev.evaluate()
    with pytest.raises(ValueError):
        COCOPanopticEvaluator(name, None, pq="device")
    MetadataCatalog.get(name + "_nojson").set(panoptic_json=str(tmp_path / "nothing.json"), panoptic_root=str(tmp_path),
                                              thing_dataset_id_to_contiguous_id={})
    with pytest.raises(FileNotFoundError):
        COCOPanopticEvaluator(name + "_nojson", None, pq="counts")
    MetadataCatalog.get(name + "_nodir").set(panoptic_json=MetadataCatalog.get(name).panoptic_json,
                                             panoptic_root=str(tmp_path / "nothing"), thing_dataset_id_to_contiguous_id={})
    with pytest.raises(FileNotFoundError):
        COCOPanopticEvaluator(name + "_nodir", None, pq="counts")
    COCOPanopticEvaluator(name + "_nodir", None)  # "files" finds out at the end, as before
    ev = COCOPanopticEvaluator(name, None, pq="counts")  # ground truth of another size than the prediction
    out = outputs()[:1]
    out[0]["panoptic_seg"] = (out[0]["panoptic_seg"][0][:, :-1], out[0]["panoptic_seg"][1])
    with pytest.raises(ValueError, match="000001"):
        ev.process(inputs[:1], out)


def test_command_line_and_build_evaluator(tmp_path, monkeypatch):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import MetadataCatalog
    from u2seg_amd.engine.trainer import default_argument_parser
    from u2seg_amd.evaluation import build_evaluator

    assert default_argument_parser().parse_args([]).panoptic_pq == "files"
    assert default_argument_parser().parse_args(["--panoptic-pq", "counts"]).panoptic_pq == "counts"
    with pytest.raises(SystemExit):
        default_argument_parser().parse_args(["--panoptic-pq", "other"])
    name = "pq_tiny_" + tmp_path.name
    cases.write_tiny_dataset(str(tmp_path), name)
    MetadataCatalog.get(name).set(evaluator_type="coco_panoptic_seg")
    monkeypatch.chdir(tmp_path)
    import u2seg_amd.evaluation as evaluation

    class Stub(evaluation.DatasetEvaluator):  # the semantic and instance evaluators need files this test does not lay out
        def __init__(self, *args, **kwargs):
            pass

    monkeypatch.setattr(evaluation, "SemSegEvaluator", Stub)
    monkeypatch.setattr(evaluation, "COCOEvaluator", Stub)
    cfg = get_cfg()
    cfg.merge_from_list(["OUTPUT_DIR", str(tmp_path / "out")])
    assert build_evaluator(cfg, name, panoptic_pq="counts")._evaluators[-1]._pq == "counts"
    assert build_evaluator(cfg, name)._evaluators[-1]._pq == "files"


def test_header_declares_and_library_exports_the_entry_point():
    from u2seg_amd import _hip

    decl = _hip.declared_symbols()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert decl["u2_panoptic_pair_counts"] == (I, [P, I, P, P])
    assert decl["u2_panoptic_pair_lds_ints"] == (I, [])
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "u2_panoptic_pair_counts") and hasattr(lib, "u2_panoptic_pair_lds_ints")
    lib.u2_panoptic_pair_lds_ints.restype = ctypes.c_int
    assert lib.u2_panoptic_pair_lds_ints() == ops.lds_table_ints() == 15 * 1024
    assert ctypes.sizeof(ops._PairImage) == 56  # U2PanopticPairImage: four pointers, six ints
