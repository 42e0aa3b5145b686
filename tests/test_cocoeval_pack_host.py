"""The host half of the device engine of COCO AP (evaluation/cocoeval_ops.py): `pack` lays out exactly the groups
`cocoeval.prepare` makes, in the orders `compute_ious` and `accumulate` use; the interface around it.  No GPU needed."""
import json
import os

import numpy as np
import pytest

from tests import cocoeval_cases as cases
from u2seg_amd.evaluation import cocoeval as CE
from u2seg_amd.evaluation import cocoeval_ops as OPS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ("u2_cocoeval_workspace_bytes", "u2_cocoeval_workspace_layout", "u2_cocoeval_match", "u2_cocoeval_accumulate",
               "u2_cocoeval_lds_iou_entries", "u2_cocoeval_lds_max_gt", "u2_cocoeval_scan_chunk")


def problems():
    fx = json.load(open(os.path.join(GOLD, "cocoeval_golden.json")))
    return {"golden": (fx["dataset"], fx["results"]), "random": cases.random_problem(seed=3)}


@pytest.mark.parametrize("name", ["golden", "random"])
def test_pack_reproduces_the_groups(name):
    dataset, results = problems()[name]
    params, gts, dts = cases.groups(dataset, results)
    packed = OPS.pack(gts, dts, params)
    cells, lists = OPS.unpack(packed)
    want = cases.expected_cells(params, gts, dts)
    assert set(cells) == set(want)  # no cell for an empty (image, category), none missing
    assert len(want) < len(params.imgIds) * len(params.catIds)
    over = tied = 0
    for key, (dt_ids, gt_ids) in want.items():
        assert cells[key]["dt_ids"] == dt_ids, key  # the score order, ties in input order, and the cut
        assert cells[key]["gt_ids"] == gt_ids, key
        over += len(dts.get(key, [])) > params.maxDets[-1]
        tied += len(set(cells[key]["dt_scores"])) < len(dt_ids)
    assert tied > 0
    if name == "golden":
        assert over > 0  # a cell beyond the budget is cut
    want_lists = cases.expected_lists(params, want, dts)
    assert lists == want_lists
    score = {d["id"]: d["score"] for v in dts.values() for d in v}
    image = {d["id"]: k[0] for k, v in dts.items() for d in v}
    across = sum(score[a] == score[b] and image[a] != image[b] for ids in want_lists.values() for a, b in zip(ids, ids[1:]))
    assert across > 0  # ties across images are in the problem
    # the layout: cells in (category, image position) order, offsets consistent, one list range per category
    keys = [(int(c), int(i)) for c, i in zip(packed.cell_cat, packed.cell_img)]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    D, G = np.diff(packed.cell_dt_off), np.diff(packed.cell_gt_off)
    assert np.array_equal(np.diff(packed.cell_iou_off), D * G) and D.max() <= params.maxDets[-1]
    assert packed.cat_dt_off[-1] == packed.n_dt == D.sum() and sorted(packed.perm.tolist()) == list(range(packed.n_dt))
    assert np.array_equal(packed.dt_rank, np.arange(packed.n_dt) - packed.cell_dt_off[packed.dt_cell])


def test_pack_mask_form_indexes_the_pair_count_tables():
    fx = json.load(open(os.path.join(GOLD, "segm_eval_golden.json")))
    dataset, results = fx["dataset"], fx["results"]
    imgs = sorted(im["id"] for im in dataset["images"])
    pc = CE.host_pair_counts(dataset, results, imgs)
    host = CE.evaluate_segm(dataset, results, pair_counts=pc)
    rows, seen, areas = [], {}, []
    for r in results:
        k = seen.get(r["image_id"], 0)
        seen[r["image_id"]] = k + 1
        rows.append(k)
        areas.append(int(pc[r["image_id"]]["area_dt"][k]))
    params = host["params"]
    gts, dts = CE.prepare(dataset["annotations"], results, params, areas)
    packed = OPS.pack(gts, dts, params, pc, rows)
    n = 0
    for c in range(packed.n_cells):
        d, g = packed.cell_dets(c), packed.cell_gts(c)
        if d.stop == d.start or g.stop == g.start:
            continue
        inter = packed.inter[packed.dt_row[d][:, None] + packed.gt_col[g][None, :]]
        table = CE.mask_ious(inter, packed.dt_marea[d], packed.gt_marea[g], packed.gt_crowd[g])
        assert np.array_equal(table, host["ious"][packed.cell_key(c)])
        n += 1
    assert n > 20
    with pytest.raises(KeyError):
        OPS.pack(gts, dts, params, {k: v for k, v in pc.items() if k != packed.cell_key(0)[0]}, rows)


def test_pack_validates():
    dataset, results = cases.random_problem(seed=1, images=4)
    params, gts, dts = cases.groups(dataset, results)
    bad = [dict(r) for r in results]
    bad[0]["score"] = float("nan")
    with pytest.raises(ValueError, match="scores"):
        OPS.pack(gts, CE.prepare(dataset["annotations"], bad, params)[1], params)
    zero = [dict(a, id=0) if k == 0 else a for k, a in enumerate(dataset["annotations"])]
    with pytest.raises(ValueError, match="annotation id 0"):
        OPS.pack(CE.prepare(zero, results, params)[0], dts, params)
    params.iouThrs = np.linspace(0.5, 0.95, 11)
    with pytest.raises(ValueError, match="pairs"):
        OPS.pack(gts, dts, params)


def test_new_prototypes_are_declared():
    from u2seg_amd import _hip

    declared = _hip.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name


def test_parser_and_builder_take_the_engine():
    from u2seg_amd.engine.trainer import default_argument_parser

    assert default_argument_parser().parse_args([]).coco_eval == "host"
    assert default_argument_parser().parse_args(["--coco-eval", "device"]).coco_eval == "device"
    with pytest.raises(SystemExit):
        default_argument_parser().parse_args(["--coco-eval", "other"])


def test_device_engine_without_a_gpu_raises(monkeypatch, tmp_path):
    import torch

    from u2seg_amd.data import DatasetCatalog, MetadataCatalog, register_coco_instances
    from u2seg_amd.evaluation import COCOEvaluator, build_evaluator

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    dataset, results = cases.random_problem(seed=1, images=3)
    with pytest.raises(RuntimeError, match="needs a GPU"):
        CE.evaluate_bbox(dataset, results, engine="device")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        CE.evaluate_segm(dataset, results, pair_counts={}, engine="device")
    with pytest.raises(ValueError, match="engine"):
        CE.evaluate_bbox(dataset, results, engine="gpu")
    host = CE.evaluate_bbox(dataset, results)
    assert np.array_equal(host["precision"], CE.evaluate_bbox(dataset, results, engine="host")["precision"])
    json_file = str(tmp_path / "val.json")
    dataset["images"] = [dict(im, file_name="%d.jpg" % im["id"], height=256, width=256) for im in dataset["images"]]
    dataset["categories"] = [dict(c, name="c%d" % c["id"]) for c in dataset["categories"]]
    json.dump(dataset, open(json_file, "w"))
    for n in ("tiny_cocoeval_host",):
        if n in DatasetCatalog:
            DatasetCatalog.remove(n)
        if n in MetadataCatalog:
            MetadataCatalog.remove(n)
    register_coco_instances("tiny_cocoeval_host", {}, json_file, str(tmp_path))
    DatasetCatalog.get("tiny_cocoeval_host")
    assert COCOEvaluator("tiny_cocoeval_host", mode="eval")._coco_eval == "host"
    with pytest.raises(RuntimeError, match="needs a GPU"):
        COCOEvaluator("tiny_cocoeval_host", mode="eval", coco_eval="device")
    with pytest.raises(ValueError, match="coco_eval"):
        COCOEvaluator("tiny_cocoeval_host", mode="eval", coco_eval="gpu")
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    assert build_evaluator(cfg, "tiny_cocoeval_host", output_folder=str(tmp_path))._coco_eval == "host"
    with pytest.raises(RuntimeError, match="needs a GPU"):
        build_evaluator(cfg, "tiny_cocoeval_host", output_folder=str(tmp_path), coco_eval="device")
