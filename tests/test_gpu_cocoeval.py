"""COCO AP matching and accumulation on the GPU (u2seg_amd/csrc/cocoeval.hip through evaluation/cocoeval_ops.py) against the
host engine, evaluation/cocoeval.py.  Inputs are exact and every output is an integer or one correctly rounded float64
operation on exact values, so every comparison with the host is ==; the only tolerance is the host engine's own against the
reference's tables (1e-12, tests/test_evaluation.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import cocoeval_cases as cases
from u2seg_amd.data import rle

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ("u2_cocoeval_workspace_bytes", "u2_cocoeval_workspace_layout", "u2_cocoeval_match", "u2_cocoeval_accumulate",
               "u2_cocoeval_lds_iou_entries", "u2_cocoeval_lds_max_gt", "u2_cocoeval_scan_chunk")
BIG = 1 << 40  # annotation ids beyond 32 bits


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.evaluation import cocoeval, cocoeval_ops

    _hip.load()
    return cocoeval, cocoeval_ops


def compare(E, dataset, results, max_dets=(1, 10, 100)):
    """Both engines on one problem; IoU tables, every cell's record for every area range and the three tables are equal.
    Returns (host accumulation, device accumulation with "records" and "packed")."""
    CE, OPS = E
    params, gts, dts = cases.groups(dataset, results, max_dets)
    ious = CE.compute_ious(gts, dts, params)
    evals = CE.evaluate_images(gts, dts, ious, params)
    host = CE.accumulate(evals, params)
    dev = OPS.evaluate(gts, dts, params, records=True)
    packed, rec = dev["packed"], dev["records"]
    assert packed.n_cells == sum(bool(gts.get(k)) or bool(dts.get(k)) for k in ious)
    for c in range(packed.n_cells):
        img, cat = packed.cell_key(c)
        D, G = len(dts.get((img, cat), [])[: params.maxDets[-1]]), len(gts.get((img, cat), []))
        assert np.array_equal(OPS.cell_ious(packed, rec, c), np.asarray(ious[img, cat], dtype=np.float64).reshape(D, G)), (img, cat)
        k, i = params.catIds.index(cat), params.imgIds.index(img)
        for a in range(len(params.areaRng)):
            want, got = evals[k][a][i], OPS.cell_record(packed, rec, c, a)
            for name, x, y in zip(("matched", "detection ignored", "scores", "ground truth ignored"), want, got):
                assert np.array_equal(x, y), (img, cat, a, name)
            assert rec["cell_valid"][c, a] == int((~want[3]).sum())
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(host[name], dev[name]), name
    return host, dev


def test_library_exports_new_prototypes(E):
    import ctypes

    from u2seg_amd import _hip

    lib = ctypes.CDLL(_hip.lib_path())
    declared = _hip.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert _hip.call_nostream("u2_abi_version") == 1


def hand_made():
    anns, results = [], []

    def gt(img, box, crowd=0, area=None, cat=1):
        anns.append({"id": BIG + len(anns) + 1, "image_id": img, "category_id": cat, "bbox": list(box), "iscrowd": crowd,
                     "area": box[2] * box[3] if area is None else area})

    def dt(img, box, score, cat=1):
        results.append({"image_id": img, "category_id": cat, "bbox": list(box), "score": score})

    gt(1, [0, 0, 40, 40]); gt(1, [50, 50, 20, 20])                                  # D = 0, G > 0
    dt(2, [0, 0, 40, 40], 0.9); dt(2, [5, 5, 100, 100], 0.8)                        # D > 0, G = 0
    gt(3, [0, 0, 100, 100], crowd=1); gt(3, [200, 200, 30, 30])                     # a crowd region matched three times
    dt(3, [10, 10, 20, 20], 0.9); dt(3, [40, 40, 30, 30], 0.8); dt(3, [60, 10, 20, 40], 0.7); dt(3, [200, 200, 30, 30], 0.6)
    gt(4, [0, 0, 20, 30]); gt(4, [0, 0, 20, 20], crowd=1)                           # regular match (IoU 2/3) kept, crowd has IoU 1
    dt(4, [0, 0, 20, 20], 0.9)
    gt(5, [0, 0, 30, 30], area=2000); gt(5, [100, 0, 20, 20])                       # "area" decides the range, not the box
    dt(5, [0, 0, 30, 30], 0.9); dt(5, [100, 0, 20, 20], 0.8); dt(5, [100, 0, 20, 22], 0.7)
    gt(6, [0, 0, 32, 32]); gt(6, [50, 50, 96, 96])                                  # areas exactly 32^2 and 96^2
    dt(6, [0, 0, 32, 32], 0.9); dt(6, [50, 50, 96, 96], 0.8); dt(6, [300, 300, 32, 32], 0.7); dt(6, [500, 500, 96, 96], 0.6)
    gt(7, [0, 0, 10, 20]); gt(7, [100, 0, 10, 40]); gt(7, [200, 0, 10, 20])         # IoU exactly 0.5, 0.75 and 0.95
    dt(7, [0, 0, 10, 10], 0.9); dt(7, [100, 0, 10, 30], 0.8); dt(7, [200, 0, 10, 19], 0.7)
    gt(8, [0, 0, 10, 10])                                                           # touching boxes: w = 0, h = 0
    dt(8, [10, 0, 10, 10], 0.9); dt(8, [0, 10, 10, 10], 0.8); dt(8, [10, 10, 5, 5], 0.7)
    for k in range(6):                                                              # 103 detections: beyond the budget
        gt(9, [20 * k, 0, 16, 16 + k])
    for k in range(103):
        dt(9, [20 * (k % 6) + (k // 6) % 3, 0, 16, 16 + (k % 6)], 0.999 - 0.004 * ((k * 37) % 103))
    gt(10, [0, 0, 20, 20]); gt(10, [0, 0, 20, 24]); gt(10, [0, 0, 24, 20])          # equal scores inside a cell
    for k in range(6):
        dt(10, [0, 0, 20 + 2 * (k % 3), 20 + 4 * (k // 3)], 0.5)
    dataset = {"images": [{"id": i} for i in range(1, 11)], "categories": [{"id": 1}], "annotations": anns}
    return dataset, results


def test_hand_made_cells(E):
    CE, OPS = E
    dataset, results = hand_made()
    host, dev = compare(E, dataset, results)
    packed, rec = dev["packed"], dev["records"]
    cell = {packed.cell_key(c)[0]: c for c in range(packed.n_cells)}
    assert np.diff(packed.cell_dt_off)[cell[1]] == 0 and np.diff(packed.cell_gt_off)[cell[2]] == 0
    assert np.diff(packed.cell_dt_off)[cell[9]] == 100
    m3 = OPS.cell_record(packed, rec, cell[3], 0)[0]
    assert (m3[0, :3] == BIG + 3).all() and m3[0, 3] == BIG + 4  # the crowd region three times, ids beyond 32 bits
    m4 = OPS.cell_record(packed, rec, cell[4], 0)[0]
    assert m4[0, 0] == BIG + 5 and m4[-1, 0] == BIG + 6  # the regular one while its IoU passes, then the crowd region
    ign5 = [OPS.cell_record(packed, rec, cell[5], a)[3].tolist() for a in range(4)]
    assert ign5 == [[False, False], [False, True], [False, True], [True, True]]
    for a, want in ((1, [False, True]), (2, [False, False]), (3, [False, True])):  # 32^2 is small and medium, 96^2 medium and large
        assert OPS.cell_record(packed, rec, cell[6], a)[3].tolist() == want, a
    iou7 = OPS.cell_ious(packed, rec, cell[7])
    assert iou7[0, 0] == 0.5 and iou7[1, 1] == 0.75 and iou7[2, 2] == 0.95
    m7 = OPS.cell_record(packed, rec, cell[7], 0)[0]
    assert m7[0, 0] > 0 and m7[1, 0] == 0 and m7[5, 1] > 0 and m7[6, 1] == 0
    assert not OPS.cell_ious(packed, rec, cell[8]).any()
    assert host["recall"][0, 0, 0, 2] > host["recall"][-1, 0, 0, 2] > 0


def sized_cells(shapes, seed):
    """One image per (D, G): ground truth on an 8-pixel grid, detections on or next to one of them (or far away), distinct
    scores in random order, 10 % crowd regions."""
    rs = np.random.RandomState(seed)
    anns, results = [], []
    for img, (D, G) in enumerate(shapes, start=1):
        first = len(anns)
        for g in range(G):
            w, h = int(rs.choice([16, 24, 40, 96])), int(rs.choice([16, 24, 40, 96]))
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "bbox": [8 * (g % 16), 8 * (g // 16), w, h],
                         "area": w * h, "iscrowd": int(rs.rand() < 0.1)})
        scores = rs.permutation(D)
        for d in range(D):
            if G and rs.rand() < 0.8:
                x, y, w, h = anns[first + int(rs.randint(G))]["bbox"]
                x, h = x + 4 * int(rs.randint(0, 2)), h + 8 * int(rs.randint(0, 2))
            else:
                x, y, w, h = 8 * int(rs.randint(0, 30)), 8 * int(rs.randint(0, 30)), 24, 24
            results.append({"image_id": img, "category_id": 1, "bbox": [x, y, w, h], "score": (1 + int(scores[d])) / (D + 1)})
    dataset = {"images": [{"id": i + 1} for i in range(len(shapes))], "categories": [{"id": 1}], "annotations": anns}
    return dataset, results


def test_sizes_across_the_lds_limits(E):
    """A cell is matched from LDS when its IoU table has at most 1024 entries AND it has at most 64 ground truth; any other
    cell reads its table and its taken-flags from global memory.  D' = 100 with G = 1 / 63 / 64 / 65 / 130 (only G = 1 fits),
    and around both limits: 16 x 64 = 1024 entries (LDS), 17 x 61 = 1037 (global), 10 x 64 (LDS), 10 x 65 and 10 x 102
    (global although the table fits)."""
    CE, OPS = E
    assert OPS.lds_iou_entries() == 1024 and OPS.lds_max_gt() == 64
    shapes = [(100, 1), (100, 63), (100, 64), (100, 65), (100, 130), (16, 64), (17, 61), (10, 64), (10, 65), (10, 102)]
    dataset, results = sized_cells(shapes, seed=5)
    host, dev = compare(E, dataset, results)
    packed = dev["packed"]
    path = {packed.cell_key(c)[0]: int(dev["records"]["path"][c]) for c in range(packed.n_cells)}
    assert [path[i + 1] for i in range(len(shapes))] == [0, 1, 1, 1, 1, 0, 1, 0, 1, 1]
    assert (host["precision"][0, :, 0, 0, 2] > 0).any()


def accumulation_problem():
    """Categories: 1 = 40 images x 80 detections (a list of 3200: 12 scan chunks of 256 and a half), 2 = ground truth without
    detections, 3 = detections without ground truth, 4 = a few of both.  Scores in hundredths: ties across images.  Image ids
    unsorted and not contiguous, results shuffled."""
    rs = np.random.RandomState(11)
    img_ids = [int(v) for v in rs.permutation(np.arange(5, 5 + 9 * 40, 9))]
    anns, results = [], []
    for img in img_ids:
        first = len(anns)
        for g in range(rs.randint(1, 5)):
            w, h = int(rs.choice([16, 40, 120])), int(rs.choice([16, 40, 120]))
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 1, "bbox": [40 * g, 0, w, h], "area": w * h,
                         "iscrowd": int(rs.rand() < 0.05)})
        last = len(anns)
        for d in range(80):
            x, y, w, h = anns[int(rs.randint(first, last))]["bbox"]
            results.append({"image_id": img, "category_id": 1, "bbox": [x + 4 * int(rs.randint(0, 3)), y, w, h + 4 * int(rs.randint(0, 3))],
                            "score": float(np.round(rs.rand(), 2))})
        if rs.rand() < 0.3:
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 2, "bbox": [0, 0, 50, 50], "area": 2500, "iscrowd": 0})
        if rs.rand() < 0.3:
            results.append({"image_id": img, "category_id": 3, "bbox": [0, 0, 50, 50], "score": float(np.round(rs.rand(), 2))})
        if rs.rand() < 0.5:
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": 4, "bbox": [0, 0, 60, 60], "area": 3600, "iscrowd": 0})
            results.append({"image_id": img, "category_id": 4, "bbox": [0, 0, 60, 60 + 6 * int(rs.randint(0, 4))],
                            "score": float(np.round(rs.rand(), 1))})
    results = [results[i] for i in rs.permutation(len(results))]
    dataset = {"images": [{"id": i} for i in img_ids], "categories": [{"id": c} for c in (1, 2, 3, 4)], "annotations": anns}
    return dataset, results


def test_accumulation(E):
    CE, OPS = E
    assert OPS.scan_chunk() == 256
    dataset, results = accumulation_problem()
    host, dev = compare(E, dataset, results)
    packed = dev["packed"]
    n1 = int(packed.cat_dt_off[1] - packed.cat_dt_off[0])
    assert n1 == 3200 and n1 > OPS.scan_chunk() and n1 % OPS.scan_chunk() != 0
    p, r = dev["precision"], dev["recall"]
    assert (p[:, :, 1, 0, :] == 0).all() and (r[:, 1, 0, :] == 0).all()     # ground truth, no detections
    assert (p[:, :, 2] == -1).all() and (r[:, 2] == -1).all() and (dev["scores"][:, :, 2] == -1).all()  # no ground truth
    assert len({float(r[0, 0, 0, m]) for m in range(3)}) == 3 and not np.array_equal(p[..., 1], p[..., 2])  # the budgets differ
    s = np.concatenate([packed.dt_score[packed.perm[packed.cat_dt_off[k]: packed.cat_dt_off[k + 1]]] for k in range(4)])
    assert len(np.unique(s)) < len(s) // 4  # ties, across images
    assert list(packed.img_ids) == sorted(packed.img_ids) and np.any(np.diff(packed.img_ids) > 1)
    full = CE.evaluate_bbox(dataset, results, engine="device")
    assert full["stats"] == CE.evaluate_bbox(dataset, results)["stats"]


def test_seeded_random_problem_twice(E):
    """30 images, 5 categories, 0-120 detections per image on an integer grid (IoU ties), scores in hundredths, 8 % crowd."""
    CE, OPS = E
    dataset, results = cases.random_problem(seed=0, images=30, cats=5, max_dets_per_image=120, crowd=0.08, score_decimals=2)
    host, dev = compare(E, dataset, results)
    assert (host["precision"] > 0).sum() > 1000
    a, b = (CE.evaluate_bbox(dataset, results, engine="device") for _ in range(2))
    want = CE.evaluate_bbox(dataset, results)
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(a[name], b[name]) and np.array_equal(a[name], want[name]), name
    assert a["stats"] == b["stats"] == want["stats"]
    before = dict(OPS.counters)
    CE.evaluate_bbox(dataset, results, engine="device")
    assert {k: OPS.counters[k] - before[k] for k in before} == {"host_syncs": 1, "d2h_transfers": 1, "h2d_transfers": 1}


def test_golden_bbox(E):
    CE, OPS = E
    fx = json.load(open(os.path.join(GOLD, "cocoeval_golden.json")))
    ref = np.load(os.path.join(GOLD, "cocoeval_golden.npz"))
    host, dev = CE.evaluate_bbox(fx["dataset"], fx["results"]), CE.evaluate_bbox(fx["dataset"], fx["results"], engine="device")
    assert set(host) == set(dev) and host["stats"] == dev["stats"]
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(host[name], dev[name]), name
        np.testing.assert_allclose(dev[name], ref[name], rtol=0, atol=1e-12)


def test_golden_segm(E):
    CE, OPS = E
    fx = json.load(open(os.path.join(GOLD, "segm_eval_golden.json")))
    ref = np.load(os.path.join(GOLD, "segm_eval_golden.npz"))
    results = [{k: v for k, v in r.items() if k != "bbox"} for r in fx["results"]]
    pc = CE.host_pair_counts(fx["dataset"], results, [im["id"] for im in fx["dataset"]["images"]])
    host = CE.evaluate_segm(fx["dataset"], results, pair_counts=pc)
    dev = CE.evaluate_segm(fx["dataset"], results, pair_counts=pc, engine="device")
    assert set(host) == set(dev) and host["stats"] == dev["stats"]
    for name in ("precision", "recall", "scores"):
        assert np.array_equal(host[name], dev[name]), name
        np.testing.assert_allclose(dev[name], ref[name], rtol=0, atol=1e-12)
    assert set(host["ious"]) == set(dev["ious"])
    for key, table in host["ious"].items():
        got = dev["ious"][key]
        assert len(table) == len(got) and np.array_equal(np.asarray(table, dtype=np.float64).reshape(-1), np.asarray(got).reshape(-1)), key


def test_evaluator_device_equals_host(E, tmp_path, monkeypatch):
    """COCOEvaluator(tasks=("bbox", "segm"), mode="eval") on four images of the segm fixture: coco_eval="device" returns the
    dict of coco_eval="host", NaNs in the same places."""
    from tests.test_mask_eval_host import same_with_nans
    from u2seg_amd.data import DatasetCatalog, MetadataCatalog, register_coco_instances
    from u2seg_amd.evaluation import COCOEvaluator, hungarian
    from u2seg_amd.structures import Boxes, Instances

    fx = json.load(open(os.path.join(GOLD, "segm_eval_golden.json")))
    ids = [1, 4, 7, 22]
    images = [dict(im, file_name="%06d.jpg" % im["id"]) for im in fx["dataset"]["images"] if im["id"] in ids]
    cats = [{"id": c["id"], "name": "c%d" % c["id"]} for c in fx["dataset"]["categories"]]
    anns = [a for a in fx["dataset"]["annotations"] if a["image_id"] in ids]
    names = {"tiny_cocoeval_gpu": anns, "tiny_cocoeval_gpu_nan": [x for x in anns if x["category_id"] != 9]}  # no ground truth of c9: NaN
    for name, kept in names.items():
        json_file = str(tmp_path / (name + ".json"))
        json.dump({"images": images, "annotations": kept, "categories": cats}, open(json_file, "w"))
        if name in DatasetCatalog:
            DatasetCatalog.remove(name)
        if name in MetadataCatalog:
            MetadataCatalog.remove(name)
        register_coco_instances(name, {}, json_file, str(tmp_path))
        DatasetCatalog.get(name)
    monkeypatch.chdir(tmp_path)
    contiguous = MetadataCatalog.get("tiny_cocoeval_gpu").thing_dataset_id_to_contiguous_id
    hungarian.save_mapping({c + 100: (-1 if c == 9 else contiguous[c]) for c in contiguous}, "./hungarian_matching/instance_mapping.json")
    inputs, outputs = [], []
    for im in images:
        rs = [r for r in fx["results"] if r["image_id"] == im["id"]]
        inst = Instances((im["height"], im["width"]))
        b = torch.tensor([r["bbox"] for r in rs], dtype=torch.float32).reshape(-1, 4)
        inst.pred_boxes = Boxes(torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], dim=1))
        inst.scores = torch.tensor([r["score"] for r in rs], dtype=torch.float32)
        inst.pred_classes = torch.tensor([r["category_id"] + 100 for r in rs], dtype=torch.int64)
        masks = [rle.decode(r["segmentation"]) for r in rs]
        inst.pred_masks = torch.from_numpy(np.stack(masks).astype(bool)) if masks else torch.zeros((0, im["height"], im["width"]), dtype=torch.bool)
        inputs.append({"image_id": im["id"], "height": im["height"], "width": im["width"]})
        outputs.append({"instances": inst})
    for name in names:
        out = {}
        for engine in ("host", "device"):
            ev = COCOEvaluator(name, output_dir="out_" + engine, mode="eval", tasks=("bbox", "segm"), coco_eval=engine)
            ev.process(inputs, [{"instances": o["instances"].to("cuda:0")} for o in outputs])
            out[engine] = ev.evaluate()
        assert set(out["host"]) == set(out["device"]) == {"bbox", "segm"}
        same_with_nans(out["host"]["bbox"], out["device"]["bbox"])
        same_with_nans(out["host"]["segm"], out["device"]["segm"])
        assert out["device"]["segm"]["AP"] > 0 and out["device"]["bbox"]["AP"] > 0
        assert any(v != v for v in out["device"]["segm"].values()) == name.endswith("nan")
