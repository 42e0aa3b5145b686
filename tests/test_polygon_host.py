"""Polygon ground truth on the host: data/polygon.py (cocoapi's polygon -> RLE conversion restated) against the known
answers of tests/golden/polygon_known_answers.json and against a literal sort / merge restatement, the integer identities the
device kernel uses, the bitmask mapper, and the opt-in route through mask_ops, cocoeval, COCOEvaluator and tools/train_net.py.
Everything is integers: every comparison is ==."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import polygon_cases as PC
from u2seg_amd.data import DatasetCatalog, MetadataCatalog, polygon, register_coco_instances, rle
from u2seg_amd.evaluation import COCOEvaluator, build_evaluator, hungarian
from u2seg_amd.structures import Boxes, Instances


def expected_mask(case):
    h, w = case["h"], case["w"]
    return rle.decode({"size": [h, w], "counts": case["counts"]})


@pytest.mark.parametrize("case", PC.known_answers(), ids=lambda c: c["name"])
def test_known_answers(case):
    h, w, polys = case["h"], case["w"], case["polygons"]
    mask = polygon.polygons_to_bitmask(polys, h, w)
    assert mask.dtype == np.bool_ and mask.shape == (h, w)
    assert int(mask.sum()) == case["area"]
    if case["counts"] is not None:
        assert sum(case["counts"]) == h * w
        assert np.array_equal(mask, expected_mask(case).astype(bool))
    for y, x in case["set"]:
        assert mask[y, x]
    for y, x in case["clear"]:
        assert not mask[y, x]
    if case["crossings"] is not None:
        assert [len(polygon.polygon_crossings(p, h, w)) for p in polys] == case["crossings"]
    if len(polys) == 1:
        assert np.array_equal(polygon.polygon_to_mask(polys[0], h, w), mask.astype(np.uint8))
        assert np.array_equal(PC.literal_mask(polys[0], h, w), mask.astype(np.uint8))
    r = polygon.polygons_to_rle(polys, h, w)
    assert r == rle.encode(mask) and isinstance(r["counts"], str)
    assert np.array_equal(rle.decode(r), mask.astype(np.uint8)) and rle.area(r) == case["area"]


def test_argument_checks_and_empty_list():
    assert not polygon.polygons_to_bitmask([], 4, 5).any() and polygon.polygons_to_bitmask([], 4, 5).shape == (4, 5)
    assert rle.area(polygon.polygons_to_rle([], 4, 5)) == 0
    for bad in ([], [1.0], [1, 2, 3]):
        with pytest.raises(ValueError):
            polygon.polygon_to_mask(bad, 4, 5)
    a = polygon.polygon_crossings([1, 1, 4, 1, 4, 3, 1, 3], 5, 6)
    assert a.dtype == np.int64 and sorted(a.tolist()) == [6, 8, 11, 13, 16, 18]


def test_parity_form_equals_sort_merge_form():
    """2 001 seeded random polygons: the prefix parity of the crossings == the literal sort / difference / merge of zero-length
    runs, for integer, fifth-of-a-pixel and arbitrary coordinates, inside and up to 4 px outside the image."""
    nonempty = 0
    for xy, h, w in PC.random_polygons(2001, seed=1):
        got = polygon.polygon_to_mask(xy, h, w)
        assert np.array_equal(got, PC.literal_mask(xy, h, w)), (xy, h, w)
        nonempty += bool(got.any())
    assert nonempty > 1000


def test_integer_identities():
    """What csrc/polygon.hip computes in integers equals the float form of the definition, u', v' = -60 .. 400."""
    vals = np.arange(-60, 401, dtype=np.int64)
    xd = (vals.astype(np.float64) + .5) / 5.0 - .5
    integral = np.floor(xd) == xd
    assert np.array_equal(integral, vals % 5 == 2)  # numpy's % is the floor-mod
    assert np.array_equal(xd[integral].astype(np.int64), (vals[integral] - 2) // 5)
    for h in (1, 7, 64, 65):
        yd = np.ceil(np.clip((vals.astype(np.float64) + .5) / 5.0 - .5, 0, h)).astype(np.int64)
        assert np.array_equal(yd, np.clip((vals + 2) // 5, 0, h)), h


def test_bitmask_mapper_rasterises_polygons():
    from u2seg_amd.data import detection_utils as utils
    from u2seg_amd.data.detection_utils import BoxMode

    polys = [[3.2, 2.1, 30.7, 5.5, 18.0, 27.9], [10, 10, 25, 10, 25, 20, 10, 20]]
    mask = np.zeros((40, 50), dtype=np.uint8)
    mask[5:9, 7:30] = 1
    annos = [{"bbox": [3, 2, 31, 28], "bbox_mode": BoxMode.XYXY_ABS, "category_id": 2, "segmentation": [np.asarray(p) for p in polys]},
             {"bbox": [7, 5, 30, 9], "bbox_mode": BoxMode.XYXY_ABS, "category_id": 1, "segmentation": rle.encode(mask)}]
    inst = utils.annotations_to_instances(annos, (40, 50), mask_format="bitmask")
    got = inst.gt_masks.tensor.numpy()
    assert got.dtype == np.bool_ and got.shape == (2, 40, 50)
    assert np.array_equal(got[0], polygon.polygons_to_bitmask(polys, 40, 50)) and got[0].sum() > 300
    assert np.array_equal(got[1], mask.astype(bool))
    with pytest.raises(NotImplementedError, match="MASK_FORMAT 'polygon'"):
        utils.annotations_to_instances(annos, (40, 50), mask_format="polygon")


def test_pair_counts_and_evaluate_segm_with_polygons():
    """Polygon ground truth scored == the same ground truth given as the RLE of its rasterisation; the default still refuses."""
    from u2seg_amd.evaluation import cocoeval as CE
    from u2seg_amd.evaluation import mask_ops

    poly_ds, rle_ds, results = PC.polygon_dataset()
    assert sum(isinstance(a["segmentation"], list) for a in poly_ds["annotations"]) == 4
    img = poly_ds["images"][0]
    h, w = img["height"], img["width"]
    pa = [a for a in poly_ds["annotations"] if a["image_id"] == img["id"]]
    ra = [a for a in rle_ds["annotations"] if a["image_id"] == img["id"]]
    masks = np.stack([rle.decode(r["segmentation"]) for r in results if r["image_id"] == img["id"]])
    got = mask_ops.mask_pair_counts(masks, pa, h, w, polygons=True)
    want = mask_ops.mask_pair_counts(masks, ra, h, w)
    for g, x in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, x)
    k = [i for i, a in enumerate(pa) if isinstance(a["segmentation"], list)][0]
    assert got[2][k] == polygon.polygons_to_bitmask(pa[k]["segmentation"], h, w).sum() > 0 and got[0][:, k].any()
    with pytest.raises(NotImplementedError, match="polygon"):
        mask_ops.mask_pair_counts(masks, pa, h, w)
    with pytest.raises(ValueError, match="polygon of 3 numbers"):
        mask_ops.mask_pair_counts(masks, [{"id": 5, "segmentation": [[1, 2, 3]]}], h, w, polygons=True)
    a = CE.evaluate_segm(poly_ds, results, polygons=True)
    b = CE.evaluate_segm(rle_ds, results)
    assert a["stats"] == b["stats"] and a["stats"]["AP"] > 0
    assert np.array_equal(a["precision"], b["precision"]) and np.array_equal(a["recall"], b["recall"])
    with pytest.raises(NotImplementedError, match="polygon"):
        CE.evaluate_segm(poly_ds, results)


def tiny_polygon_dataset(tmp_path, monkeypatch, names=("tiny_poly", "tiny_poly_as_rle")):
    """polygon_cases.polygon_dataset() on disk under two names, a mapping file and the results as CPU Instances."""
    poly_ds, rle_ds, results = PC.polygon_dataset()
    os.makedirs(tmp_path / "images", exist_ok=True)
    for im in poly_ds["images"]:
        Image.fromarray(np.zeros((im["height"], im["width"], 3), dtype=np.uint8)).save(tmp_path / "images" / im["file_name"])
    for name, ds in zip(names, (poly_ds, rle_ds)):
        for cat in (DatasetCatalog, MetadataCatalog):
            if name in cat:
                cat.remove(name)
        json_file = str(tmp_path / (name + ".json"))
        json.dump(ds, open(json_file, "w"))
        register_coco_instances(name, {}, json_file, str(tmp_path / "images"))
        DatasetCatalog.get(name)
    monkeypatch.chdir(tmp_path)
    contiguous = MetadataCatalog.get(names[0]).thing_dataset_id_to_contiguous_id
    hungarian.save_mapping({c + 100: (-1 if c == 9 else contiguous[c]) for c in contiguous}, "./hungarian_matching/instance_mapping.json")
    inputs, outputs = [], []
    for im in poly_ds["images"]:
        rs = [r for r in results if r["image_id"] == im["id"]]
        inst = Instances((im["height"], im["width"]))
        b = torch.tensor([r["bbox"] for r in rs], dtype=torch.float32).reshape(-1, 4)
        inst.pred_boxes = Boxes(torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], dim=1))
        inst.scores = torch.tensor([r["score"] for r in rs], dtype=torch.float32)
        inst.pred_classes = torch.tensor([r["category_id"] + 100 for r in rs], dtype=torch.int64)
        masks = [rle.decode(r["segmentation"]) for r in rs]
        inst.pred_masks = torch.from_numpy(np.stack(masks).astype(bool)) if masks else torch.zeros((0, im["height"], im["width"]), dtype=torch.bool)
        inputs.append({"image_id": im["id"], "height": im["height"], "width": im["width"]})
        outputs.append({"instances": inst})
    return inputs, outputs


def same_with_nans(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


def test_coco_evaluator_rasterizes_when_asked(tmp_path, monkeypatch):
    inputs, outputs = tiny_polygon_dataset(tmp_path, monkeypatch)
    with pytest.raises(NotImplementedError, match="polygon"):
        COCOEvaluator("tiny_poly", mode="eval", tasks=("bbox", "segm"))
    with pytest.raises(ValueError, match="gt_polygons"):
        COCOEvaluator("tiny_poly", mode="eval", tasks=("bbox", "segm"), gt_polygons="maybe")
    ev = COCOEvaluator("tiny_poly", output_dir="out_poly", mode="eval", tasks=("bbox", "segm"), gt_polygons="rasterize")
    ev.process(inputs, outputs)
    res = ev.evaluate()
    ref = COCOEvaluator("tiny_poly_as_rle", output_dir="out_rle", mode="eval", tasks=("bbox", "segm"))
    ref.process(inputs, outputs)
    want = ref.evaluate()
    assert set(res) == {"bbox", "segm"} and res["segm"]["AP"] > 0
    same_with_nans(res["bbox"], want["bbox"])
    same_with_nans(res["segm"], want["segm"])
    for a, b in zip(ev._predictions, ref._predictions):
        for key in ("inter", "area_dt", "area_gt"):
            assert np.array_equal(a["segm_pairs"][key], b["segm_pairs"][key]), key
    # the RLE-only dataset gives the same with either setting
    same = COCOEvaluator("tiny_poly_as_rle", output_dir="out_same", mode="eval", tasks=("bbox", "segm"), gt_polygons="rasterize")
    same.process(inputs, outputs)
    same_with_nans(same.evaluate()["segm"], want["segm"])


def test_library_declares_the_polygon_entry():
    import ctypes

    from u2seg_amd import _hip

    decl = _hip.declared_symbols()
    assert decl["u2_mask_planes_from_polygons"] == (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 3
                                                    + [ctypes.c_longlong, ctypes.c_void_p])
    assert decl["u2_mask_polygon_scratch_words"] == (ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_int])
    assert os.path.exists(_hip.lib_path()), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_hip.lib_path())
    assert hasattr(lib, "u2_mask_planes_from_polygons") and hasattr(lib, "u2_mask_polygon_scratch_words")
    from u2seg_amd.evaluation.mask_ops import _PolyMask

    assert ctypes.sizeof(_PolyMask) == 24
    pm = (_PolyMask * 3)()
    for k, (h, w, n) in enumerate(((65, 3, 3), (0, 9, 4), (5, 6, 1))):
        pm[k].H, pm[k].W, pm[k].num_polys = h, w, n
    assert _hip.call_nostream("u2_mask_polygon_scratch_words", pm, 3) == 2 * 3 * 2


def test_gt_polygons_flag_through_train_net(tmp_path, monkeypatch):
    """tools/train_net.py --eval-gt-polygons rasterize: the flag parses (default refuse) and reaches the instance evaluator,
    which then scores a dataset with polygon ground truth that the default refuses (device cpu, a stub model)."""
    import importlib.util

    from u2seg_amd.config import get_cfg
    from u2seg_amd.engine import default_argument_parser

    assert default_argument_parser().parse_args([]).eval_gt_polygons == "refuse"
    args = default_argument_parser().parse_args(["--eval-only", "--eval-mode", "eval", "--eval-tasks", "bbox,segm",
                                                 "--eval-gt-polygons", "rasterize"])
    assert args.eval_gt_polygons == "rasterize"
    fx = json.load(open(os.path.join(PC.GOLD, "eval_golden.json")))
    arrays = np.load(os.path.join(PC.GOLD, "eval_golden.npz"))
    root = tmp_path / "data"
    img_dir = root / "coco" / "val2017"
    sem_dir = root / "datasets" / "panoptic_anns" / "panoptic_stuff_val2017"
    for d in (img_dir, sem_dir, root / "coco" / "annotations"):
        os.makedirs(d)
    anns = []
    for a in fx["annotations"]:
        x, y, bw, bh = a["bbox"]
        anns.append(dict(a, segmentation=[[x, y, x + bw, y, x + bw, y + bh, x, y + bh]]))
    for im in fx["images"]:
        stem = im["file_name"][:-4]
        Image.fromarray(np.zeros((im["height"], im["width"], 3), dtype=np.uint8)).save(img_dir / im["file_name"])
        Image.fromarray(arrays["gt_" + stem], mode="L").save(sem_dir / (stem + ".png"))
    cats = [{"id": c, "name": str(c), "supercategory": str(c)} for c in range(1, 801)]
    json.dump({"images": fx["images"], "annotations": anns, "categories": cats},
              open(root / "coco" / "annotations" / "instances_val2017.json", "w"))
    monkeypatch.setenv("DETECTRON2_DATASETS", str(root))
    monkeypatch.setenv("CLUSTER_NUM", "800")
    monkeypatch.chdir(tmp_path)
    for cat in (DatasetCatalog, MetadataCatalog):
        for name in list(cat.keys()):
            cat.remove(name)
    repo = os.path.dirname(os.path.dirname(PC.GOLD))
    spec = importlib.util.spec_from_file_location("u2seg_train_net_polygons", os.path.join(repo, "tools", "train_net.py"))
    train_net = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_net)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(repo, "configs", "COCO-PanopticSegmentation", "u2seg_eval_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", 0, "OUTPUT_DIR", str(tmp_path / "out")])
    by_id = {im["id"]: k for k, im in enumerate(fx["images"])}

    class Replay(torch.nn.Module):
        def forward(self, batch):
            outs = []
            for x in batch:
                k = by_id[x["image_id"]]
                im, p, pan = fx["images"][k], fx["predictions"][k], fx["panoptic_inputs"][k]
                inst = Instances((im["height"], im["width"]))
                boxes = torch.tensor(p["boxes"], dtype=torch.float32).reshape(-1, 4)
                inst.pred_boxes = Boxes(boxes)
                inst.scores = torch.tensor(p["scores"], dtype=torch.float32)
                inst.pred_classes = torch.tensor(p["classes"], dtype=torch.int64)
                masks = torch.zeros((len(boxes), im["height"], im["width"]), dtype=torch.bool)
                for m, b in zip(masks, boxes.tolist()):
                    m[max(int(b[1]), 0) : int(np.ceil(b[3])), max(int(b[0]), 0) : int(np.ceil(b[2]))] = True
                inst.pred_masks = masks
                outs.append({"instances": inst, "sem_seg": torch.from_numpy(arrays["logits_" + im["file_name"][:-4]]),
                             "panoptic_seg": (torch.tensor(pan["ids"], dtype=torch.int32), [dict(s) for s in pan["segments_info"]])})
            return outs

    name = cfg.DATASETS.TEST[0]
    tasks = tuple(args.eval_tasks.split(","))
    train_net.evaluate_on_disk_datasets(cfg, Replay(), "hungarian_matching", "cpu", tasks, gt_polygons=args.eval_gt_polygons)
    with pytest.raises(NotImplementedError, match="polygon"):
        train_net.evaluate_on_disk_datasets(cfg, Replay(), "eval", "cpu", tasks)
    both = train_net.evaluate_on_disk_datasets(cfg, Replay(), "eval", "cpu", tasks, gt_polygons=args.eval_gt_polygons)[name]
    assert set(both) == {"sem_seg", "bbox", "segm", "panoptic_seg"}
    assert all(k in both["segm"] for k in ("AP", "AP50", "AP75", "APs", "APm", "APl")) and 0 <= both["segm"]["AP50"] <= 100
    ev = build_evaluator(cfg, name, eval_mode="eval", tasks=tasks, gt_polygons="rasterize")
    assert any(getattr(e, "_gt_polygons", None) == "rasterize" for e in ev._evaluators)
    ev = build_evaluator(cfg, name, eval_mode="eval")
    assert all(getattr(e, "_gt_polygons", "refuse") == "refuse" for e in ev._evaluators)
