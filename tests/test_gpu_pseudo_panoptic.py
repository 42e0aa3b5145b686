"""The pseudo-panoptic merge on the GPU (u2seg_amd/csrc/labelprep.hip through merge_images_device and generate) against
merge_image, the host definition, on the cases of tests/pseudo_panoptic_cases.py, and against the reference script's golden
tree.  Integers throughout: every comparison is array_equal or ==.  Every launched case keeps the contract of the launchers;
the violations are refused on the host (tests/test_pseudo_panoptic_host.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import pseudo_panoptic_cases as cases
from u2seg_amd.data import pseudo_panoptic as PP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = cases.make_cases()
ALL = ("rgb", "sem", "ids")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def items_of(names):
    return [(CASES[n][0], copy.deepcopy(CASES[n][1])) for n in names]


def check_image(res, records, want, where):
    ids, segments, _, given = want
    assert res["segments_info"] == segments, where
    assert [r["id"] for r in records] == given, where  # every record receives its id, the dropped ones too
    assert res["ids"].dtype == np.uint32 and np.array_equal(res["ids"], ids), where
    assert res["rgb"].dtype == np.uint8 and np.array_equal(res["rgb"], PP.id2rgb(ids)), where
    assert res["sem"].dtype == np.uint8 and np.array_equal(res["sem"], cases.label_map(ids, segments)), where


@pytest.mark.parametrize("name", list(CASES))
def test_single_image_equals_merge_image(hip, name):
    """1 x 1, 1 x 70, 65 x 3, 130 x 67 and 427 x 640; n = 0, 1, 3, 7, 12 and 70; an all-zero instance, a buried one, equal box
    areas, classes absent / fully covered / covered exactly 7/10 / one pixel more, labels outside 0..26."""
    want = cases.expected(*CASES[name], 5)
    items = items_of([name])
    (res,), nxt = PP.merge_images_device(items, cases.CLASS_NUM, 5, DEV, outputs=ALL)
    assert nxt == want[2]
    check_image(res, items[0][1], want, name)


def test_ragged_batch_runs_the_ids_on_across_2_to_the_24(hip):
    """Five images of different sizes in one batch == five merge_image calls in sequence, first id 16 777 210: the ids
    cross 2^24, where the id image wraps like id2rgb and the uint32 id map does not; batch 1 gives the same as batch 5."""
    items = items_of(cases.RAGGED)
    results, nxt = PP.merge_images_device(items, cases.CLASS_NUM, cases.WRAP_FIRST_ID, DEV, outputs=ALL)
    seg_id, crossed = cases.WRAP_FIRST_ID, False
    for n, (_, records), res in zip(cases.RAGGED, items, results):
        want = cases.expected(*CASES[n], seg_id)
        check_image(res, records, want, n)
        crossed = crossed or (int(want[0].max()) >= 2 ** 24 and not np.array_equal(PP.rgb2id(res["rgb"]), want[0]))
        seg_id = want[2]
    assert nxt == seg_id and crossed
    seg_id = cases.WRAP_FIRST_ID
    for n, res in zip(cases.RAGGED, results):
        one = items_of([n])
        (single,), seg_id = PP.merge_images_device(one, cases.CLASS_NUM, seg_id, DEV, outputs=ALL)
        assert single["segments_info"] == res["segments_info"], n
        for k in ALL:
            assert np.array_equal(single[k], res[k]), (n, k)
    assert seg_id == nxt


def test_more_images_than_one_launch_describes(hip):
    """The launchers describe 64 images per launch: 66 small images in one batch, the ids running on over the seam."""
    names = [("1x70", "1x1_one", "65x3_one", "1x1_none")[i % 4] for i in range(66)]
    items = items_of(names)
    results, nxt = PP.merge_images_device(items, cases.CLASS_NUM, 3, DEV, outputs=ALL)
    seg_id = 3
    for i, (n, (_, records), res) in enumerate(zip(names, items, results)):
        want = cases.expected(*CASES[n], seg_id)
        check_image(res, records, want, (i, n))
        seg_id = want[2]
    assert nxt == seg_id


def test_outputs_are_optional_and_an_empty_batch_is_empty(hip):
    items = items_of(["130x67_orders"])
    (res,), nxt = PP.merge_images_device(items, cases.CLASS_NUM, 9, DEV)
    want = cases.expected(*CASES["130x67_orders"], 9)
    assert sorted(res) == ["rgb", "segments_info", "sem"] and nxt == want[2]
    assert np.array_equal(res["rgb"], PP.id2rgb(want[0])) and np.array_equal(res["sem"], cases.label_map(want[0], want[1]))
    (res,), _ = PP.merge_images_device(items_of(["130x67_orders"]), cases.CLASS_NUM, 9, DEV, outputs=("ids",))
    assert sorted(res) == ["ids", "segments_info"] and np.array_equal(res["ids"], want[0])
    assert PP.merge_images_device([], cases.CLASS_NUM, 9, DEV) == ([], 9)


def test_generate_on_the_device_matches_the_reference_scripts(hip, tmp_path):
    """generate(device=..., sem_seg_root=...) on the tree of the reference-script fixture: the json, every png and every
    label map equal what generate_pseudo_panoptic.py and prepare_stuff_panoptic_fpn.py produced (pseudo_panoptic_golden,
    label_prep_golden).  Batch 1 makes the second image's ids depend on the first batch's readback."""
    from PIL import Image

    fx = json.load(open(os.path.join(GOLD, "pseudo_panoptic_golden.json")))
    arrays = np.load(os.path.join(GOLD, "pseudo_panoptic_golden.npz"))
    sem_gold = np.load(os.path.join(GOLD, "label_prep_golden.npz"))
    for batch in (16, 1):
        root = tmp_path / ("b%d" % batch)
        ann_root = root / "datasets" / "prepare_ours" / "u2seg_annotations"
        sem_dir = ann_root / "semantic_annotations" / "stego_coco_train_semantic_seg_resized"
        for d in (ann_root / "ins_annotations", sem_dir, ann_root / "panoptic_annotations",
                  root / "datasets" / "datasets" / "panoptic_anns"):
            os.makedirs(d)
        json.dump(fx["template"], open(root / "datasets" / "datasets" / "panoptic_anns" / "panoptic_train2017.json", "w"))
        json.dump(fx["pseudo"], open(ann_root / "ins_annotations" / "cocotrain_800_ins_panoptic.json", "w"))
        with open(ann_root / "semantic_annotations" / "coco_train_img_file_names.txt", "w") as f:
            for i, name in enumerate(fx["names"]):
                f.write(name + "\n")
                np.save(sem_dir / ("%d.npy" % i), arrays["semantic_%d" % i])
        out = PP.generate(str(root), 800, "train", device=DEV, batch_images=batch, sem_seg_root=str(root / "sem"))
        assert out == fx["expected"]
        assert json.load(open(ann_root / "panoptic_annotations" / "cocotrain_800.json")) == fx["expected"]
        for a in out["annotations"]:
            png = np.asarray(Image.open(ann_root / "panoptic_annotations" / "cocotrain_800" / a["file_name"]))
            assert np.array_equal(PP.rgb2id(png), arrays["ids_" + a["file_name"]])
            got = np.asarray(Image.open(root / "sem" / a["file_name"]))
            assert got.dtype == np.uint8 and np.array_equal(got, sem_gold["sem_" + a["file_name"]])
