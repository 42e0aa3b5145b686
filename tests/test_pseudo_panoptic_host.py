"""Host side of the device pseudo-panoptic merge (u2seg_amd/data/pseudo_panoptic.py: pack_items, coverage_skips, the refusals)
without a GPU.  The expectation is merge_image; tests/test_gpu_pseudo_panoptic.py runs the same cases through the kernels."""
import copy

import numpy as np
import pytest

from tests import pseudo_panoptic_cases as cases
from u2seg_amd.data import pseudo_panoptic as PP
from u2seg_amd.data import rle

CASES = cases.make_cases()


def test_cases_are_seeded_and_hit_what_they_are_for():
    again = cases.make_cases()
    assert list(again) == list(CASES)
    for name in CASES:
        assert np.array_equal(again[name][0], CASES[name][0]) and again[name][1] == CASES[name][1]
    # the buried instance vanishes, its id is consumed; the all-zero instance vanishes too
    sem, inst = CASES["130x67_orders"]
    ids, segments, nxt, given = cases.expected(sem, inst, 5)
    assert sorted(given) == list(range(5, 12)) and given[3] == 5            # the buried one has the largest box: first id
    kept = {s["id"] for s in segments if s["category_id"] <= cases.CLASS_NUM}
    assert given[3] not in kept and given[2] not in kept and len(kept) == 5
    assert given[0] < given[4] and (ids[115, 40] == given[4])               # equal box areas: the later record is on top
    # the coverage rule: label 2 (exactly 7/10 covered) claimed, label 3 (one pixel more) skipped, label 4 (all covered) and
    # the labels outside 0..26 unclaimed
    for name in ("130x67_coverage", "130x67_coverage_u8"):
        sem, inst = CASES[name]
        ids, segments, nxt, given = cases.expected(sem, inst, 1)
        stuff = [s["category_id"] - cases.CLASS_NUM for s in segments if s["category_id"] > cases.CLASS_NUM]
        assert stuff == [1, 3]
        assert (ids[20:25, 0:20] == 0).all() and (ids[72:74, 20:30] == 0).all() and (ids[7:10, 0:10] == nxt - 1).all()


@pytest.mark.parametrize("name", list(CASES))
def test_device_algorithm_in_numpy_equals_merge_image(name):
    sem, inst = CASES[name]
    for first_id in (1, cases.WRAP_FIRST_ID):
        ids, segments, nxt, given = cases.expected(sem, inst, first_id)
        (got,), got_next = cases.emulate([(sem, copy.deepcopy(inst))], first_id)
        assert got_next == nxt and got[1] == segments and got[2] == given
        assert got[0].dtype == np.uint32 and np.array_equal(got[0], ids)


def test_ragged_batch_in_numpy_equals_sequential_merge_image():
    items = [(CASES[n][0], copy.deepcopy(CASES[n][1])) for n in cases.RAGGED]
    got, got_next = cases.emulate(items, cases.WRAP_FIRST_ID)
    nxt = cases.WRAP_FIRST_ID
    for n, g in zip(cases.RAGGED, got):
        ids, segments, nxt, given = cases.expected(*CASES[n], nxt)
        assert np.array_equal(g[0], ids) and g[1] == segments and g[2] == given
    assert got_next == nxt and nxt > 2 ** 24


def test_pack_items_order_counts_offsets():
    names = ("130x67_orders", "1x1_none", "1x70")
    items = [(CASES[n][0], copy.deepcopy(CASES[n][1])) for n in names]
    packed = PP.pack_items(items)
    assert packed["sizes"] == [(130, 67), (1, 1), (1, 70)] and packed["num"] == [7, 0, 3]
    # stable, by decreasing box area: the buried instance's declared box is the image; the twins keep their order
    inst = items[0][1]
    areas = [r["bbox"][2] * r["bbox"][3] for r in inst]
    order = packed["orders"][0]
    assert order == PP.paint_order(inst) and sorted(order) == list(range(7)) and order[0] == 3
    assert all(areas[a] > areas[b] or (areas[a] == areas[b] and a < b) for a, b in zip(order, order[1:]))
    assert order.index(0) + 1 == order.index(4)
    assert packed["orders"][1] == [] and packed["orders"][2] == PP.paint_order(items[2][1])
    # the counts of all instances, flattened in paint order, compressed strings parsed
    flat = [rle.counts_of(items[i][1][k]["segmentation"]) for i in (0, 2) for k in packed["orders"][i]]
    assert packed["offsets"].dtype == np.int64 and packed["counts"].dtype == np.int32
    assert packed["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(c) for c in flat])]).tolist()
    assert packed["counts"].tolist() == [c for lst in flat for c in lst]
    for m, c in enumerate(flat):
        assert sum(c) == (130 * 67 if m < 7 else 70)
    # labels: int maps are narrowed to bytes with everything outside 0..26 as 255, byte maps pass as they are
    sem = PP.pack_items([CASES["130x67_coverage"]])["sems"][0]
    assert sem.dtype == np.uint8 and set(np.unique(sem).tolist()) == {0, 2, 3, 4, 255}
    sem8 = PP.pack_items([CASES["130x67_coverage_u8"]])["sems"][0]
    assert np.array_equal(sem8, CASES["130x67_coverage_u8"][0])
    empty = PP.pack_items([])
    assert empty["sizes"] == [] and empty["offsets"].tolist() == [0] and empty["counts"].size == 0


def test_integer_coverage_rule_is_the_float_rule():
    """10 covered > 7 total == covered / total > 0.7 in float64, for every total <= 2000 and every covered <= total."""
    for total in range(1, 2001):
        covered = np.arange(total + 1, dtype=np.int64)
        assert np.array_equal(PP.coverage_skips(covered, total), covered / total > PP.COVERED_FRACTION), total
    assert PP.coverage_skips(70, 100) is False and PP.coverage_skips(71, 100) is True
    rng = np.random.default_rng(1)
    for total in rng.integers(1, 2 ** 31, size=2000).tolist():
        for covered in (7 * total // 10 - 1, 7 * total // 10, 7 * total // 10 + 1):
            if 0 <= covered <= total:
                assert PP.coverage_skips(covered, total) == (np.float64(covered) / np.float64(total) > PP.COVERED_FRACTION)


def test_refusals_come_before_any_launch():
    one = cases.instance(np.ones((2, 3)))
    with pytest.raises(ValueError, match="2\\^31"):
        PP.pack_items([(np.broadcast_to(np.uint8(0), (65536, 32768)), [])])
    with pytest.raises(ValueError, match="instances"):
        PP.pack_items([(np.zeros((2, 3), dtype=np.uint8), [one] * 65536)])
    assert len(PP.pack_items([(np.zeros((2, 3), dtype=np.uint8), [one] * 3)])["offsets"]) == 4
    with pytest.raises(ValueError, match="size"):
        PP.pack_items([(np.zeros((3, 2), dtype=np.uint8), [one])])
    for counts in ([2, 3], [2, 5], [7, -1], [8, -2]):
        bad = dict(one, segmentation={"size": [2, 3], "counts": counts})
        with pytest.raises(ValueError, match="RLE counts"):
            PP.pack_items([(np.zeros((2, 3), dtype=np.uint8), [bad])])
        with pytest.raises(ValueError, match="RLE counts"):  # the same condition as the host decoder's
            rle.decode(bad["segmentation"])
    with pytest.raises(ValueError):
        PP.pack_items([(np.zeros((2, 3), dtype=np.float32), [])])
    # no host fallback: without a GPU device the merge raises, like --device-mapper
    with pytest.raises(RuntimeError, match="GPU"):
        PP.merge_images_device([(np.zeros((2, 3), dtype=np.uint8), [copy.deepcopy(one)])], 800, 1, "cpu")
    with pytest.raises(ValueError, match="outputs"):
        PP.merge_images_device([], 800, 1, "cuda", outputs=("png",))
    with pytest.raises(ValueError, match="sem_seg_root"):
        PP.generate("/nonexistent", 800, "train", device=None, sem_seg_root="/nonexistent/sem")
