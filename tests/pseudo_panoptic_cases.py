"""Seeded cases of the pseudo-panoptic merge, shared by tests/test_pseudo_panoptic_host.py and
tests/test_gpu_pseudo_panoptic.py.  The expectation on every case is u2seg_amd.data.pseudo_panoptic.merge_image itself (pinned
against the reference's script in tests/test_data_path.py); `emulate` is the device's algorithm in numpy - ranks, integer
counts, the integer coverage rule - so that its equivalence is checked without a GPU.

The shapes are the smallest at which the kernels can go wrong: a single pixel, a single row, heights that are no multiple of
the 64-row band (plane padding bits), more columns than one work-group's strip only in the one full-size image."""
import copy

import numpy as np

from u2seg_amd.data import pseudo_panoptic as PP
from u2seg_amd.data import rle

CLASS_NUM = 800


def uncompressed(mask):
    """Column-major run lengths of a 0/1 mask, starting with the zeros, as a list."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    if flat.size == 0:
        return []
    change = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return ([0] if flat[0] else []) + counts


def instance(mask, cat=1, bbox=None, compressed=False):
    """A pseudo instance record of `mask`; bbox defaults to the tight box, counts are a list or the compressed string."""
    mask = np.asarray(mask, dtype=np.uint8)
    h, w = mask.shape
    seg = rle.encode(mask) if compressed else {"size": [h, w], "counts": uncompressed(mask)}
    if bbox is None:
        bbox = rle.to_bbox(rle.encode(mask))
    return {"bbox": [float(v) for v in bbox], "segmentation": seg, "category_id": int(cat), "iscrowd": 0,
            "area": int(mask.sum())}


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), dtype=np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def ellipse(h, w, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).astype(np.uint8)


def blocky(rng, h, w, block, labels=27):
    """A semantic map of constant blocks with labels 0..labels-1."""
    grid = rng.integers(0, labels, size=((h + block - 1) // block, (w + block - 1) // block))
    return np.repeat(np.repeat(grid, block, axis=0), block, axis=1)[:h, :w].astype(np.int64)


def make_cases(seed=0):
    """name -> (semantic, instances), in a fixed order."""
    rng = np.random.default_rng(seed)
    cases = {}
    # a single pixel: one instance on it; and no instance at all (a record with an empty list)
    cases["1x1_one"] = (np.array([[3]], dtype=np.int64), [instance(np.ones((1, 1)), cat=7)])
    cases["1x1_none"] = (np.array([[26]], dtype=np.int64), [])
    # a single row of 70 columns: one word per column with one valid bit
    h, w = 1, 70
    cases["1x70"] = (blocky(rng, h, w, 9), [instance(rect(h, w, 0, 1, 5, 40), 2), instance(rect(h, w, 0, 1, 30, 66), 3, compressed=True),
                                           instance(rect(h, w, 0, 1, 69, 70), 4)])
    # 65 x 3: two bands, the second of one row; n = 1
    h, w = 65, 3
    cases["65x3_one"] = (blocky(rng, h, w, 2), [instance(rect(h, w, 60, 65, 1, 3), 5)])
    # 65 x 3 with 70 instances (more than one 64-bit word of ranks): random small rectangles, many of them buried
    inst = []
    for k in range(70):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        inst.append(instance(rect(h, w, y0, min(h, y0 + int(rng.integers(1, 12))), x0, min(w, x0 + int(rng.integers(1, 3)))),
                             1 + k, compressed=bool(k % 2)))
    cases["65x3_seventy"] = (blocky(rng, h, w, 3), inst)
    # 130 x 67: three bands, the last of two rows.  An all-zero instance, an instance buried by later (smaller-box) ones whose
    # id is still consumed, two instances of equal box area that overlap (the stable order decides who is on top)
    h, w = 130, 67
    buried = instance(rect(h, w, 60, 70, 10, 20), 11, bbox=[0, 0, 67, 130])
    cover_a = instance(rect(h, w, 55, 66, 5, 25), 12)
    cover_b = instance(rect(h, w, 64, 75, 8, 22), 13, compressed=True)
    nothing = instance(np.zeros((h, w)), 14, bbox=[3, 3, 5, 5])
    twin_a = instance(rect(h, w, 100, 130, 30, 50), 15)
    twin_b = instance(rect(h, w, 110, 130, 35, 65), 16)
    assert twin_a["bbox"][2] * twin_a["bbox"][3] == twin_b["bbox"][2] * twin_b["bbox"][3]
    cases["130x67_orders"] = (blocky(rng, h, w, 16), [twin_a, cover_b, nothing, buried, twin_b, cover_a,
                                                      instance(ellipse(h, w, 30, 40, 25, 20), 17)])
    # coverage rule on 130 x 67: label 2 covered exactly 70 of 100 (claimed), label 3 covered 71 of 100 (skipped), label 4
    # completely covered, labels 5.. absent, label 0 untouched; plus labels outside 0..26, which belong to no class
    sem = np.zeros((h, w), dtype=np.int64)
    cover = np.zeros((h, w), dtype=np.uint8)
    sem[0:10, 0:10] = 2
    cover[0:7, 0:10] = 1
    sem[64:74, 20:30] = 3
    cover[64:71, 20:30] = 1
    cover[71, 20] = 1
    sem[120:130, 57:67] = 4
    cover[120:130, 57:67] = 1
    sem[20:30, 0:5] = 27
    sem[20:30, 5:10] = 255
    sem[20:30, 10:15] = -1
    sem[20:30, 15:20] = 300
    cover[25:30, 0:20] = 1
    cases["130x67_coverage"] = (sem, [instance(cover, 21)])
    # the same labels as bytes (uint8 maps go to the device as they are): 27, 200 and 255 are no class
    sem8 = np.where((sem >= 0) & (sem < 256), sem, 200).astype(np.uint8)
    cases["130x67_coverage_u8"] = (sem8, [instance(cover, 21, compressed=True)])
    # one image of the training size: 427 x 640, 12 ellipses over a blocky 27-class map
    h, w = 427, 640
    inst = [instance(ellipse(h, w, rng.integers(40, h - 40), rng.integers(40, w - 40), rng.integers(15, 120), rng.integers(15, 160)),
                     1 + k, compressed=True) for k in range(12)]
    cases["427x640_twelve"] = (blocky(rng, h, w, 48), inst)
    return cases


RAGGED = ("130x67_orders", "1x1_none", "65x3_seventy", "130x67_coverage", "1x70")  # the batch of five images
WRAP_FIRST_ID = 16777210                                                        # ids cross 2^24 inside the batch


def expected(semantic, instances, first_id, class_num=CLASS_NUM):
    """merge_image on a copy of the records: (id map, segments_info, next id, the "id" every record received)."""
    inst = copy.deepcopy(instances)
    ids, segments, nxt = PP.merge_image(semantic, inst, class_num, first_id)
    return ids, segments, nxt, [r["id"] for r in inst]


def label_map(ids, segments, class_num=CLASS_NUM):
    """What separate_semantic_from_panoptic writes for an id map (taken as it is, not through a png) with
    create_cate(class_num): things 0, stuff category class_num + c -> c, everything else 255."""
    out = np.full(ids.shape, 255, dtype=np.uint8)
    for seg in segments:
        out[ids == seg["id"]] = 0 if seg["category_id"] <= class_num else seg["category_id"] - class_num
    return out


def emulate(items, first_id, class_num=CLASS_NUM):
    """The device's algorithm in numpy on the packed batch: per image (id map, segments_info, ids given to the records), and
    the next free id.  Integer arithmetic only."""
    packed = PP.pack_items(items)
    out, nxt, m = [], int(first_id), 0
    counts, offs = packed["counts"], packed["offsets"]
    for (semantic, instances), (h, w), order, sem in zip(items, packed["sizes"], packed["orders"], packed["sems"]):
        rank = np.zeros((h, w), dtype=np.int32)
        for r in range(len(order)):
            if h * w:
                c = counts[offs[m]:offs[m + 1]]
                m += 1
                values = np.zeros(len(c), dtype=np.uint8)
                values[1::2] = 1
                rank[np.repeat(values, c).reshape(w, h).T == 1] = r + 1
        base = nxt
        given = [0] * len(order)
        for r, k in enumerate(order):
            given[k] = base + r
        segments = [dict(instances[k], id=base + r) for r, k in enumerate(order) if (rank == r + 1).any()]
        nxt = base + len(order)
        ids = np.where(rank > 0, np.uint32(base) + rank.astype(np.uint32) - np.uint32(1), np.uint32(0)).astype(np.uint32)
        for c in range(1, PP.NUM_STUFF + 1):
            total = int((sem == c - 1).sum())
            covered = int(((sem == c - 1) & (rank > 0)).sum())
            if total - covered > 0 and not PP.coverage_skips(covered, total):
                ids[(sem == c - 1) & (rank == 0)] = nxt
                segments.append({"category_id": c + class_num, "id": nxt, "iscrowd": 0, "bbox": [], "area": 0})
                nxt += 1
        out.append((ids, segments, given))
    return out, nxt
