"""Generates tests/golden/segm_eval_golden.json / .npz: the reference's C++ COCO evaluation core
(detectron2/layers/csrc/cocoeval/cocoeval.cpp: COCOevalEvaluateImages + COCOevalAccumulate, compiled into the _C extension
that make_fixtures.import_reference builds) fed with MASK areas and MASK IoUs on a synthetic instance-segmentation problem.
Runs only where the reference is checked out; the output is committed and the tests read nothing else.

    python tests/golden/make_segm_eval_fixture.py

Problem: 12 images of 200 x 300 (one of 120 x 90), 5 categories.  Ground truth: ellipses of three size classes (mask areas
around 110, 2 000 and 15 000 pixels: small, medium, large BY MASK AREA), `area` = mask area, `segmentation` = compressed
RLE, for the crowd regions (about one in seven) uncompressed RLE as COCO stores them.  Detections carry `bbox` and a
compressed RLE `segmentation`: jittered copies of the instances, some in the wrong class, strays, scores with two decimals
(ties), 130 detections in the cell (image 1, category 2) (budget truncation), one empty mask, and planted in image 4 a
3-pixel ring in a 40 x 40 box - box area 1 600 (medium), mask area 444 (small) - on a ground-truth ring of the same shape.

Expected values: the IoU table of every (image, category) cell, computed HERE densely in float64 from the arrays the masks
were drawn into - inter / (area_dt + area_gt - inter), inter / area_dt for a crowd region, 0 where that denominator is 0 -
with the detections in descending score order (stable) cut at 100, and the precision / recall / score tables the C++ makes
of them.  Nothing of u2seg_amd.evaluation computes an expected value; data/rle.py only writes the strings."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from u2seg_amd.data import rle  # noqa: E402

CATS = (1, 2, 5, 7, 9)


def ellipse(h, w, cx, cy, rx, ry):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx - cx) / max(rx, 0.5)) ** 2 + ((yy - cy) / max(ry, 0.5)) ** 2) <= 1.0).astype(np.uint8)


def ring(h, w, x0, y0, side, t):
    m = np.zeros((h, w), dtype=np.uint8)
    m[y0 : y0 + side, x0 : x0 + side] = 1
    m[y0 + t : y0 + side - t, x0 + t : x0 + side - t] = 0
    return m


def box_of(m):
    ys, xs = np.nonzero(m)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def main():
    from make_fixtures import import_reference

    import_reference()
    C = sys.modules["detectron2._C"]
    rs = np.random.RandomState(33)
    images = [{"id": 3 * i + 1, "height": 200, "width": 300} for i in range(12)]
    images[7]["height"], images[7]["width"] = 120, 90
    anns, results, gt_masks, dt_masks, aid = [], [], [], [], 1

    def add_gt(im, cat, m, crowd):
        nonlocal aid
        r = rle.encode(m)
        seg = {"size": r["size"], "counts": rle.counts_of(r)} if crowd else r
        anns.append({"id": aid, "image_id": im["id"], "category_id": cat, "bbox": box_of(m), "area": float(m.sum()),
                     "iscrowd": int(crowd), "segmentation": seg})
        gt_masks.append(m)
        aid += 1

    def add_dt(im, cat, m, score, bbox=None):
        results.append({"image_id": im["id"], "category_id": cat, "bbox": box_of(m) if bbox is None else bbox, "score": score,
                        "segmentation": rle.encode(m)})
        dt_masks.append(m)

    for im in images:
        h, w = im["height"], im["width"]
        for _ in range(rs.randint(0, 7)):
            r0 = rs.choice([6.0, 25.0, 70.0]) * rs.uniform(0.8, 1.2)
            rx, ry = min(r0, w / 2 - 2), min(r0 * rs.uniform(0.7, 1.3), h / 2 - 2)
            cx, cy = rs.uniform(rx, w - rx), rs.uniform(ry, h - ry)
            cat = int(rs.choice(CATS))
            m = ellipse(h, w, cx, cy, rx, ry)
            if m.sum() == 0:
                continue
            add_gt(im, cat, m, rs.rand() < 0.15)
            for _ in range(rs.randint(0, 4)):  # detections around the instance, some in the wrong class
                j = rs.uniform(-1, 1, 4) * r0 * rs.choice([0.03, 0.15, 0.5])
                add_dt(im, cat if rs.rand() < 0.8 else int(rs.choice(CATS)),
                       ellipse(h, w, cx + j[0], cy + j[1], max(rx + j[2], 1), max(ry + j[3], 1)),
                       float(np.round(rs.uniform(0.05, 1.0), 2)))  # two decimals: ties happen
        for _ in range(rs.randint(0, 5)):  # strays
            add_dt(im, int(rs.choice(CATS)), ellipse(h, w, rs.uniform(0, w), rs.uniform(0, h), rs.uniform(3, 25), rs.uniform(3, 25)),
                   float(np.round(rs.uniform(0.05, 0.6), 2)))
    im1, im4 = images[0], images[1]
    for k in range(130):  # one crowded cell beyond the 100-detection budget
        add_dt(im1, 2, ellipse(200, 300, 15 + 2 * k % 250, 15 + k % 150, 14, 14), float(np.round(rs.uniform(0.01, 0.99), 3)))
    add_gt(im4, 5, ring(200, 300, 100, 60, 40, 3), False)  # mask area 444: small; its box is medium
    add_dt(im4, 5, ring(200, 300, 101, 60, 40, 3), 0.9)
    add_dt(im4, 5, np.zeros((200, 300), dtype=np.uint8), 0.5, bbox=[10.0, 10.0, 20.0, 20.0])  # an empty mask
    add_dt(im4, 7, np.zeros((200, 300), dtype=np.uint8), 0.4, bbox=[10.0, 10.0, 20.0, 20.0])

    img_ids, cat_ids = sorted(im["id"] for im in images), sorted(CATS)
    area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    max_dets = [1, 10, 100]
    iou_thrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
    rec_thrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
    gts, dts = {}, {}
    for k, a in enumerate(anns):
        gts.setdefault((a["image_id"], a["category_id"]), []).append(k)
    for k, r in enumerate(results):
        dts.setdefault((r["image_id"], r["category_id"]), []).append(k)
    arrays, iou_cpp, gt_cpp, dt_cpp = {}, [], [], []
    for i in img_ids:
        iou_row, gt_row, dt_row = [], [], []
        for c in cat_ids:
            g, d = gts.get((i, c), []), dts.get((i, c), [])
            gt_row.append([C.InstanceAnnotation(int(anns[k]["id"]), 0.0, float(anns[k]["area"]), bool(anns[k]["iscrowd"]),
                                                bool(anns[k]["iscrowd"])) for k in g])
            dt_row.append([C.InstanceAnnotation(k + 1, float(results[k]["score"]), float(dt_masks[k].sum()), False, False)
                           for k in d])
            if not g and not d:
                iou_row.append([])
                continue
            order = np.argsort([-results[k]["score"] for k in d], kind="mergesort")[: max_dets[-1]]
            table = np.zeros((len(order), len(g)), dtype=np.float64)
            for a_, di in enumerate(order):
                dm = dt_masks[d[di]].astype(bool)
                for b_, gk in enumerate(g):
                    gm = gt_masks[gk].astype(bool)
                    inter = int((dm & gm).sum())
                    union = int(dm.sum()) if anns[gk]["iscrowd"] else int(dm.sum()) + int(gm.sum()) - inter
                    table[a_, b_] = inter / union if union > 0 else 0.0
            arrays["iou_%d_%d" % (i, c)] = table
            iou_row.append(table.tolist() if table.size else [])
        iou_cpp.append(iou_row)
        gt_cpp.append(gt_row)
        dt_cpp.append(dt_row)
    evals = C.COCOevalEvaluateImages(area_rng, max_dets[-1], iou_thrs.tolist(), iou_cpp, gt_cpp, dt_cpp)

    class P:
        pass

    pobj = P()
    pobj.recThrs, pobj.maxDets, pobj.iouThrs = rec_thrs.tolist(), max_dets, iou_thrs.tolist()
    pobj.catIds, pobj.areaRng, pobj.imgIds, pobj.useCats = cat_ids, area_rng, img_ids, 1
    acc = C.COCOevalAccumulate(pobj, evals)
    counts = list(acc["counts"])
    arrays["precision"] = np.array(acc["precision"]).reshape(counts)
    arrays["scores"] = np.array(acc["scores"]).reshape(counts)
    arrays["recall"] = np.array(acc["recall"]).reshape(counts[:1] + counts[2:])
    dataset = {"images": images, "annotations": anns, "categories": [{"id": c} for c in CATS]}
    planted = [k for k, r in enumerate(results) if r["bbox"][2] * r["bbox"][3] > 32 ** 2 and 0 < dt_masks[k].sum() < 32 ** 2]
    json.dump({"dataset": dataset, "results": results, "box_medium_mask_small": planted},
              open(os.path.join(HERE, "segm_eval_golden.json"), "w"))
    np.savez_compressed(os.path.join(HERE, "segm_eval_golden.npz"), **arrays)
    areas = np.array([a["area"] for a in anns])
    print("wrote segm_eval_golden: %d gt (%d crowd; %d small, %d medium, %d large), %d detections, %d with a medium box and a "
          "small mask; mean precision over valid entries %.4f; json %d bytes, npz %d bytes"
          % (len(anns), sum(a["iscrowd"] for a in anns), (areas < 1024).sum(), ((areas >= 1024) & (areas <= 9216)).sum(),
             (areas > 9216).sum(), len(results), len(planted), float(arrays["precision"][arrays["precision"] > -1].mean()),
             os.path.getsize(os.path.join(HERE, "segm_eval_golden.json")), os.path.getsize(os.path.join(HERE, "segm_eval_golden.npz"))))


if __name__ == "__main__":
    main()
