"""Inputs shared by test_cocoeval_pack_host.py and test_gpu_cocoeval.py: seeded COCO problems (dataset dict + results) and the
groups `cocoeval.prepare` makes of them, restated the way `cocoeval.compute_ious` / `accumulate` order them."""
import numpy as np

from u2seg_amd.evaluation import cocoeval as CE


def random_problem(seed=0, images=30, cats=5, max_dets_per_image=120, crowd=0.08, score_decimals=2, shuffle=True):
    """Integer-grid boxes (IoU ties), half of the detections on or next to a ground truth, rounded scores (score ties inside a
    cell and across images), crowd regions, image ids that are neither sorted nor contiguous, results in shuffled order."""
    rs = np.random.RandomState(seed)
    img_ids = [int(v) for v in rs.permutation(np.arange(3, 3 + 7 * images, 7))]
    cat_ids = [2 + 3 * k for k in range(cats)]
    anns, results = [], []
    for img in img_ids:
        first = len(anns)
        for _ in range(rs.randint(0, 9)):
            w, h = int(rs.choice([8, 16, 32, 40, 96, 120])), int(rs.choice([8, 16, 32, 40, 96, 120]))
            x, y = int(rs.randint(0, 12)) * 8, int(rs.randint(0, 12)) * 8
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": int(rs.choice(cat_ids)), "bbox": [x, y, w, h],
                         "area": w * h, "iscrowd": int(rs.rand() < crowd)})
        own = rs.choice(cat_ids, size=2, replace=False)
        for _ in range(rs.randint(0, max_dets_per_image + 1)):
            w, h = int(rs.choice([8, 16, 32, 40, 96, 120])), int(rs.choice([8, 16, 32, 40, 96, 120]))
            x, y = int(rs.randint(0, 12)) * 8, int(rs.randint(0, 12)) * 8
            cat = int(own[int(rs.rand() < 0.3)])
            if len(anns) > first and rs.rand() < 0.5:  # near a ground truth of the image: the same box, or one grid step off
                a = anns[int(rs.randint(first, len(anns)))]
                (x, y, w, h), cat = a["bbox"], a["category_id"]
                x, w = x + 8 * int(rs.randint(0, 2)), w + 8 * int(rs.randint(0, 2))
            results.append({"image_id": img, "category_id": cat, "bbox": [x, y, w, h],
                            "score": float(np.round(rs.rand(), score_decimals))})
    if shuffle:
        results = [results[i] for i in rs.permutation(len(results))]
    dataset = {"images": [{"id": i} for i in img_ids], "categories": [{"id": c} for c in cat_ids], "annotations": anns}
    return dataset, results


def groups(dataset, results, max_dets=(1, 10, 100)):
    imgs = sorted(im["id"] for im in dataset["images"])
    cats = sorted(c["id"] for c in dataset["categories"])
    params = CE.Params(imgs, cats, max_dets)
    gts, dts = CE.prepare(dataset["annotations"], results, params)
    return params, gts, dts


def expected_cells(params, gts, dts):
    """{(image, category): (detection ids in score order, cut; ground-truth ids)} over the non-empty pairs."""
    out = {}
    for img in params.imgIds:
        for cat in params.catIds:
            gt, dt = gts.get((img, cat), []), dts.get((img, cat), [])
            if not gt and not dt:
                continue
            order = np.argsort([-d["score"] for d in dt], kind="mergesort")[: params.maxDets[-1]]
            out[img, cat] = ([dt[i]["id"] for i in order], [g["id"] for g in gt])
    return out


def expected_lists(params, cells, dts):
    """{category: detection ids of all images in accumulate's order} (stable descending score over the images in
    params.imgIds order)."""
    score = {d["id"]: d["score"] for v in dts.values() for d in v}
    out = {}
    for cat in params.catIds:
        ids = [i for img in params.imgIds for i in cells.get((img, cat), ([], []))[0]]
        order = np.argsort([-score[i] for i in ids], kind="mergesort")
        out[cat] = [ids[i] for i in order]
    return out
