"""Shared by tests/test_polygon_host.py and tests/test_gpu_polygon.py: the known answers, a literal restatement of cocoapi's
rleFrPoly (sort / difference / merge form, scalar Python), seeded random polygons and a tiny dataset with polygon ground truth."""
import copy
import json
import math
import os
import random

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def known_answers():
    return json.load(open(os.path.join(GOLD, "polygon_known_answers.json")))["cases"]


def literal_counts(xy, h, w):
    """rleFrPoly of common/maskApi.c line by line: the uncompressed counts of one polygon."""
    k = len(xy) // 2
    scale = 5.0
    x = [int(scale * xy[2 * j] + .5) for j in range(k)]
    y = [int(scale * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else 0.0  # 0 / 0 in C; the one point of such an edge is the vertex
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + .5))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / scale - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / scale - .5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            a.append(int(xd) * h + int(yd))
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return b


def literal_mask(xy, h, w):
    counts = np.asarray(literal_counts(xy, h, w), dtype=np.int64)
    assert counts.sum() == h * w and (counts >= 0).all()
    values = np.zeros(len(counts), dtype=np.uint8)
    values[1::2] = 1
    return np.repeat(values, counts).reshape(w, h).T


def random_polygons(n, seed, max_side=89):
    """(xy, h, w): k = 1..11 points; integer, fifth-of-a-pixel or arbitrary coordinates, up to 4 px outside the image."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        h, w, k, kind = rng.randint(1, max_side), rng.randint(1, max_side), rng.randint(1, 11), i % 3
        xy = []
        for _ in range(k):
            for side in (w, h):
                c = rng.uniform(-4, side + 4)
                xy.append(float(round(c)) if kind == 0 else round(c * 5) / 5 if kind == 1 else c)
        out.append((xy, h, w))
    return out


def blob_polygon(rng, h, w, vertices):
    """A star-shaped blob of `vertices` points around a centre inside the image (numpy RandomState)."""
    cx, cy = rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h)
    rx, ry = rng.uniform(0.05 * w, 0.4 * w), rng.uniform(0.05 * h, 0.4 * h)
    ang = np.sort(rng.uniform(0, 2 * np.pi, vertices))
    rad = rng.uniform(0.6, 1.0, vertices)
    return np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], axis=1).reshape(-1).tolist()


def polygon_dataset():
    """The four images [1, 4, 7, 10] of segm_eval_golden with polygon ground truth mixed in: (dataset with one annotation per
    image turned into polygons - two overlapping ones for the first -, the same dataset with those annotations as the RLE of
    the polygons' rasterisation, the fixture's results for these images)."""
    from u2seg_amd.data import polygon

    fx = json.load(open(os.path.join(GOLD, "segm_eval_golden.json")))
    ids = [1, 4, 7, 10]
    images = [dict(im, file_name="%06d.jpg" % im["id"]) for im in fx["dataset"]["images"] if im["id"] in ids]
    size = {im["id"]: (im["height"], im["width"]) for im in images}
    cats = [{"id": c["id"], "name": "c%d" % c["id"]} for c in fx["dataset"]["categories"]]
    anns = [a for a in fx["dataset"]["annotations"] if a["image_id"] in ids]
    poly, as_rle = copy.deepcopy(anns), copy.deepcopy(anns)
    seen = set()
    for k, a in enumerate(anns):
        if a["image_id"] in seen or a.get("iscrowd"):
            continue
        seen.add(a["image_id"])
        x, y, bw, bh = a["bbox"]
        ring = [x + .3, y - 1.2, x + bw + .4, y + .25 * bh, x + .8 * bw, y + bh + .6, x - 1.5, y + .7 * bh]
        polys = [ring] if len(seen) > 1 else [ring, [x + .5 * bw, y, x + 1.5 * bw, y + .5 * bh, x + .5 * bw, y + bh]]
        poly[k]["segmentation"] = polys
        as_rle[k]["segmentation"] = polygon.polygons_to_rle(polys, *size[a["image_id"]])
    assert len(seen) == len(ids)
    results = [r for r in fx["results"] if r["image_id"] in ids]
    return ({"images": images, "annotations": poly, "categories": cats},
            {"images": images, "annotations": as_rle, "categories": cats}, results)
