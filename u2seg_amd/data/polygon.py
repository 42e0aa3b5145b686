"""COCO polygon segmentations -> masks without pycocotools (the reference calls pycocotools' frPyObjects / merge / decode:
detectron2/structures/masks.py:polygons_to_bitmask).  This module is the definition; csrc/polygon.hip computes the same on
the device.

The algorithm is cocoapi's rleFrPoly (common/maskApi.c), restated; every arithmetic step is one float64 operation and
(int) truncates toward zero:
1. the k vertices go to a 5x finer integer grid, X = (int)(5 x + .5), and the ring is closed;
2. every edge is walked in max(|dx|, |dy|) + 1 integer points from its start to its end vertex: the longer axis advances by
   one per point, the other is (int)(c0 + s t + .5) with t counted from the end whose stepping coordinate is smaller, c0 that
   end's other coordinate and s = (double)(difference of the other coordinate) / (length along the stepping axis);
3. every consecutive pair of points (u0, v0) -> (u1, v1) with u1 != u0 is a crossing of a vertical grid line: with
   u' = u1 if u1 < u0 else u1 - 1, xd = (u' + .5) / 5 - .5 must be an integer in [0, w - 1], yd = ceil of (min(v0, v1) + .5) / 5 - .5
   clamped to [0, h]; the crossing toggles the column-major scan at position a = xd h + yd;
4. pixel i = x h + y is set iff an odd number of crossings have a <= i (cocoapi sorts the positions, takes differences as run
   lengths and merges the zero-length runs: two crossings at one position cancel);
5. the mask of an annotation is the union of its polygons' masks (mask_util.merge); one self-intersecting polygon is even-odd.

In integers (tests/test_polygon_host.py proves both): the pair counts iff u' mod 5 == 2 (floor-mod), then xd = (u' - 2) / 5;
yd = clamp(floor_div(v' + 2, 5), 0, h).

cocoapi itself is not available to this project: the definition is pinned by the known answers of
tests/golden/polygon_known_answers.json, not against the pycocotools binary."""
import numpy as np

from . import rle

SCALE = 5.0


def _ring(xy):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1)
    if xy.size == 0 or xy.size % 2:
        raise ValueError("a polygon is a flat list [x0, y0, x1, y1, ...] of at least one point, got %d numbers" % xy.size)
    return xy


def polygon_points(xy):
    """Steps 1 and 2: the int64 points (u [m], v [m]) along the closed boundary on the 5x grid, edge after edge."""
    xy = _ring(xy)
    X = (SCALE * xy[0::2] + 0.5).astype(np.int64)  # astype truncates toward zero like (int)
    Y = (SCALE * xy[1::2] + 0.5).astype(np.int64)
    xs, ys, xe, ye = X, Y, np.roll(X, -1), np.roll(Y, -1)
    dx, dy = np.abs(xe - xs), np.abs(ys - ye)
    xmajor = dx >= dy
    flip = (xmajor & (xs > xe)) | (~xmajor & (ys > ye))
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    length = np.where(xmajor, dx, dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(xmajor, (ye - ys).astype(np.float64), (xe - xs).astype(np.float64)) / length.astype(np.float64)
    n = length + 1
    edge = np.repeat(np.arange(len(n)), n)
    d = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    t = np.where(flip[edge], length[edge] - d, d)
    xm = xmajor[edge]
    minor0 = np.where(xm, ys[edge], xs[edge]).astype(np.float64)
    prod = np.where(length[edge] > 0, s[edge], 0.0) * t.astype(np.float64)  # a point edge never uses s (0 / 0)
    minor = ((minor0 + prod) + 0.5).astype(np.int64)
    major = t + np.where(xm, xs[edge], ys[edge])
    return np.where(xm, major, minor), np.where(xm, minor, major)


def crossings_of_points(u, v, h, w):
    """Step 3 in its float form: the scan positions, in the order of the point pairs that yield them."""
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    keep = u1 != u0
    u0, u1, v0, v1 = u0[keep], u1[keep], v0[keep], v1[keep]
    xd = (np.where(u1 < u0, u1, u1 - 1).astype(np.float64) + 0.5) / SCALE - 0.5
    ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = (np.minimum(v0, v1).astype(np.float64) + 0.5) / SCALE - 0.5
    yd = np.ceil(np.clip(yd, 0, h))
    return (xd[ok].astype(np.int64) * int(h) + yd[ok].astype(np.int64)).astype(np.int64)


def polygon_crossings(xy, h, w):
    """int64 scan positions a = xd h + yd (0 <= a <= h w) of the polygon's crossings, unsorted, duplicates kept."""
    u, v = polygon_points(xy)
    return crossings_of_points(u, v, int(h), int(w))


def polygon_to_mask(xy, h, w):
    """One polygon -> uint8 [h, w] of 0/1: the prefix parity of its crossings over the column-major scan."""
    h, w = int(h), int(w)
    a = polygon_crossings(xy, h, w)
    toggles = np.bincount(a, minlength=h * w + 1)[: h * w]
    return (np.cumsum(toggles) & 1).astype(np.uint8).reshape(w, h).T


def polygons_to_bitmask(polygons, h, w):
    """list of flat polygons -> bool [h, w], the union of the polygons' masks (the reference's function of this name).  An
    empty list gives an all-zero mask (the reference would hand pycocotools' merge an empty list)."""
    out = np.zeros((int(h), int(w)), dtype=bool)
    for p in polygons:
        out |= polygon_to_mask(p, h, w).astype(bool)
    return out


def polygons_to_rle(polygons, h, w):
    """The compressed RLE dict of `polygons_to_bitmask` (cocoapi's annToRLE for a polygon annotation)."""
    return rle.encode(polygons_to_bitmask(polygons, h, w))
