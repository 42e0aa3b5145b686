"""Shared inputs of the test-time-augmentation tests (tests/test_tta_host.py, tests/test_gpu_tta.py): the 6-view image case, view
geometries for the box kernels with their numpy float32 definitions, and the mask-mean cases."""
import numpy as np
import torch

from u2seg_amd.data import transforms as T
from u2seg_amd.modeling.test_time_augmentation import DatasetMapperTTA, apply_box_f32

MIN_SIZES, MAX_SIZE = (32, 54, 80), 100          # of a 54 x 81 input: down-scaling, identity, up-scaling with MAX_SIZE binding
VIEW_SHAPES = [(32, 48), (32, 48), (54, 81), (54, 81), (67, 100), (67, 100)]   # by hand from get_output_shape's rule
THRESH = np.float32(1e-8)


def mapper():
    return DatasetMapperTTA(min_sizes=MIN_SIZES, max_size=MAX_SIZE, flip=True)


def image_input(pre_resize=True, seed=5):
    """A 54 x 81 uint8 input whose original image is 108 x 162 (pre_resize) or the input itself."""
    rs = np.random.RandomState(seed)
    # smooth structure plus noise: a resize of pure noise would hide an off-by-one in the tables behind rounding to mid-grey
    yy, xx = np.mgrid[0:54, 0:81]
    base = np.stack([(3 * xx + yy) % 256, (5 * yy + 2 * xx) % 256, (xx * yy) % 256]).astype(np.int64)
    image = np.clip(base + rs.randint(-20, 21, size=base.shape), 0, 255).astype(np.uint8)
    h, w = (108, 162) if pre_resize else (54, 81)
    return {"image": torch.from_numpy(image), "height": h, "width": w}


def nan_equal(a, b):
    """torch.equal with NaNs in the same places counted as equal (a NaN row stays a NaN row, the bits of the rest are compared)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros((), dtype=a.dtype)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


# ---- box kernels ----------------------------------------------------------------------------------------------------------------
def box_views():
    """Two images with different clip sizes and five views: (image, TransformList original -> view).  Image 0 is its own
    original (no pre-resize), image 1 was resized to its input; flips with and without a pre-resize."""
    pre = T.ResizeTransform(333, 517, 200, 311)          # image 1: original 333 x 517, input 200 x 311
    return [
        (0, T.TransformList([T.ResizeTransform(150, 217, 97, 140)])),
        (0, T.TransformList([T.ResizeTransform(150, 217, 211, 305), T.HFlipTransform(305)])),
        (0, T.TransformList([T.ResizeTransform(150, 217, 150, 217), T.HFlipTransform(217)])),
        (1, T.TransformList([pre, T.ResizeTransform(200, 311, 131, 204)])),
        (1, T.TransformList([pre, T.ResizeTransform(200, 311, 263, 409), T.HFlipTransform(409)])),
    ]


BOX_CLIP = [(150, 217), (333, 517)]   # (height, width) of the two originals


def view_size(tfm):
    r = [t for t in tfm.transforms if isinstance(t, T.ResizeTransform)][-1]
    return r.new_h, r.new_w


def random_boxes(rs, n, h, w, special=True):
    """n float32 boxes around an h x w canvas, a good part of them outside it; with `special` row 1 holds a NaN and row 2 an inf
    (when there are that many)."""
    x = np.sort(rs.uniform(-0.25 * w, 1.25 * w, size=(n, 2)), axis=1)
    y = np.sort(rs.uniform(-0.25 * h, 1.25 * h, size=(n, 2)), axis=1)
    b = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)
    if special and n > 2:
        b[1, 0], b[2, 3] = np.nan, np.inf
    return b


def detections_case(n, seed=11):
    """n detections spread over the five views (view 2 keeps zero rows), scores around the merge threshold: (per-view boxes,
    per-view scores).  Scores: uniform, with exact 1e-8 (float32), the next float above it, 0, a NaN and an inf mixed in."""
    rs = np.random.RandomState(seed + n)
    views = box_views()
    share = np.array([0.3, 0.25, 0.0, 0.25, 0.2])
    counts = np.floor(share * n).astype(int)
    counts[0] += n - counts.sum()
    boxes, scores = [], []
    for (_, tfm), c in zip(views, counts):
        h, w = view_size(tfm)
        boxes.append(random_boxes(rs, c, h, w))
        s = rs.uniform(0, 1, size=c).astype(np.float32)
        for k, v in enumerate([THRESH, np.nextafter(THRESH, np.float32(1)), np.float32(0), np.float32(np.nan), np.float32(np.inf)]):
            if 3 + k < c:
                s[3 + k] = v
        scores.append(s)
    return boxes, scores


def to_original_expected(boxes, scores):
    """The numpy float32 definition of u2_tta_boxes_to_original for detections_case's layout."""
    out_b, out_c = [], []
    for (im, tfm), b, s in zip(box_views(), boxes, scores):
        m = apply_box_f32(tfm, b, inverse=True)
        h, w = BOX_CLIP[im]
        lim = np.array([w, h, w, h], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            out_c.append(np.isfinite(m).all(axis=1) & np.isfinite(s) & (s > THRESH))
            out_b.append(np.minimum(np.maximum(m, np.float32(0)), lim))   # Boxes.clip; a NaN stays
    return np.concatenate(out_b).astype(np.float32), np.concatenate(out_c)


def to_views_expected(per_image_boxes):
    """The numpy float32 definition of u2_tta_boxes_to_views: per view, the boxes of its image mapped forward, not clipped."""
    return [apply_box_f32(tfm, per_image_boxes[im]) for im, tfm in box_views()]


# ---- mask mean ------------------------------------------------------------------------------------------------------------------
# (views, rows) per image of a launch
REDUCE_CASES = [[(1, 1), (2, 37)], [(3, 0), (18, 37)], [(18, 1), (2, 0)], [(3, 37)], [(2, 0)]]


def reduce_case(images, side, seed=3):
    """Per image a list of V float32 [R, 1, P, P] probability tensors and the flip flag of every view (alternating, the first
    view of the second image flipped)."""
    g = torch.Generator().manual_seed(seed + side + sum(v * 100 + r for v, r in images))
    probs, flips = [], []
    for i, (v, r) in enumerate(images):
        probs.append([torch.rand((r, 1, side, side), generator=g, dtype=torch.float32) for _ in range(v)])
        flips.append([(k + i) % 2 for k in range(v)])
    return probs, flips


def reduce_expected(probs, flips):
    """The sequential float32 loop on the host: per image sum_v (flipped view mirrored) in view order, one division by float(V)."""
    out = []
    for views, fl in zip(probs, flips):
        acc = None
        for p, f in zip(views, fl):
            p = p.flip(dims=[3]) if f else p
            acc = p.clone() if acc is None else acc + p
        out.append(acc / float(len(views)))
    return torch.cat(out)


def reduce_exact_mean(probs, flips):
    out = []
    for views, fl in zip(probs, flips):
        acc = sum((p.flip(dims=[3]) if f else p).double() for p, f in zip(views, fl))
        out.append(acc / len(views))
    return torch.cat(out)
