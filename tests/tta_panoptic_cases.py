"""Shared inputs of the semantic / panoptic test-time-augmentation tests (tests/test_tta_panoptic_host.py,
tests/test_gpu_tta_panoptic.py): the view lists of the accumulate kernel's cases, their logits, and the
float64 definition of the mean of the views' logits."""
import numpy as np

# name -> (C, H, W, views); a view is (h, w, flipped)
_MIXED_18 = [(33, 257), (33, 257), (17, 129), (17, 129), (66, 514), (66, 514), (20, 150), (20, 151), (41, 300), (41, 301),
             (50, 400), (49, 399), (33, 200), (25, 257), (11, 90), (12, 91), (70, 520), (3, 5)]
CASES = {
    # identity, down- and up-scaling by 2, each plain and flipped; odd width under the flip
    "c28_37x53_v6": (28, 37, 53, [(37, 53, 0), (37, 53, 1), (19, 27, 0), (19, 27, 1), (74, 106, 0), (74, 106, 1)]),
    "c1_1x1_v1": (1, 1, 1, [(1, 1, 0)]),
    # the register limit; a wide row over two blocks; strong up- and down-scaling with the edge clamps
    "c64_8x300_v2": (64, 8, 300, [(5, 7, 1), (16, 600, 0)]),
    # one-row and one-column sources
    "c3_64x96_v2": (3, 64, 96, [(1, 9, 0), (9, 1, 1)]),
    "c28_33x257_v18": (28, 33, 257, [(h, w, k % 2) for k, (h, w) in enumerate(_MIXED_18)]),
}
MAGNITUDE = 8.0  # the logits are uniform in [-MAGNITUDE, MAGNITUDE]


def bound(num_views, magnitude=MAGNITUDE):
    """|float32 result - float64 definition| <= (V + 8) * 2^-24 * M: a bilinear term carries at most six roundings of values
    bounded by M, the sequential sum of V such terms at most (V - 1) u V M, the division by V one more rounding."""
    return (num_views + 8) * 2.0 ** -24 * magnitude


def make_views(name, seed=0, pad=(3, 5), fill=np.nan):
    """The logits of a case: per view a float32 [C, h + pad[0], w + pad[1]] block whose top-left [C, h, w] window holds the
    view (uniform in [-MAGNITUDE, MAGNITUDE]) and whose padding holds `fill`.  Returns (blocks, windows, flips)."""
    c, _, _, views = CASES[name]
    rs = np.random.RandomState(seed)
    blocks = []
    for h, w, _ in views:
        block = np.full((c, h + pad[0], w + pad[1]), fill, dtype=np.float32)
        block[:, :h, :w] = rs.uniform(-MAGNITUDE, MAGNITUDE, size=(c, h, w)).astype(np.float32)
        blocks.append(block)
    return blocks, [(h, w) for h, w, _ in views], [bool(f) for _, _, f in views]


def _taps(n_in, n_out):
    """One axis of F.interpolate(mode="bilinear", align_corners=False) as the kernels compute it, every step rounded to
    float32: (i0, i1, weight of i0, weight of i1) for the n_out outputs."""
    scale = np.float32(n_in) / np.float32(n_out)
    o = np.arange(n_out, dtype=np.float32)
    s = np.maximum(scale * (o + np.float32(0.5)) - np.float32(0.5), np.float32(0.0))
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    lo = s - i0.astype(np.float32)
    hi = np.float32(1.0) - lo
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return i0, i1, hi.astype(np.float64), lo.astype(np.float64)


def view_term_f64(view, window, flipped, H, W):
    """sem_seg_postprocess(view[:, :h, :w], (h, w), H, W), mirrored along x when flipped: float32 coordinates and weights,
    float64 products and sums.  The view itself where (h, w) == (H, W)."""
    h, w = window
    v = np.asarray(view)[:, :h, :w].astype(np.float64)
    if (h, w) == (H, W):
        term = v
    else:
        y0, y1, hy, ly = _taps(h, H)
        x0, x1, hx, lx = _taps(w, W)
        top = hx * v[:, y0][:, :, x0] + lx * v[:, y0][:, :, x1]
        bottom = hx * v[:, y1][:, :, x0] + lx * v[:, y1][:, :, x1]
        term = hy[:, None] * top + ly[:, None] * bottom
    return term[:, :, ::-1] if flipped else term


def mean_logits_f64(views, windows, flips, H, W):
    """The mean over the views of their terms, summed in view order and divided by V, in float64: [C, H, W]."""
    acc = None
    for view, window, flipped in zip(views, windows, flips):
        term = view_term_f64(view, window, flipped, H, W)
        acc = term if acc is None else acc + term
    return acc / float(len(views))
