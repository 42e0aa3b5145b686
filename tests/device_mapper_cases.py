"""Shared cases of the device-mapper tests (tests/test_device_mapper_host.py on the CPU, tests/test_gpu_device_mapper.py on
the GPU): the size pairs, the image kinds, the mask shapes, and the PIL / numpy references, computed once per process."""
import functools

import numpy as np
from PIL import Image

from u2seg_amd.data import device_mapper as dm
from u2seg_amd.data import rle

# (source (h, w), target (H, W)): 1 x 1, an upscale from one row, the two one-axis identities, an upscale (3 taps), a strong
# downscale (9 taps), a mild one, a large upscale, and one full-size pair (short edge 427 -> 800)
SIZE_PAIRS = [((1, 1), (1, 1)), ((1, 7), (3, 5)), ((5, 3), (5, 9)), ((9, 5), (4, 5)), ((48, 64), (80, 107)),
              ((120, 90), (31, 23)), ((37, 53), (24, 34)), ((33, 71), (240, 516)), ((427, 640), (800, 1199))]
FLIPS = [(False, False), (True, False), (False, True), (True, True)]  # (horizontal, vertical)
IMAGE_KINDS = ("zeros", "full", "random", "checker")


@functools.lru_cache(maxsize=None)
def source(h, w, kind="random"):
    """(image uint8 [h, w, 3], label map uint8 [h, w] with the value 255 in it)."""
    rs = np.random.RandomState(1000 * h + w)
    if kind == "zeros":
        img = np.zeros((h, w, 3), dtype=np.uint8)
    elif kind == "full":
        img = np.full((h, w, 3), 255, dtype=np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
        img[:, :, 1] = 255 - img[:, :, 1]
    else:
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    lab = rs.randint(0, 256, (h, w)).astype(np.uint8)
    lab.flat[rs.randint(0, h * w)] = 255
    lab.flat[0] = 255
    for a in (img, lab):
        a.setflags(write=False)
    return img, lab


def flipped(a, hflip, vflip):
    a = a[:, ::-1] if hflip else a
    return a[::-1] if vflip else a


@functools.lru_cache(maxsize=None)
def pil_resized(h, w, H, W, kind="random"):
    """(PIL bilinear resize of the image, PIL nearest resize of the label map), unflipped."""
    img, lab = source(h, w, kind)
    return (np.asarray(Image.fromarray(img).resize((W, H), Image.BILINEAR)),
            np.asarray(Image.fromarray(lab, mode="L").resize((W, H), Image.NEAREST)))


def pil_nearest_index(n, out):
    """The source index PIL's nearest resize reads for every output index of an axis of length n resized to out, recovered
    from the pixels: row 0 carries index % 256, row 1 index // 256."""
    idx = np.arange(n)
    two = np.stack([idx % 256, idx // 256]).astype(np.uint8)
    got = np.asarray(Image.fromarray(two, mode="L").resize((out, 2), Image.NEAREST)).astype(np.int64)
    return got[1] * 256 + got[0]


def counts_of_mask(mask):
    """Uncompressed RLE counts of a 0/1 array [h, w] (column-major scan, first run zeros)."""
    return rle.counts_of(rle.encode(np.asarray(mask, dtype=np.uint8)))


def unsampled_pixel(h, w, tables):
    """A source pixel (y, x) no output pixel reads through the nearest tables (None when every row or every column is read)."""
    ys = np.setdiff1d(np.arange(h), tables["ny"])
    xs = np.setdiff1d(np.arange(w), tables["nx"])
    if ys.size == 0 and xs.size == 0:
        return None
    return (int(ys[0]) if ys.size else 0, int(xs[0]) if xs.size else 0)


def mask_shapes(h, w, tables=None):
    """Named source masks [h, w] of the mask kernel's cases, as count lists."""
    out = {}
    out["empty"] = [h * w]
    out["full"] = [0, h * w]
    for name, (y, x) in {"corner_tl": (0, 0), "corner_tr": (0, w - 1), "corner_bl": (h - 1, 0), "corner_br": (h - 1, w - 1)}.items():
        m = np.zeros((h, w), dtype=np.uint8)
        m[y, x] = 1
        out[name] = counts_of_mask(m)
    m = np.zeros((h, w), dtype=np.uint8)
    m[h // 2, :] = 1
    out["row_stripe"] = counts_of_mask(m)
    m = np.zeros((h, w), dtype=np.uint8)
    m[:, w // 3] = 1
    out["col_stripe"] = counts_of_mask(m)
    out["checker"] = [1] * (h * w)  # alternating along the column-major scan: h * w runs; a checkerboard when h is odd
    if tables is not None:
        px = unsampled_pixel(h, w, tables)
        if px is not None:
            m = np.zeros((h, w), dtype=np.uint8)
            m[px] = 1
            out["vanishing"] = counts_of_mask(m)
    return out


def record(h, w, H, W, hflip=False, vflip=False, count_lists=(), kind="random", labels=True):
    """A raw record built without files: source of `kind`, the given masks (count lists), one box and class per mask."""
    img, lab = source(h, w, kind)
    tables = dm.build_tables(h, w, H, W, hflip, vflip)
    ends = [dm.run_ends(c, h, w) for c in count_lists]
    boxes = np.tile(np.array([[0, 0, W, H]], dtype=np.float32), (len(ends), 1))
    return dm.make_raw_record({"height": h, "width": w, "image_id": 1000 * h + w}, img, lab if labels else None, tables, ends,
                              boxes, list(range(len(ends))), has_masks=True)


def host_outputs(rec):
    """(image [3, H, W], label map [H, W] or None, masks bool [N, H, W], counts int32 [N]) of a raw record by the host
    definitions."""
    meta = rec[dm.RAW_KEY]
    tables, ends = dm.unpack_tables(meta, rec["dm_tables"].numpy())
    tables["x_identity"], tables["y_identity"] = meta["x_identity"], meta["y_identity"]
    image = dm.host_image(rec["dm_image"].numpy(), tables)
    labels = dm.host_labels(rec["dm_sem_seg"].numpy(), tables) if "dm_sem_seg" in rec else None
    masks, counts = dm.host_masks(ends, meta["h"], tables)
    return image, labels, masks, counts
