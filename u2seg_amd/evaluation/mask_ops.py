"""Per-image mask work of the "segm" task: COCO run-length strings of the predicted masks and the pixel counts that mask
IoU needs (intersection of every predicted mask with every ground-truth mask of the image, and both areas).

Two paths with identical results.  Host: data/rle.py's encode / decode in numpy, which is the definition.  Device
(csrc/maskeval.hip, taken whenever the masks live on a GPU): the byte canvases are packed into column-major bit planes once,
the strings are made from the planes (count -> scan -> lengths -> scan -> emit; the scans are torch.cumsum), the
ground truth comes up as uncompressed counts and becomes planes there, the intersections are popcounts of plane & plane.
One call of `mask_batch` costs two host synchronisations and two device-to-host transfers whatever the number of images:
the arena size, then strings + string ends + areas + boxes + intersections in one buffer.  `counters` counts them.

Ground truth must be an RLE dict (compressed or uncompressed counts); polygons are out of scope."""
import ctypes

import numpy as np
import torch

from .. import _hip
from ..data import rle

counters = {"host_syncs": 0, "d2h_transfers": 0}


class _MaskImage(ctypes.Structure):
    """Mirror of U2MaskImage (include/u2seg_hip.h)."""

    _fields_ = [("first", ctypes.c_int), ("n", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("in_offset", ctypes.c_longlong), ("plane_offset", ctypes.c_longlong), ("col_offset", ctypes.c_longlong)]


class _PairImage(ctypes.Structure):
    """Mirror of U2PairImage (include/u2seg_hip.h)."""

    _fields_ = [("dt_offset", ctypes.c_longlong), ("gt_offset", ctypes.c_longlong), ("out_offset", ctypes.c_longlong),
                ("D", ctypes.c_int), ("G", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("dt_first", ctypes.c_int), ("pad_", ctypes.c_int)]


def is_polygon(segmentation):
    return not isinstance(segmentation, dict)


def gt_counts(ann, height, width, image_id=None):
    """The uncompressed counts of a ground-truth annotation's RLE, checked against the image size."""
    seg = ann.get("segmentation")
    where = "annotation %s of image %s" % (ann.get("id"), ann.get("image_id", image_id))
    if seg is None or is_polygon(seg):
        raise NotImplementedError("%s: mask evaluation needs RLE ground truth; polygon segmentations are not supported "
                                  "(no polygon rasteriser in this project)" % where)
    if [int(v) for v in seg["size"]] != [int(height), int(width)]:
        raise ValueError("%s: ground-truth RLE of size %s, prediction of size %s" % (where, list(seg["size"]), [height, width]))
    counts = rle.counts_of(seg)
    if sum(counts) != height * width or any(c < 0 for c in counts):
        raise ValueError("%s: RLE counts sum to %d, mask has %d pixels" % (where, sum(counts), height * width))
    return counts


def words_per_column(h):
    return (int(h) + 63) // 64


def unpack_planes(planes, n, h, w):
    """int64 [n * w * ceil(h / 64)] plane words (host) -> uint8 [n, h, w] and the padding bits [n, w, pad] (must be zero)."""
    wpc = words_per_column(h)
    words = np.asarray(planes).view(np.uint64).reshape(n, w, wpc)
    bits = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(n, w, wpc * 64)
    return bits[:, :, :h].transpose(0, 2, 1).copy(), bits[:, :, h:]


def _layout(sizes, counts):
    """Descriptors of a ragged batch: image i has counts[i] masks of sizes[i]; images without pixels or masks get n = 0."""
    descs = (_MaskImage * max(len(sizes), 1))()
    first = words = cols = 0
    for i, ((h, w), n) in enumerate(zip(sizes, counts)):
        d = descs[i]
        n = n if h * w > 0 else 0
        d.first, d.n, d.H, d.W, d.in_offset, d.plane_offset, d.col_offset = first, n, int(h), int(w), 0, words, cols
        first += n
        words += n * w * words_per_column(h)
        cols += n * w
    return descs, first, words, cols


def _sync_fetch(t):
    counters["host_syncs"] += 1
    counters["d2h_transfers"] += 1
    return t.cpu()


def planes_from_counts(counts_per_image, sizes, device):
    """Ground-truth planes on the device from uncompressed counts: counts_per_image[i] = list (per mask) of count lists.
    Returns (planes int64, descriptors, number of masks)."""
    descs, m, words, _ = _layout(sizes, [len(c) for c in counts_per_image])
    planes = torch.empty(max(words, 1), dtype=torch.int64, device=device)
    if m:
        lists = [np.asarray(c, dtype=np.int32) for (h, w), masks in zip(sizes, counts_per_image) if h * w > 0 for c in masks]
        offs = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
        cum = torch.cumsum(torch.from_numpy(np.concatenate(lists)).to(device), 0, dtype=torch.int64)
        _hip.call("u2_mask_planes_from_counts", cum, torch.from_numpy(offs).to(device), planes, descs, len(sizes))
    return planes, descs, m


def _canvas_base(masks):
    """One base address + a byte offset per image for canvases that may sit in different allocations."""
    ptrs = [m.data_ptr() for m in masks if m.numel()]
    base = min(ptrs) if ptrs else 0
    return base, [(m.data_ptr() - base if m.numel() else 0) for m in masks]


def mask_batch(masks_list, gt_counts_list=None, strings=True):
    """masks_list: per image a bool / uint8 tensor [n_i, H_i, W_i] on one GPU.  gt_counts_list: per image a list of
    uncompressed count lists (already checked by gt_counts), or None.  Returns per image a dict with "rles" (when strings),
    "area" int64 [n_i], "bbox" float64 [n_i, 4] (x, y, w, h) and, with ground truth, "inter" int64 [n_i, G_i]."""
    dev = masks_list[0].device
    masks = []
    for m in masks_list:
        assert m.dim() == 3 and m.device == dev and m.dtype in (torch.bool, torch.uint8), (m.shape, m.device, m.dtype)
        m = m.contiguous()
        masks.append(m if m.data_ptr() % 16 == 0 else m.clone())
    sizes = [(int(m.shape[1]), int(m.shape[2])) for m in masks]
    nums = [int(m.shape[0]) for m in masks]
    descs, total, words, cols = _layout(sizes, nums)
    base, offsets = _canvas_base(masks)
    if base % 16 or any(o % 16 for o in offsets):  # cannot happen with whole allocations; then one packed copy is read instead
        chunks, offsets, off = [], [], 0
        for m in masks:
            offsets.append(off)
            pad = (-m.numel()) % 16
            chunks += [m.reshape(-1).view(torch.uint8), torch.zeros(pad, dtype=torch.uint8, device=dev)]
            off += m.numel() + pad
        packed = torch.cat(chunks)
        base = packed.data_ptr()
    for d, o in zip(descs, offsets):
        d.in_offset = int(o)
    nimg = len(sizes)
    planes = torch.empty(max(words, 1), dtype=torch.int64, device=dev)
    area = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    box = torch.zeros(max(total, 1) * 4, dtype=torch.int32, device=dev)
    parts = []
    if total:
        _hip.call("u2_mask_pack_planes", base, planes, area, box, descs, nimg)
    arena_bytes = 0
    if strings and total:
        colcnt = torch.empty(cols, dtype=torch.int32, device=dev)
        last3 = torch.empty(cols * 3, dtype=torch.int32, device=dev)
        _hip.call("u2_mask_rle_count", planes, colcnt, last3, descs, nimg)
        cntcum = torch.cumsum(colcnt, 0, dtype=torch.int64)
        # lastne from a prefix count and a scatter (torch.cummax scans a 1-d tensor with one work-group): slots[r] = the r-th
        # non-empty column, slots[0] = -1 = none, the last slot takes the empty columns' writes
        idx = torch.arange(cols, dtype=torch.int64, device=dev)
        rank = torch.cumsum(colcnt > 0, 0, dtype=torch.int64)
        slots = torch.full((cols + 2,), -1, dtype=torch.int64, device=dev)
        slots.scatter_(0, torch.where(colcnt > 0, rank, torch.full_like(rank, cols + 1)), idx)
        lastne = slots[rank]
        collen = torch.empty(cols, dtype=torch.int32, device=dev)
        _hip.call("u2_mask_rle_lengths", planes, colcnt, last3, cntcum, lastne, collen, descs, nimg)
        strcum = torch.cumsum(collen, 0, dtype=torch.int64)
        last_col = np.concatenate([d.col_offset + np.arange(1, d.n + 1, dtype=np.int64) * d.W - 1 for d in descs[:nimg]])
        ends = strcum[torch.from_numpy(last_col).to(dev)]
        counters["host_syncs"] += 1
        counters["d2h_transfers"] += 1
        arena_bytes = int(strcum[-1])  # the one value the host has to learn before it can size the arena
        arena = torch.empty(max(arena_bytes, 1), dtype=torch.uint8, device=dev)
        _hip.call("u2_mask_rle_emit", planes, colcnt, last3, cntcum, lastne, strcum, arena, arena_bytes, descs, nimg)
        parts += [arena[:arena_bytes], ends.view(torch.uint8)]
    parts += [area[:total].view(torch.uint8), box[: total * 4].view(torch.uint8)]
    n_inter = 0
    if gt_counts_list is not None:
        gt_planes, gdescs, _ = planes_from_counts(gt_counts_list, sizes, dev)
        pairs = (_PairImage * max(nimg, 1))()
        for i in range(nimg):
            p, d, g = pairs[i], descs[i], gdescs[i]
            p.dt_offset, p.gt_offset, p.out_offset = d.plane_offset, g.plane_offset, n_inter
            p.D, p.G, p.H, p.W, p.dt_first = d.n, g.n, d.H, d.W, d.first
            n_inter += d.n * g.n
        inter = torch.empty(max(n_inter, 1), dtype=torch.int32, device=dev)
        if n_inter:
            _hip.call("u2_mask_pair_counts", planes, gt_planes, box, inter, pairs, nimg)
        parts.append(inter[:n_inter].view(torch.uint8))
    host = _sync_fetch(torch.cat(parts)).numpy()
    pos = 0

    def take(nbytes, dtype):
        nonlocal pos
        out = host[pos : pos + nbytes].view(dtype)
        pos += nbytes
        return out

    if strings and total:
        text = take(arena_bytes, np.uint8).tobytes().decode("ascii")
        ends_h = [0] + take(8 * total, np.int64).tolist()
    area_h = take(4 * total, np.int32).astype(np.int64)
    box_h = take(16 * total, np.int32).reshape(total, 4).astype(np.float64)
    inter_h = take(4 * n_inter, np.int32).astype(np.int64) if gt_counts_list is not None else None
    out, ipos = [], 0
    for i, ((h, w), n) in enumerate(zip(sizes, nums)):
        d = descs[i]
        res = {}
        if d.n == n:
            sl = slice(d.first, d.first + n)
            res["area"], res["bbox"] = area_h[sl].copy(), box_h[sl].copy()
            if strings:
                res["rles"] = [{"size": [h, w], "counts": text[ends_h[m] : ends_h[m + 1]]} for m in range(d.first, d.first + n)]
        else:  # an image without pixels: nothing went to the device
            res["area"], res["bbox"] = np.zeros(n, dtype=np.int64), np.zeros((n, 4))
            if strings:
                res["rles"] = [{"size": [h, w], "counts": ""} for _ in range(n)]
        if gt_counts_list is not None:
            g = len(gt_counts_list[i])
            if d.n == n and h * w > 0:
                res["inter"] = inter_h[ipos : ipos + n * g].reshape(n, g).copy()
                ipos += n * g
            else:
                res["inter"] = np.zeros((n, g), dtype=np.int64)
        out.append(res)
    return out


def _host_image(masks, counts, h, w, strings=True):
    m = np.asarray(masks).astype(np.uint8)
    res = {}
    if strings:
        res["rles"] = [rle.encode(x) for x in m]
    res["area"] = m.sum(axis=(1, 2), dtype=np.int64)
    if counts is not None:
        gm = [rle.decode({"size": [h, w], "counts": c}) for c in counts]
        inter = np.zeros((len(m), len(gm)), dtype=np.int64)
        for j, g in enumerate(gm):
            inter[:, j] = (m & g[None]).sum(axis=(1, 2), dtype=np.int64)
        res["inter"] = inter
    return res


def mask_batch_any(masks_list, gt_counts_list=None, strings=True):
    """`mask_batch` on the device when the masks are there, the numpy definition otherwise ("rles", "area", "inter")."""
    if masks_list and masks_list[0].is_cuda:
        return mask_batch(masks_list, gt_counts_list, strings)
    return [_host_image(m.numpy(), None if gt_counts_list is None else gt_counts_list[i], int(m.shape[1]), int(m.shape[2]), strings)
            for i, m in enumerate(masks_list)]


def encode_masks(pred_masks):
    """bool / uint8 [K, H, W] (tensor or array) -> [{"size": [H, W], "counts": compressed str}]: rle.encode of every mask; on
    the device when the tensor is there."""
    if isinstance(pred_masks, torch.Tensor) and pred_masks.is_cuda:
        return mask_batch([pred_masks])[0]["rles"]
    m = pred_masks.numpy() if isinstance(pred_masks, torch.Tensor) else np.asarray(pred_masks)
    return [rle.encode(np.asarray(x, dtype=np.uint8)) for x in m]


def mask_pair_counts(pred_masks, gt_annotations, height, width):
    """inter int64 [D, G] = pixels shared by predicted mask d and ground-truth mask g, area_dt int64 [D], area_gt int64 [G].
    pred_masks: [D, height, width] tensor or array; gt_annotations: dicts with an RLE "segmentation" of that size."""
    counts = [gt_counts(a, height, width) for a in gt_annotations]
    area_gt = np.array([sum(c[1::2]) for c in counts], dtype=np.int64).reshape(len(counts))
    if not isinstance(pred_masks, torch.Tensor):
        pred_masks = torch.from_numpy(np.ascontiguousarray(np.asarray(pred_masks)).astype(np.uint8))
    assert tuple(pred_masks.shape[1:]) == (height, width), (pred_masks.shape, height, width)
    res = mask_batch_any([pred_masks], [counts], strings=False)[0]
    return res["inter"], res["area"], area_gt
