"""Per-image mask work of the "segm" task: COCO run-length strings of the predicted masks and the pixel counts that mask
IoU needs (intersection of every predicted mask with every ground-truth mask of the image, and both areas).

Two paths with identical results.  Host: data/rle.py's encode / decode in numpy, which is the definition.  Device
(csrc/maskeval.hip, taken whenever the masks live on a GPU): the byte canvases are packed into column-major bit planes once,
the strings are made from the planes (count -> scan -> lengths -> scan -> emit; the scans are torch.cumsum), the
ground truth comes up as uncompressed counts and becomes planes there, the intersections are popcounts of plane & plane.
One call of `mask_batch` costs two host synchronisations and two device-to-host transfers whatever the number of images:
the arena size, then strings + string ends + areas + boxes + intersections (+ ground-truth areas) in one buffer.  `counters`
counts them.

Ground truth is an RLE dict (compressed or uncompressed counts).  Polygon lists are refused unless the caller asks for them
(`polygons=True` / `gt=`): then they are rasterised by data/polygon.py's definition, on the device by csrc/polygon.hip into
planes next to the RLE ones, with the same number of synchronisations and transfers."""
import ctypes

import numpy as np
import torch

from .. import _hip
from ..data import polygon, rle

counters = {"host_syncs": 0, "d2h_transfers": 0}


class _MaskImage(ctypes.Structure):
    """Mirror of U2MaskImage (include/u2seg_hip.h)."""

    _fields_ = [("first", ctypes.c_int), ("n", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("in_offset", ctypes.c_longlong), ("plane_offset", ctypes.c_longlong), ("col_offset", ctypes.c_longlong)]


class _PolyMask(ctypes.Structure):
    """Mirror of U2PolyMask (include/u2seg_hip.h)."""

    _fields_ = [("H", ctypes.c_int), ("W", ctypes.c_int), ("plane_offset", ctypes.c_longlong),
                ("first_poly", ctypes.c_int), ("num_polys", ctypes.c_int)]


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


MAX_POLYGON_COORD = 1e8  # 5 x + .5 stays an int32 on the device


def gt_polygons(ann, image_id=None):
    """The polygons of a ground-truth annotation as float64 arrays [2 k], checked: every polygon a flat list of k >= 1 points
    (cocoapi rasterises what the json holds; dropping polygons of fewer than 3 points is the dataset loader's business)."""
    where = "annotation %s of image %s" % (ann.get("id"), ann.get("image_id", image_id))
    seg = ann.get("segmentation")
    if not isinstance(seg, (list, tuple)):
        raise ValueError("%s: segmentation of type %s is neither an RLE dict nor a list of polygons" % (where, type(seg).__name__))
    out = []
    for p in seg:
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        if p.size == 0 or p.size % 2:
            raise ValueError("%s: a polygon of %d numbers" % (where, p.size))
        if not (np.abs(p) <= MAX_POLYGON_COORD).all():
            raise ValueError("%s: polygon coordinates must be finite and within +-%g" % (where, MAX_POLYGON_COORD))
        out.append(p)
    return out


def gt_mask(ann, height, width, image_id=None):
    """The host definition of a ground-truth annotation's mask, uint8 [height, width]: RLE decoded, polygons rasterised."""
    if isinstance(ann.get("segmentation"), dict):
        return rle.decode({"size": [height, width], "counts": gt_counts(ann, height, width, image_id)})
    return polygon.polygons_to_bitmask(gt_polygons(ann, image_id), height, width).astype(np.uint8)


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


def planes_from_annotations(anns_per_image, sizes, device):
    """Ground-truth planes on the device from annotations whose "segmentation" is an RLE dict or a list of polygons:
    anns_per_image[i] = the annotation dicts of image i (size sizes[i]).  RLE annotations go through
    u2_mask_planes_from_counts, polygon annotations through u2_mask_planes_from_polygons; the launcher of the former wants an
    image's masks contiguous, so an image's planes are ordered RLE first.  Returns (planes int64, descriptors (n = masks of the
    image, plane_offset = its first plane), info: "order" = per image the annotation index of every plane, "m" = planes in
    all, "area" = int64 [m] on the host with the RLE masks' areas filled in, "poly_rows" = the planes that came from polygons
    and "poly_area" = their areas, int32 on the device).  Two uploads at most (one int64 buffer: count offsets, polygon offsets, vertices; the counts)."""
    nimg = len(sizes)
    descs = (_MaskImage * max(nimg, 1))()   # what the pair kernel needs: all planes of the image
    rdescs = (_MaskImage * max(nimg, 1))()  # the RLE planes of the image, for u2_mask_planes_from_counts
    pmasks, order, count_lists, polys, rle_area = [], [], [], [], []
    words = m = 0
    for i, ((h, w), anns) in enumerate(zip(sizes, anns_per_image)):
        h, w = int(h), int(w)
        is_rle = [isinstance(a.get("segmentation"), dict) for a in anns]
        parsed = [gt_counts(a, h, w) if r else gt_polygons(a) for a, r in zip(anns, is_rle)]
        idx = [k for k, r in enumerate(is_rle) if r] + [k for k, r in enumerate(is_rle) if not r]
        order.append(idx)
        n = len(anns) if h * w > 0 else 0
        nr = sum(is_rle) if n else 0
        nw = w * words_per_column(h)
        d, r = descs[i], rdescs[i]
        d.first, d.n, d.H, d.W, d.in_offset, d.plane_offset, d.col_offset = m, n, h, w, 0, words, 0
        r.first, r.n, r.H, r.W, r.in_offset, r.plane_offset, r.col_offset = len(count_lists), nr, h, w, 0, words, 0
        for j, k in enumerate(idx[:n]):
            if is_rle[k]:
                count_lists.append(np.asarray(parsed[k], dtype=np.int32))
                rle_area.append((m + j, int(sum(parsed[k][1::2]))))
            else:
                pm = _PolyMask()
                pm.H, pm.W, pm.plane_offset, pm.first_poly, pm.num_polys = h, w, words + j * nw, len(polys), len(parsed[k])
                pmasks.append((m + j, pm))
                polys += parsed[k]
        m += n
        words += n * nw
    planes = torch.empty(max(words, 1), dtype=torch.int64, device=device)
    area = np.zeros(m, dtype=np.int64)
    for row, v in rle_area:
        area[row] = v
    info = {"order": order, "m": m, "area": area, "poly_rows": [row for row, _ in pmasks],
            "poly_area": torch.zeros(len(pmasks), dtype=torch.int32, device=device)}
    if m == 0:
        return planes, descs, info
    offs = np.concatenate([[0], np.cumsum([len(c) for c in count_lists])]).astype(np.int64)
    poffs = np.concatenate([[0], np.cumsum([len(p) // 2 for p in polys])]).astype(np.int64)
    xy = np.concatenate(polys) if polys else np.zeros(0, dtype=np.float64)
    up = torch.from_numpy(np.concatenate([offs, poffs, xy.view(np.int64)])).to(device)
    if count_lists:
        cum = torch.cumsum(torch.from_numpy(np.concatenate(count_lists)).to(device), 0, dtype=torch.int64)
        _hip.call("u2_mask_planes_from_counts", cum, up[: len(offs)], planes, rdescs, nimg)
    if pmasks:
        pm = (_PolyMask * len(pmasks))(*[p for _, p in pmasks])
        need = int(_hip.call_nostream("u2_mask_polygon_scratch_words", pm, len(pmasks)))
        scratch = torch.empty(max(need, 1), dtype=torch.int64, device=device)
        _hip.call("u2_mask_planes_from_polygons", up[len(offs) + len(poffs) :].view(torch.float64),
                  up[len(offs) : len(offs) + len(poffs)], pm, len(pmasks), planes, info["poly_area"], scratch, need)
    return planes, descs, info


def _canvas_base(masks):
    """One base address + a byte offset per image for canvases that may sit in different allocations."""
    ptrs = [m.data_ptr() for m in masks if m.numel()]
    base = min(ptrs) if ptrs else 0
    return base, [(m.data_ptr() - base if m.numel() else 0) for m in masks]


def mask_batch(masks_list, gt_counts_list=None, strings=True, gt=None):
    """masks_list: per image a bool / uint8 tensor [n_i, H_i, W_i] on one GPU.  gt_counts_list: per image a list of
    uncompressed count lists (already checked by gt_counts), or None.  gt (instead of gt_counts_list): per image the list of
    ground-truth annotation dicts, RLE or polygon segmentations in any mix.  Returns per image a dict with "rles" (when
    strings), "area" int64 [n_i], "bbox" float64 [n_i, 4] (x, y, w, h) and, with ground truth, "inter" int64 [n_i, G_i]
    (columns in annotation order); with `gt` also "area_gt" int64 [G_i], the areas of the rasterised ground truth."""
    assert gt is None or gt_counts_list is None
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
    ginfo = None
    if gt is not None:
        gt_planes, gdescs, ginfo = planes_from_annotations(gt, sizes, dev)
        gt_counts_list = gt  # below only the number of ground truths per image is read
    elif gt_counts_list is not None:
        gt_planes, gdescs, _ = planes_from_counts(gt_counts_list, sizes, dev)
    if gt_counts_list is not None:
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
    if ginfo is not None:
        parts.append(ginfo["poly_area"].view(torch.uint8))
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
    if ginfo is not None:
        ginfo["area"][ginfo["poly_rows"]] = take(4 * len(ginfo["poly_rows"]), np.int32)
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
        if ginfo is not None:  # planes are RLE first: back to annotation order
            gd, order = gdescs[i], ginfo["order"][i]
            res["area_gt"] = np.zeros(len(order), dtype=np.int64)
            if gd.n:
                res["area_gt"][order] = ginfo["area"][gd.first : gd.first + gd.n]
            inter = np.empty_like(res["inter"])
            inter[:, order] = res["inter"]
            res["inter"] = inter
        out.append(res)
    return out


def _host_image(masks, counts, h, w, strings=True, anns=None):
    m = np.asarray(masks).astype(np.uint8)
    res = {}
    if strings:
        res["rles"] = [rle.encode(x) for x in m]
    res["area"] = m.sum(axis=(1, 2), dtype=np.int64)
    if counts is not None or anns is not None:
        if anns is not None:
            gm = [gt_mask(a, h, w) for a in anns]
            res["area_gt"] = np.array([g.sum(dtype=np.int64) for g in gm], dtype=np.int64).reshape(len(gm))
        else:
            gm = [rle.decode({"size": [h, w], "counts": c}) for c in counts]
        inter = np.zeros((len(m), len(gm)), dtype=np.int64)
        for j, g in enumerate(gm):
            inter[:, j] = (m & g[None]).sum(axis=(1, 2), dtype=np.int64)
        res["inter"] = inter
    return res


def mask_batch_any(masks_list, gt_counts_list=None, strings=True, gt=None):
    """`mask_batch` on the device when the masks are there, the numpy definition otherwise ("rles", "area", "inter" and, with
    `gt`, "area_gt")."""
    if masks_list and masks_list[0].is_cuda:
        return mask_batch(masks_list, gt_counts_list, strings, gt)
    return [_host_image(m.numpy(), None if gt_counts_list is None else gt_counts_list[i], int(m.shape[1]), int(m.shape[2]), strings,
                        None if gt is None else gt[i]) for i, m in enumerate(masks_list)]


def encode_masks(pred_masks):
    """bool / uint8 [K, H, W] (tensor or array) -> [{"size": [H, W], "counts": compressed str}]: rle.encode of every mask; on
    the device when the tensor is there."""
    if isinstance(pred_masks, torch.Tensor) and pred_masks.is_cuda:
        return mask_batch([pred_masks])[0]["rles"]
    m = pred_masks.numpy() if isinstance(pred_masks, torch.Tensor) else np.asarray(pred_masks)
    return [rle.encode(np.asarray(x, dtype=np.uint8)) for x in m]


def mask_pair_counts(pred_masks, gt_annotations, height, width, polygons=False):
    """inter int64 [D, G] = pixels shared by predicted mask d and ground-truth mask g, area_dt int64 [D], area_gt int64 [G].
    pred_masks: [D, height, width] tensor or array; gt_annotations: dicts with an RLE "segmentation" of that size.
    polygons=True: a "segmentation" may also be a list of polygons, rasterised by data/polygon.py's definition (on the device
    when the masks are there); area_gt is then the rasterised area."""
    if not polygons:
        counts = [gt_counts(a, height, width) for a in gt_annotations]
        area_gt = np.array([sum(c[1::2]) for c in counts], dtype=np.int64).reshape(len(counts))
    if not isinstance(pred_masks, torch.Tensor):
        pred_masks = torch.from_numpy(np.ascontiguousarray(np.asarray(pred_masks)).astype(np.uint8))
    assert tuple(pred_masks.shape[1:]) == (height, width), (pred_masks.shape, height, width)
    if polygons:
        res = mask_batch_any([pred_masks], strings=False, gt=[list(gt_annotations)])[0]
        return res["inter"], res["area"], res["area_gt"]
    res = mask_batch_any([pred_masks], [counts], strings=False)[0]
    return res["inter"], res["area"], area_gt
