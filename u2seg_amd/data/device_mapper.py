"""The training mapper with its pixel work left to the device (opt-in).

`DatasetMapper` decodes, resizes with PIL (bilinear image, nearest label map), decodes every RLE mask and resizes it, flips, and
ships target-size pixels.  `DeviceMapper` loads the same files and draws the same augmentation parameters from numpy's global
stream in the same order, but applies nothing to pixels: it returns a *raw record* - the source-size image and label map, the
RLE masks as run ends (never decoded), the boxes (transformed on the host as before) and small per-axis tables that say, for
every output index, which source indices feed it and with what weight.  With INPUT.CROP the record
holds the window's pixels and tables, the run ends of the whole annotation and the window's place in it; with masks the
boxes are then the masks' tight boxes, made on the device next to the decode.  csrc/augment.hip turns a batch of raw records into what
`DatasetMapper` would have produced (data/build.py: DevicePrefetcher), bit for bit: everything PIL does here is integer
arithmetic once the tables exist, and the tables are built below in float64 in PIL's own order of operations
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc; Geometry.c: ImagingScaleAffine).

The module also holds the host definitions of the three kernels (`host_image`, `host_labels`, `host_masks`): numpy functions
from a raw record to exactly what the kernels must write.  They are the yardstick of the GPU tests and are themselves pinned
against PIL and `DatasetMapper` on the CPU."""
import copy
import ctypes
import functools

import numpy as np
import torch

from ..structures import BitMasks, Boxes, Instances
from . import detection_utils as utils
from . import rle
from . import transforms as T
from .dataset_mapper import DatasetMapper, crop_from_config

PRECISION_BITS = 32 - 8 - 2  # Resample.c: coefficients carry 22 fractional bits
RAW_KEY = "dm_meta"          # a dict with this key is a raw record
TENSOR_KEYS = ("dm_image", "dm_sem_seg", "dm_tables", "dm_boxes", "dm_classes")


# ---- tables -------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=256)
def bilinear_axis(in_size, out_size):
    """PIL's bilinear coefficients of one axis: bounds int32 [out, 2] (first source index, tap count) and coefficients int32
    [out, ksize] with 22 fractional bits (zero behind the tap count).  Vectorised over the output indices; along the taps the
    operations keep PIL's order (the weights are summed left to right).  Read-only: a training run meets a few dozen
    (source, target) lengths, so the tables are kept."""
    in_size, out_size = int(in_size), int(out_size)
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = 0.0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # C's (int) truncates; the operand is > -1 here
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    k = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.abs(((k + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((w < 1.0) & (k < xmax[:, None]), 1.0 - w, 0.0)  # taps behind the count are 0: adding them changes nothing
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):  # the sum in PIL's order
        ww = ww + w[:, j]
    coef = np.where(ww[:, None] != 0.0, w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    fixed = np.where(coef < 0, -0.5 + coef * (1 << PRECISION_BITS), 0.5 + coef * (1 << PRECISION_BITS)).astype(np.int32)
    return _frozen(bounds, fixed)


def identity_axis(size):
    """The tables of an axis PIL does not resample: one tap of exactly 1.0 on the same index."""
    bounds = np.stack([np.arange(size, dtype=np.int32), np.ones(size, dtype=np.int32)], axis=1)
    return bounds, np.full((size, 1), 1 << PRECISION_BITS, dtype=np.int32)


@functools.lru_cache(maxsize=256)
def nearest_axis(in_size, out_size):
    """PIL's nearest source index per output index (ImagingScaleAffine: the coordinate starts at half a step and is advanced
    by repeated addition in double precision)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size == out_size:
        return _frozen(np.arange(out_size, dtype=np.int32))  # Image.resize returns a copy
    a = float(in_size) / out_size
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = 0.0 + a * 0.5
    pos = np.add.accumulate(steps)  # sequential additions, like the C loop
    idx = pos.astype(np.int64)      # COORD: (int) of a non-negative double
    if idx[-1] >= in_size:
        raise ValueError("nearest table %d -> %d leaves the source (PIL would write its fill value there)" % (in_size, out_size))
    return _frozen(idx.astype(np.int32))


def build_tables(h, w, H, W, hflip=False, vflip=False):
    """The per-axis tables of one sample: source (h, w) resized to (H, W), then flipped.  A flip reverses the output order of
    its axis' tables - nothing downstream knows about flips."""
    t = {"x_identity": w == W, "y_identity": h == H}
    t["bx_bounds"], t["bx_coef"] = identity_axis(w) if w == W else bilinear_axis(w, W)
    t["by_bounds"], t["by_coef"] = identity_axis(h) if h == H else bilinear_axis(h, H)
    t["nx"], t["ny"] = nearest_axis(w, W), nearest_axis(h, H)
    if hflip:
        for k in ("bx_bounds", "bx_coef", "nx"):
            t[k] = np.ascontiguousarray(t[k][::-1])
    if vflip:
        for k in ("by_bounds", "by_coef", "ny"):
            t[k] = np.ascontiguousarray(t[k][::-1])
    return t


def run_ends(counts, h, w):
    """Inclusive prefix sums of an RLE's counts (uint32): the column-major position behind every run."""
    c = np.asarray(counts, dtype=np.int64)
    if c.size == 0 or (c < 0).any() or int(c.sum()) != h * w:
        raise ValueError("RLE counts sum to %d, mask has %d pixels" % (int(c.sum()), h * w))
    return np.cumsum(c).astype(np.uint32)


_TABLE_ORDER = ("bx_bounds", "bx_coef", "by_bounds", "by_coef", "nx", "ny")


def pack_tables(tables, ends_per_mask):
    """One int32 array with every table and the run ends, and the element offset of each part in it:
    (array, {"bx_bounds": .., .., "mask_offs": ..}).  mask_offs points at [num_masks + 1] offsets (relative to the array) of
    the masks' run ends."""
    parts, where, cursor = [], {}, 0
    for k in _TABLE_ORDER:
        a = np.ascontiguousarray(tables[k], dtype=np.int32).reshape(-1)
        where[k] = cursor
        parts.append(a)
        cursor += a.size
    where["mask_offs"] = cursor
    n = len(ends_per_mask)
    offs = cursor + n + 1 + np.concatenate([[0], np.cumsum([len(e) for e in ends_per_mask])]).astype(np.int64)
    parts.append(offs.astype(np.int32))
    parts += [np.asarray(e, dtype=np.uint32).view(np.int32) for e in ends_per_mask]
    return np.concatenate(parts).astype(np.int32, copy=False), where


def unpack_tables(meta, flat):
    """The tables of a raw record as named arrays (views of `flat`, the record's int32 array) and the list of run ends."""
    flat = np.asarray(flat)
    H, W, kx, ky, o = meta["H"], meta["W"], meta["kx"], meta["ky"], meta["offsets"]
    t = {"bx_bounds": flat[o["bx_bounds"]:o["bx_bounds"] + 2 * W].reshape(W, 2),
         "bx_coef": flat[o["bx_coef"]:o["bx_coef"] + W * kx].reshape(W, kx),
         "by_bounds": flat[o["by_bounds"]:o["by_bounds"] + 2 * H].reshape(H, 2),
         "by_coef": flat[o["by_coef"]:o["by_coef"] + H * ky].reshape(H, ky),
         "nx": flat[o["nx"]:o["nx"] + W], "ny": flat[o["ny"]:o["ny"] + H]}
    n = meta["num_masks"]
    offs = flat[o["mask_offs"]:o["mask_offs"] + n + 1]
    ends = [flat[offs[m]:offs[m + 1]].view(np.uint32) for m in range(n)]
    return t, ends


# ---- host definitions of the kernels --------------------------------------------------------------------------------------
def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _filter_axis0(a, bounds, coef):
    """out[i] = clip8((2^21 + sum_k a[first_i + k] * coef[i, k]) >> 22) along axis 0 of a uint8 array, in int32 like the kernel."""
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.uint8)
    a32 = a.astype(np.int32)
    for i, (first, n) in enumerate(bounds):
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for k in range(n):
            acc += a32[first + k] * coef[i, k]
        out[i] = _clip8(acc)
    return out


def host_image(image, tables):
    """uint8 [h, w, 3] -> CHW uint8 [3, H, W]: the horizontal pass over the rows the vertical pass reads, rounded to uint8,
    then the vertical pass; a pass whose axis is an identity only reorders."""
    image = np.asarray(image)
    if tables["x_identity"]:
        tmp = image[:, tables["bx_bounds"][:, 0]]
    else:
        tmp = _filter_axis0(image.transpose(1, 0, 2), tables["bx_bounds"], tables["bx_coef"]).transpose(1, 0, 2)
    if tables["y_identity"]:
        out = tmp[tables["by_bounds"][:, 0]]
    else:
        out = _filter_axis0(tmp, tables["by_bounds"], tables["by_coef"])
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def host_labels(labels, tables):
    """uint8 [h, w] -> int64 [H, W] through the two index tables."""
    return np.asarray(labels)[tables["ny"][:, None], tables["nx"][None, :]].astype(np.int64)


def host_masks(ends_per_mask, h, tables, window=None):
    """Run ends -> (bool [N, H, W], int32 [N] pixel counts): output pixel (y, x) reads source (ny[y], nx[x]), whose column-major
    position is p = nx[x] * h + ny[y]; its value is the parity of the number of run ends <= p.  window = (x0, y0, mask_h,
    mask_w): the tables index a window at (x0, y0) of a mask_h x mask_w code, p = (x0 + nx[x]) * mask_h + y0 + ny[y]."""
    H, W = len(tables["ny"]), len(tables["nx"])
    x0, y0, h = (0, 0, h) if window is None else (window[0], window[1], window[2])
    p = (x0 + tables["nx"].astype(np.int64))[None, :] * h + (y0 + tables["ny"].astype(np.int64))[:, None]
    out = np.zeros((len(ends_per_mask), H, W), dtype=bool)
    for m, ends in enumerate(ends_per_mask):
        out[m] = (np.searchsorted(np.asarray(ends, dtype=np.int64), p.reshape(-1), side="right") & 1).reshape(H, W).astype(bool)
    return out, out.sum(axis=(1, 2)).astype(np.int32)


def finish_on_host(raw):
    """A raw record -> the dict `DatasetMapper` returns, computed with the host definitions (tests, and consumers without a
    GPU that want to look at a raw record)."""
    meta = raw[RAW_KEY]
    tables, ends = unpack_tables(meta, raw["dm_tables"].numpy())
    tables["x_identity"], tables["y_identity"] = meta["x_identity"], meta["y_identity"]
    out = {k: v for k, v in raw.items() if k != RAW_KEY and k not in TENSOR_KEYS}
    out["image"] = torch.from_numpy(host_image(raw["dm_image"].numpy(), tables))
    if "dm_sem_seg" in raw:
        out["sem_seg"] = torch.from_numpy(host_labels(raw["dm_sem_seg"].numpy(), tables))
    if meta["has_instances"]:
        masks = counts = tight = None
        if meta["has_masks"]:
            masks, counts = host_masks(ends, meta["h"], tables, meta.get("window"))
            masks = torch.from_numpy(masks)
            if meta.get("recompute_boxes"):
                tight = BitMasks(masks).get_bounding_boxes().tensor
        out["instances"] = assemble_instances(meta, raw["dm_boxes"], raw["dm_classes"], masks, counts, tight)
    return out


def assemble_instances(meta, boxes, classes, masks, counts, tight=None):
    """Instances from the box-kept rows: rows whose mask has no pixel are dropped (the by_mask half of
    filter_empty_instances).  `counts`: host int32 [N]; the tensors may live on any device.  tight (fp32 [N, 4], records with
    recompute_boxes): the masks' tight boxes, which replace `boxes`; there the host kept every row, a mask with a pixel has a
    tight box of at least 1 x 1 and an empty one a zero box, so count > 0 is by_box & by_mask."""
    if tight is not None:
        boxes = tight
    if masks is not None and counts is not None and not bool((np.asarray(counts) > 0).all()):
        keep = torch.from_numpy(np.flatnonzero(np.asarray(counts) > 0)).to(boxes.device)
        boxes, classes, masks = boxes[keep], classes[keep], masks[keep]
    inst = Instances((meta["H"], meta["W"]))
    inst.gt_boxes = Boxes(boxes)
    inst.gt_classes = classes
    if masks is not None:
        inst.gt_masks = BitMasks(masks)
    return inst


# ---- the device side: a batch of raw records through csrc/augment.hip -----------------------------------------------------
class _AugWindow(ctypes.Structure):
    """Mirror of U2AugWindow (include/u2seg_hip.h)."""

    _fields_ = [(k, ctypes.c_int) for k in ("x0", "y0", "mask_h", "mask_w")]


def describe_windows(records):
    """The windows of a batch for u2_aug_rle_masks_boxes (a record without one: the whole of its own h x w), or None when no
    record of the batch has masks and a window (or boxes to recompute) - such a batch takes u2_aug_rle_masks."""
    if not any((d[RAW_KEY].get("window") is not None or d[RAW_KEY].get("recompute_boxes")) and d[RAW_KEY]["num_masks"]
               for d in records):
        return None
    windows = (_AugWindow * len(records))()
    for win, d in zip(windows, records):
        meta = d[RAW_KEY]
        win.x0, win.y0, win.mask_h, win.mask_w = meta.get("window") or (0, 0, meta["h"], meta["w"])
    return windows


class _AugImage(ctypes.Structure):
    """Mirror of U2AugImage (include/u2seg_hip.h)."""

    _fields_ = ([(k, ctypes.c_int) for k in ("h", "w", "H", "W", "kx", "ky", "x_identity", "y_identity", "row0", "nrows",
                                             "num_masks", "first_mask")]
                + [(k, ctypes.c_longlong) for k in ("src_offset", "lab_offset", "img_out_offset", "lab_out_offset",
                                                    "mask_out_offset", "bx_bounds", "bx_coef", "by_bounds", "by_coef", "nx", "ny",
                                                    "mask_offs", "ends_base")])


_OUT_ALIGN = 256


def describe_batch(records, block_ptr):
    """Descriptors of a batch of raw records whose tensors are views of one block starting at address block_ptr (device or
    host: the layout is the same), and the sizes of the outputs: (descriptors, image bytes, label elements, mask bytes, masks)."""
    descs = (_AugImage * max(len(records), 1))()
    img_bytes = lab_elems = mask_bytes = masks = 0
    for a, d in zip(descs, records):
        meta, o = d[RAW_KEY], d[RAW_KEY]["offsets"]
        for k in ("h", "w", "H", "W", "kx", "ky", "row0", "nrows", "num_masks"):
            setattr(a, k, int(meta[k]))
        a.x_identity, a.y_identity, a.first_mask = int(meta["x_identity"]), int(meta["y_identity"]), masks
        a.src_offset = d["dm_image"].data_ptr() - block_ptr
        a.lab_offset = d["dm_sem_seg"].data_ptr() - block_ptr if "dm_sem_seg" in d else -1
        at = d["dm_tables"].data_ptr() - block_ptr
        assert at % 4 == 0 and at >= 0 and a.src_offset >= 0, "the tensors of a raw record are views of one aligned block"
        for k in _TABLE_ORDER + ("mask_offs",):
            setattr(a, k, at // 4 + int(o[k]))
        a.ends_base = at // 4
        a.img_out_offset, a.lab_out_offset, a.mask_out_offset = img_bytes, lab_elems, mask_bytes
        hw = a.H * a.W
        img_bytes += (3 * hw + _OUT_ALIGN - 1) // _OUT_ALIGN * _OUT_ALIGN
        lab_elems += hw if a.lab_offset >= 0 else 0
        mask_bytes += (a.num_masks * hw + _OUT_ALIGN - 1) // _OUT_ALIGN * _OUT_ALIGN
        masks += a.num_masks
    return descs, img_bytes, lab_elems, mask_bytes, masks


class PendingBatch:
    """A batch of raw records whose kernels have been launched: the tensors are there, the per-mask pixel counts are on their
    way to pinned memory.  `finish()` (after the event the launching stream recorded behind that copy) applies the by_mask
    filter and gives the list of mapped dicts."""

    def __init__(self, records, block, image, labels, masks, counts_host, descs, boxes=None):
        self.records, self.block, self.image, self.labels, self.masks = records, block, image, labels, masks
        self.counts_host, self.descs = counts_host, descs
        self.boxes = boxes  # int32 [masks, 4] on the device: the tight boxes (batches with a cropped record with masks), or None

    def outputs(self, i):
        """What the kernels wrote for record i, unfiltered: (image [3, H, W], label map [H, W] or None, masks [N, H, W], counts
        int32 [N] on the host - valid once the launching stream has passed the copy)."""
        a, hw = self.descs[i], self.descs[i].H * self.descs[i].W
        image = self.image[a.img_out_offset:a.img_out_offset + 3 * hw].view(3, a.H, a.W)
        labels = self.labels[a.lab_out_offset:a.lab_out_offset + hw].view(a.H, a.W) if a.lab_offset >= 0 else None
        masks = self.masks[a.mask_out_offset:a.mask_out_offset + a.num_masks * hw].view(a.num_masks, a.H, a.W)
        return image, labels, masks, self.counts_host[a.first_mask:a.first_mask + a.num_masks]

    def finish(self, stream=None):
        """stream: the stream that will consume the batch, when it is not the one the kernels were launched on.  The four
        allocations are marked as used by it BEFORE anything is read there: the by_mask filter gathers the surviving rows
        into new tensors on the consumer stream, and when it fires for every record that held a view of an allocation,
        nothing that is handed out keeps that allocation alive - unmarked, it would go back to the launching stream's pool
        and be overwritten by the next batch's kernels while the gather is still queued."""
        if stream is not None:
            for t in (self.block, self.image, self.labels, self.masks, self.boxes):
                if t is not None and t.is_cuda:
                    t.record_stream(stream)
        out = []
        for a, d in zip(self.descs, self.records):
            meta, hw = d[RAW_KEY], a.H * a.W
            rec = {k: v for k, v in d.items() if k != RAW_KEY and k not in TENSOR_KEYS}
            rec["image"] = self.image[a.img_out_offset:a.img_out_offset + 3 * hw].view(3, a.H, a.W)
            if a.lab_offset >= 0:
                rec["sem_seg"] = self.labels[a.lab_out_offset:a.lab_out_offset + hw].view(a.H, a.W)
            if meta["has_instances"]:
                masks = counts = tight = None
                if meta["has_masks"]:
                    masks = self.masks[a.mask_out_offset:a.mask_out_offset + a.num_masks * hw].view(a.num_masks, a.H, a.W)
                    counts = self.counts_host[a.first_mask:a.first_mask + a.num_masks].numpy()
                    if meta.get("recompute_boxes"):  # the boxes stay on the device: only the counts crossed
                        tight = self.boxes[a.first_mask:a.first_mask + a.num_masks].to(torch.float32)
                rec["instances"] = assemble_instances(meta, d["dm_boxes"], d["dm_classes"], masks, counts, tight)
            out.append(rec)
        return out


def launch_batch(records, block, host_block, counts_host=None):
    """Launches the three calls of csrc/augment.hip for a batch of raw records on torch's current stream and starts the copy of
    the per-mask counts into `counts_host` (pinned int32, at least as long as the batch has masks; allocated when None).
    records: the raw records with their tensors on the device, views of `block` (uint8, one allocation); host_block: the host
    copy the block was filled from (the launchers check the tables there before anything runs).  Returns a PendingBatch."""
    from .. import _hip

    if not block.is_cuda:
        raise RuntimeError("raw records of the DeviceMapper are finished by HIP kernels: they need a GPU (no host fallback)")
    dev, nbytes = block.device, block.numel()
    assert host_block.numel() >= nbytes and not host_block.is_cuda
    descs, img_bytes, lab_elems, mask_bytes, masks = describe_batch(records, block.data_ptr())
    n = len(records)
    image = torch.empty(max(img_bytes, 1), dtype=torch.uint8, device=dev)
    labels = torch.empty(max(lab_elems, 1), dtype=torch.int64, device=dev)
    mask_out = torch.empty(max(mask_bytes, 1), dtype=torch.bool, device=dev)
    counts = torch.empty(max(masks, 1), dtype=torch.int32, device=dev)
    need = int(_hip.call_nostream("u2_aug_resize_bilinear_scratch_bytes", descs, n))
    if need < 0:
        raise RuntimeError("u2_aug_resize_bilinear_scratch_bytes failed with status %d" % need)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    host_ptr = host_block.data_ptr()
    _hip.call("u2_aug_resize_bilinear_u8", block, nbytes, host_ptr, image, img_bytes, scratch, need, descs, n)
    if lab_elems:
        _hip.call("u2_aug_resize_nearest_u8", block, nbytes, host_ptr, labels, lab_elems, descs, n)
    windows, boxes = describe_windows(records), None
    if masks and windows is None:
        _hip.call("u2_aug_rle_masks", block, nbytes, host_ptr, mask_out, mask_bytes, counts, masks, descs, n)
    elif masks:  # a cropped record with masks: the windowed decode, and the tight boxes with it
        boxes = torch.empty((masks, 4), dtype=torch.int32, device=dev)
        _hip.call("u2_aug_rle_masks_boxes", block, nbytes, host_ptr, mask_out, mask_bytes, counts, boxes, masks, descs, windows, n)
    if counts_host is None or counts_host.numel() < masks:
        counts_host = torch.empty(max(masks, 1), dtype=torch.int32, pin_memory=True)
    if masks:
        counts_host[:masks].copy_(counts[:masks], non_blocking=True)
    return PendingBatch(records, block, image, labels, mask_out, counts_host, descs, boxes)


def make_raw_record(passthrough, image, labels, tables, ends, boxes=None, classes=(), has_masks=False, window=None,
                    recompute_boxes=False):
    """The raw record of one sample: `passthrough` plus the source image (HWC uint8) and label map (uint8 or None) as they
    were loaded, the tables of build_tables and the run ends of the box-kept masks in one int32 tensor, the box-kept boxes
    (fp32 [N, 4], None: a sample without annotations) and classes, and the sizes and offsets the device side needs.
    window = (x0, y0, mask_h, mask_w), a cropped sample: image and labels are the window's pixels, the tables those of the
    window, the run ends still those of the whole mask_h x mask_w annotation.  recompute_boxes: nothing was dropped by its box
    and `boxes` is replaced by the masks' tight boxes when the record is finished."""
    record = dict(passthrough)
    h, w = image.shape[:2]
    H, W = len(tables["ny"]), len(tables["nx"])
    flat, where = pack_tables(tables, ends)
    record["dm_image"] = torch.from_numpy(np.array(image, dtype=np.uint8, order="C"))  # a writable copy: PIL's buffer is not
    if labels is not None:
        assert labels.shape == (h, w) and labels.dtype == np.uint8, (labels.shape, labels.dtype)
        record["dm_sem_seg"] = torch.from_numpy(np.array(labels, dtype=np.uint8, order="C"))
    record["dm_tables"] = torch.from_numpy(flat)
    if boxes is not None:
        record["dm_boxes"] = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).reshape(-1, 4)
        record["dm_classes"] = torch.tensor([int(c) for c in classes], dtype=torch.int64)
    rows = np.concatenate([tables["by_bounds"][:, 0], tables["by_bounds"][:, 0] + tables["by_bounds"][:, 1]])
    record[RAW_KEY] = {"h": h, "w": w, "H": H, "W": W, "kx": int(tables["bx_coef"].shape[1]),
                       "ky": int(tables["by_coef"].shape[1]), "x_identity": bool(tables["x_identity"]),
                       "y_identity": bool(tables["y_identity"]), "row0": int(rows.min()),
                       "nrows": int(rows.max() - rows.min()), "num_masks": len(ends), "has_instances": boxes is not None,
                       "has_masks": bool(has_masks), "offsets": where}
    if window is not None:
        record[RAW_KEY]["window"] = tuple(int(v) for v in window)
    if recompute_boxes and has_masks:
        record[RAW_KEY]["recompute_boxes"] = True
    return record


# ---- the mapper -----------------------------------------------------------------------------------------------------------
_ACCEPTED_AUGMENTATIONS = (T.ResizeShortestEdge, T.RandomFlip, T.RandomCrop)
_ACCEPTED_TRANSFORMS = (T.ResizeTransform, T.HFlipTransform, T.VFlipTransform, T.NoOpTransform, T.CropTransform)


class DeviceMapper:
    """DeviceMapper(cfg, is_train=True): `DatasetMapper`'s constructor contract, for training.  Calling it on a dataset dict
    gives a raw record (see the module docstring); `DevicePrefetcher` finishes it on the GPU."""

    def __init__(self, cfg=None, is_train=True, *, augmentations=None, image_format=None, use_instance_mask=None,
                 instance_mask_format=None, recompute_boxes=None):
        if not is_train:
            raise NotImplementedError("DeviceMapper serves the training loader; the test-mode loader keeps DatasetMapper")
        if cfg is not None:
            unsupported = cfg.MODEL.KEYPOINT_ON or cfg.MODEL.LOAD_PROPOSALS
            assert not unsupported, "keypoint / precomputed-proposal inputs are not part of the U2Seg configs"
            augmentations, recompute_boxes = crop_from_config(cfg, is_train, augmentations, recompute_boxes)
            image_format = image_format or cfg.INPUT.FORMAT
            use_instance_mask = cfg.MODEL.MASK_ON if use_instance_mask is None else use_instance_mask
            instance_mask_format = instance_mask_format or cfg.INPUT.MASK_FORMAT
        self.is_train = True
        self.augmentations = list(augmentations)
        for i, a in enumerate(self.augmentations):
            if i > 0 and isinstance(a, (T.RandomCrop, T.CropTransform)):
                raise NotImplementedError("DeviceMapper cannot run %s at position %d of the augmentations (behind %s): the "
                                          "device path crops at position 0 only, in front of the resize and of any flip"
                                          % (type(a).__name__, i, type(self.augmentations[i - 1]).__name__))
            ok = isinstance(a, _ACCEPTED_TRANSFORMS) if isinstance(a, T.Transform) else isinstance(a, _ACCEPTED_AUGMENTATIONS)
            if not ok:
                raise NotImplementedError("DeviceMapper cannot run %s on the device: it takes ResizeShortestEdge / RandomFlip "
                                          "(ResizeTransform, HFlipTransform, VFlipTransform, NoOpTransform) behind an optional "
                                          "RandomCrop / CropTransform" % type(a).__name__)
            if isinstance(a, (T.ResizeShortestEdge, T.ResizeTransform)) and a.interp != T.Image.BILINEAR:
                raise NotImplementedError("DeviceMapper cannot run %s with interpolation %r on the device: bilinear only"
                                          % (type(a).__name__, a.interp))
        self.image_format = image_format
        self.use_instance_mask = bool(use_instance_mask)
        self.instance_mask_format = instance_mask_format or "polygon"
        self.recompute_boxes = bool(recompute_boxes)
        assert self.use_instance_mask or not self.recompute_boxes, "recompute_boxes requires instance masks"

    def _load(self, record):
        return DatasetMapper._load(self, record)  # the same files, exif handling and size check

    def _draw(self, shape):
        """The transforms of one sample, drawn exactly like AugmentationList does on pixels: every augmentation reads only the
        shape of the image its predecessors left (a stand-in array of that shape, never touched)."""
        h, w = shape
        tfms = []
        for a in self.augmentations:
            t = a if isinstance(a, T.Transform) else a.get_transform(np.broadcast_to(np.uint8(0), (h, w, 3)))
            if not isinstance(t, _ACCEPTED_TRANSFORMS):
                raise NotImplementedError("DeviceMapper cannot run %s on the device" % type(t).__name__)
            if isinstance(t, T.ResizeTransform):
                assert (t.h, t.w) == (h, w), ((t.h, t.w), (h, w))
                h, w = t.new_h, t.new_w
            elif isinstance(t, T.CropTransform):
                assert 0 <= t.x0 and 0 <= t.y0 and t.x0 + t.w <= w and t.y0 + t.h <= h and t.w > 0 and t.h > 0, (vars(t), (h, w))
                h, w = t.h, t.w
            tfms.append(t)
        return T.TransformList(tfms), (h, w)

    @staticmethod
    def _geometry(transforms, shape):
        """(H, W, hflip, vflip) of a chain of resizes and flips; a flip commutes with a resize of the same axis (both index
        tables are applied to the output order), so only the parity of the flips matters."""
        (h, w), hflip, vflip = shape, False, False
        for t in transforms:
            if isinstance(t, T.ResizeTransform):
                if hflip or vflip:
                    raise NotImplementedError("DeviceMapper: a ResizeTransform behind a flip")  # PIL's taps are not mirror-symmetric
                h, w = t.new_h, t.new_w
            elif isinstance(t, T.HFlipTransform):
                hflip = not hflip
            elif isinstance(t, T.VFlipTransform):
                vflip = not vflip
        return h, w, hflip, vflip

    def __call__(self, dataset_dict):
        record = copy.deepcopy(dataset_dict)
        image, labels = self._load(record)
        h, w = image.shape[:2]
        transforms, _ = self._draw((h, w))
        resizes = [t for t in transforms if isinstance(t, T.ResizeTransform)]
        if len(resizes) > 1:
            raise NotImplementedError("DeviceMapper: more than one ResizeTransform")
        window = None
        if len(transforms) and isinstance(transforms[0], T.CropTransform):  # position 0 (the constructor): the window goes up
            crop = transforms[0]
            window = (crop.x0, crop.y0, h, w)
            image = crop.apply_image(image)
            labels = None if labels is None else crop.apply_image(labels)
        sh, sw = image.shape[:2]
        H, W, hflip, vflip = self._geometry(transforms, (sh, sw))
        tables = build_tables(sh, sw, H, W, hflip, vflip)
        annotations = record.pop("annotations", None)
        ends, has_instances, has_masks = [], annotations is not None, False
        boxes, classes = np.zeros((0, 4), dtype=np.float32), []
        if has_instances:
            kept = []
            for anno in annotations:
                if anno.get("iscrowd", 0) != 0:
                    continue  # crowd regions do not train the detector
                anno.pop("keypoints", None)
                segm = anno.pop("segmentation", None)
                if not self.use_instance_mask:
                    segm = None
                anno = utils.transform_instance_annotations(anno, transforms, (H, W))  # box only: the segmentation is set aside
                anno["segmentation"] = segm
                kept.append(anno)
            has_masks = bool(kept) and kept[0]["segmentation"] is not None
            if has_masks and self.instance_mask_format != "bitmask":
                raise NotImplementedError("INPUT.MASK_FORMAT '%s': the U2Seg configs use 'bitmask'" % self.instance_mask_format)
            all_boxes = (np.stack([utils.BoxMode.convert(a["bbox"], a["bbox_mode"], utils.BoxMode.XYXY_ABS) for a in kept])
                         if kept else np.zeros((0, 4)))
            box_t = torch.as_tensor(all_boxes, dtype=torch.float32).reshape(-1, 4)
            keep = Boxes(box_t).nonempty(threshold=1e-5).numpy()  # the by_box half of filter_empty_instances
            if self.recompute_boxes and has_masks:
                keep[:] = True  # the boxes will be those of the masks: the device says which rows have one
            boxes = box_t.numpy()[keep]
            classes = [int(a["category_id"]) for a, k in zip(kept, keep) if k]
            if has_masks:
                for a, k in zip(kept, keep):
                    segm = a["segmentation"]
                    if not isinstance(segm, dict):
                        raise NotImplementedError("DeviceMapper decodes RLE segmentations on the device; a %s segmentation "
                                                  "(polygons / bitmaps in training) is not supported" % type(segm).__name__)
                    if [int(v) for v in segm["size"]] != [h, w]:
                        raise ValueError("RLE of size %s on an image of size %s" % (list(segm["size"]), [h, w]))
                    counts = rle.counts_of(segm)  # parsed and checked for every instance, decoded for none
                    e = run_ends(counts, h, w)
                    if k:
                        ends.append(e)
        return make_raw_record(record, image, labels, tables, ends, boxes if has_instances else None, classes, has_masks,
                               window, self.recompute_boxes)
