"""Launch wrappers with no autograd node and no state: level assignment, mask crops, IoU matching, the semantic upsample of
inference, row-wise top-k, box decoding and NMS."""
import ctypes
import math

import torch

from .. import _hip
from .weights import BF16, _check_act, zeros_f32


def assign_levels(boxes, min_level, max_level, canonical_size=224, canonical_level=4):
    n = boxes.shape[0]
    lv = torch.empty(n, dtype=torch.int32, device=boxes.device)
    _hip.call("u2_assign_levels", boxes.contiguous(), lv, n, min_level, max_level, float(canonical_size), canonical_level)
    return lv


def mask_crop(masks_u8, rois, size):
    """BitMasks.crop_and_resize (structures/masks.py:191-218): masks [Nm,H,W] uint8, rois [R,5]."""
    r = rois.shape[0]
    out = torch.empty((r, size, size), dtype=torch.uint8, device=rois.device)
    _hip.call("u2_mask_crop", masks_u8.contiguous(), rois.contiguous(), out, r, masks_u8.shape[1], masks_u8.shape[2], size)
    return out


def iou_match(boxes, gt, ngt, lo, hi, allow_low_quality):
    """boxes [n,4] (shared) or [B,n,4]; gt [B,G,4]; ngt [B] int32 -> match [B,n] int32, labels [B,n] int8."""
    per_image = boxes.dim() == 3
    b, g = gt.shape[0], gt.shape[1]
    n = boxes.shape[-2]
    dev = gt.device
    match = torch.empty((b, n), dtype=torch.int32, device=dev)
    mval = torch.empty((b, n), dtype=torch.float32, device=dev)
    labels = torch.empty((b, n), dtype=torch.int8, device=dev)
    gmax = torch.empty((b, g), dtype=torch.int32, device=dev) if allow_low_quality else None
    _hip.call("u2_iou_match", boxes.contiguous(), int(per_image), gt.contiguous(), ngt.contiguous(), match, mval, gmax,
              labels, b, n, g, float(lo), float(hi), int(allow_low_quality))
    return match, labels, mval


def sem_seg_upsample(x, num_classes, scale):
    """x [B, H, W, Cp] bf16 -> (fp32 [B, num_classes, H*scale, W*scale] bilinear-upsampled logits, int64 [B, H*scale, W*scale]
    argmax) (u2_semseg_upsample; inference only)."""
    _check_act(x)
    b, h, w, cp = x.shape
    out = torch.empty((b, num_classes, h * scale, w * scale), dtype=torch.float32, device=x.device)
    amax = torch.empty((b, h * scale, w * scale), dtype=torch.int64, device=x.device)
    _hip.call("u2_semseg_upsample", x, out, amax, b, h, w, cp, num_classes, int(scale))
    return out, amax


class _TopkSeg(ctypes.Structure):
    """U2TopkSeg of include/u2seg_hip.h."""
    _fields_ = ([(f, ctypes.c_void_p) for f in ("vals", "mask", "idx_in", "cnt_in", "out_vals", "out_idx", "out_cnt")]
                + [("row_stride", ctypes.c_longlong)]
                + [(f, ctypes.c_int) for f in ("dtype", "rows", "n", "group", "pitch", "mask_value", "k", "largest", "cnt_group",
                                               "idx_mod", "idx_mul", "reserved")])


def _ptr(t):
    return None if t is None else t.data_ptr()


_TOPK_MAX_K = 16384  # u2_topk_rows keeps the k survivors of a row in LDS (8 bytes each)


def topk_rows(vals, k, largest=True, mask=None, mask_value=1, group=1, pitch=1, n=None, want_vals=True):
    """Row-wise selection with a total order (u2_topk_rows): the k best of every row ranked by (value descending if
    `largest` else ascending, index ascending).  vals: [rows, n] fp32 / bf16 contiguous, or - with group / pitch / n - the
    `group` valid columns of a [rows, n // group, pitch]-shaped map (element i at (i // group) * pitch + i % group).
    mask (int8 [rows, n]): only elements equal to mask_value take part.
    Returns (values fp32 [rows, k] or None, indices int32 [rows, k], counts int32 [rows])."""
    return topk_rows_multi([dict(vals=vals, k=k, largest=largest, mask=mask, mask_value=mask_value, group=group, pitch=pitch, n=n,
                                 want_vals=want_vals)])[0]


def topk_rows_multi(specs):
    """Several independent selections (each a dict of topk_rows' arguments) in two launches of u2_topk_rows_multi instead of
    one or two per selection: the per-level pre-NMS top-k of all feature levels, or the two draws of a sampler over the same keys.
    A row is streamed by ONE work-group (five to seven dependent sweeps): long rows are cut into equal segments that are ranked
    as rows of their own in the first launch (reporting positions in the full row), and the survivors (k per segment, the real
    ones counted) are ranked again in the second.  Returns a list of (values or None, indices, counts)."""
    first, second, results = [], [], [None] * len(specs)
    keep = []  # the intermediate tensors are referenced by raw pointers only: they must outlive the launches below
    for j, sp in enumerate(specs):
        vals, k, largest = sp["vals"], int(sp["k"]), int(bool(sp.get("largest", True)))
        if k > _TOPK_MAX_K:
            # beyond the kernel's LDS-resident survivor list (e.g. PRE_NMS_TOPK = 12000 summed over the levels): a stable
            # device sort gives the same total order
            results[j] = _topk_rows_sorted(sp)
            continue
        mask, mask_value = sp.get("mask"), int(sp.get("mask_value", 1))
        group, pitch, n, want_vals = int(sp.get("group", 1)), int(sp.get("pitch", 1)), sp.get("n"), sp.get("want_vals", True)
        assert vals.is_cuda and vals.dtype in (torch.float32, BF16) and vals.is_contiguous()
        dev, rows = vals.device, vals.shape[0]
        if n is None:
            assert vals.dim() == 2
            n = vals.shape[1]
        row_stride = vals[0].numel()
        if mask is not None:
            assert mask.dtype == torch.int8 and mask.is_contiguous() and tuple(mask.shape) == (rows, n)
        idx = torch.empty((rows, k), dtype=torch.int32, device=dev)
        out = torch.empty((rows, k), dtype=torch.float32, device=dev) if want_vals else None
        cnt = torch.empty((rows,), dtype=torch.int32, device=dev)
        results[j] = (out, idx, cnt)
        dtype = 1 if vals.dtype == BF16 else 0
        segs = _topk_segments(rows, n, group, pitch, row_stride, k)
        if segs > 1:
            seg_n = n // segs
            k1 = min(k, seg_n)
            v1 = torch.empty((rows * segs, k1), dtype=torch.float32, device=dev)
            i1 = torch.empty((rows * segs, k1), dtype=torch.int32, device=dev)
            c1 = torch.empty((rows * segs,), dtype=torch.int32, device=dev)
            keep.append((v1, i1, c1))
            first.append(_TopkSeg(_ptr(vals), _ptr(mask), None, None, _ptr(v1), _ptr(i1), _ptr(c1), row_stride // segs, dtype,
                                  rows * segs, seg_n, group, pitch, mask_value, k1, largest, 1, segs, seg_n, 0))
            # dtype 2: fp32 storage of bf16 values (the survivors of a bf16 map) - two digit sweeps instead of four
            second.append(_TopkSeg(_ptr(v1), None, _ptr(i1), _ptr(c1), _ptr(out), _ptr(idx), _ptr(cnt), segs * k1, 2 * dtype, rows,
                                   segs * k1, 1, 1, 0, k, largest, k1, 1, 0, 0))
        else:
            first.append(_TopkSeg(_ptr(vals), _ptr(mask), None, None, _ptr(out), _ptr(idx), _ptr(cnt), row_stride, dtype, rows, n,
                                  group, pitch, mask_value, k, largest, 1, 1, 0, 0))
    for batch in (first, second):
        batch.sort(key=lambda g: -g.n)  # the longest rows start first
        for at in range(0, len(batch), 8):
            part = batch[at:at + 8]
            _hip.call("u2_topk_rows_multi", (_TopkSeg * len(part))(*part), len(part))
    del keep
    return results


def _topk_rows_sorted(sp):
    """topk_rows for k beyond the kernel's limit: torch's stable sort on the device under the same total order (value descending /
    ascending, index ascending; -0.0 equal to +0.0, every NaN the greatest value), same outputs (zeros as +0.0, NaNs as the quiet
    NaN; padding: index 0, value -/+ inf)."""
    vals, k, largest = sp["vals"], int(sp["k"]), bool(sp.get("largest", True))
    mask, mask_value = sp.get("mask"), int(sp.get("mask_value", 1))
    group, pitch, n = int(sp.get("group", 1)), int(sp.get("pitch", 1)), sp.get("n")
    rows = vals.shape[0]
    if n is None:
        n = vals.shape[1]
    v = vals.reshape(rows, -1)
    if group != 1 or pitch != 1:
        v = v.reshape(rows, -1, pitch)[:, : n // group, :group].reshape(rows, n)
    v = v[:, :n].float()
    # the kernel's canonical values, so that no sort backend can order them by bit pattern: -0.0 -> +0.0, any NaN -> quiet NaN
    v = torch.where(v != v, torch.full_like(v, float("nan")), v + 0.0)
    fill = float("-inf") if largest else float("inf")
    part = torch.ones_like(v, dtype=torch.bool) if mask is None else (mask == mask_value)
    order = torch.sort(torch.where(part, v, torch.full_like(v, fill)), dim=1, descending=largest, stable=True)[1]
    # elements that do not take part may tie with real -inf / +inf values: rank them last explicitly
    order = torch.gather(order, 1, torch.sort((~torch.gather(part, 1, order)).to(torch.int8), dim=1, stable=True)[1])[:, :k]
    cnt = part.sum(dim=1).clamp(max=k).to(torch.int32)
    real = torch.arange(order.shape[1], device=v.device)[None] < cnt[:, None]
    idx = torch.where(real, order, torch.zeros_like(order)).to(torch.int32)
    out = None
    if sp.get("want_vals", True):
        out = torch.where(real, torch.gather(v, 1, order), torch.full_like(v[:, : order.shape[1]], fill))
    if idx.shape[1] < k:  # k larger than the row
        pad = k - idx.shape[1]
        idx = torch.nn.functional.pad(idx, (0, pad))
        out = torch.nn.functional.pad(out, (0, pad), value=fill) if out is not None else None
    return out, idx, cnt


def _topk_segments(rows, n, group, pitch, row_stride, k):
    """How many equal segments to cut the rows of a selection into (1 = none): only long rows that few work-groups would
    stream, a divisor of the group count (segments must tile the row exactly), segments still several times longer than k.
    The first launch streams n / s elements per work-group, the merging second one s * k (at about twice the cost per element:
    fp32 keys, carried indices): s is the admissible divisor nearest to sqrt(n / 2k)."""
    if n < 32768 or rows >= 128 or n % group or row_stride != (n // group) * pitch:
        return 1
    groups = n // group
    target = math.sqrt(n / (2.0 * k))
    best, best_d = 1, None
    for s in range(2, 33):
        if groups % s == 0 and n // s >= max(4096, 2 * k) and rows * s <= 256:
            d = abs(math.log(s / target))
            if best_d is None or d < best_d:
                best, best_d = s, d
    return best


def apply_deltas(src, deltas, weights, img_idx=None, sizes=None, clamp=math.log(1000.0 / 16)):
    n = src.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=src.device)
    do_clip = sizes is not None
    _hip.call("u2_apply_deltas", src.contiguous(), deltas.contiguous(), img_idx, sizes, out, n, weights[0], weights[1],
              weights[2], weights[3], float(clamp), int(do_clip))
    return out


def apply_deltas_cls(src, deltas, num_classes, weights, clamp=math.log(1000.0 / 16)):
    """Class-specific decode: deltas [R, LP] (bf16 or fp32, 4 * num_classes valid columns, read where they lie) against
    src fp32 [R, 4] -> fp32 [R, 4 * num_classes]; no R x K x 4 copy of the source boxes is formed (u2_apply_deltas_cls)."""
    r, lp = deltas.shape
    assert deltas.dtype in (torch.bfloat16, torch.float32) and src.shape == (r, 4) and src.dtype == torch.float32
    out = torch.empty((r, 4 * num_classes), dtype=torch.float32, device=src.device)
    _hip.call("u2_apply_deltas_cls", src.contiguous(), deltas.contiguous(), int(deltas.dtype == torch.bfloat16), out, r,
              num_classes, lp, weights[0], weights[1], weights[2], weights[3], float(clamp))
    return out


class _RpnLevel(ctypes.Structure):
    """U2RpnLevel of include/u2seg_hip.h."""
    _fields_ = ([(f, ctypes.c_void_p) for f in ("deltas", "anchors", "idx", "scores")]
                + [(f, ctypes.c_int) for f in ("hwa", "k", "pitch", "reserved")])


def rpn_decode(levels, num_anchors, batch, kmax, sizes, weights, clamp, min_size):
    """Decoded, clipped and filtered RPN candidates of all levels in one launch (u2_rpn_decode).  levels: list of dicts with
    deltas (NHWC bf16 view whose channel 0 is the first delta), anchors [hwa, 4] fp32, idx [B, k] int32, scores [B, k] fp32.
    Returns boxes [B * L, kmax, 4], scores [B * L, kmax] (row = image * L + level), keep int8 [B * L, kmax], nonfinite int32 [1]."""
    dev = sizes.device
    rows = batch * len(levels)
    boxes = torch.empty((rows, kmax, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((rows, kmax), dtype=torch.float32, device=dev)
    keep = torch.empty((rows, kmax), dtype=torch.int8, device=dev)
    nonfinite = zeros_f32((1,), dev).view(torch.int32)
    segs = []
    for lv in levels:
        d, anc, idx, sc = lv["deltas"], lv["anchors"], lv["idx"], lv["scores"]
        assert d.dtype == BF16 and d.dim() == 4 and d.stride(3) == 1 and d.stride(2) == d.stride(1) // d.shape[2]
        assert anc.dtype == torch.float32 and anc.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous()
        assert sc.dtype == torch.float32 and sc.is_contiguous() and tuple(idx.shape) == tuple(sc.shape) == (batch, idx.shape[1])
        hwa = d.shape[1] * d.shape[2] * num_anchors
        assert anc.shape[0] == hwa and d.stride(0) == d.shape[1] * d.shape[2] * d.stride(2)
        segs.append(_RpnLevel(d.data_ptr(), anc.data_ptr(), idx.data_ptr(), sc.data_ptr(), hwa, idx.shape[1], d.stride(2), 0))
    _hip.call("u2_rpn_decode", (_RpnLevel * len(segs))(*segs), len(segs), num_anchors, batch, kmax, sizes, float(weights[0]),
              float(weights[1]), float(weights[2]), float(weights[3]), float(clamp), float(min_size), boxes, scores, keep, nonfinite)
    return boxes, scores, keep, nonfinite


def batched_nms(boxes, group, counts, thr, max_keep):
    """boxes [B,n,4] sorted by descending score, group [B,n] int32, counts [B] int32 ->
    keep [B,max_keep] int32 (positions in the sorted order), nkeep [B] int32."""
    b, n = boxes.shape[0], boxes.shape[1]
    ws_bytes = _hip.call_nostream("u2_nms_workspace_bytes", b, n)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=boxes.device)
    keep = torch.zeros((b, max_keep), dtype=torch.int32, device=boxes.device)
    nkeep = torch.zeros(b, dtype=torch.int32, device=boxes.device)
    _hip.call("u2_batched_nms", boxes.contiguous(), group.contiguous(), counts.contiguous(), ws, keep, nkeep, b, n,
              float(thr), max_keep)
    return keep, nkeep
