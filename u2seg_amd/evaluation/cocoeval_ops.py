"""The two heavy stages of COCO AP - greedy matching per (image, category) and the precision / recall curves per (category,
area range, detection budget, IoU threshold) - on the device (csrc/cocoeval.hip).

The definition is evaluation/cocoeval.py (`_match_image`, `accumulate`), which stays the default engine; this path returns
the same tables value for value: the IoU, recall and precision quotients are single IEEE operations on exact inputs, the
rest is integer work.

`pack` lays the groups of `cocoeval.prepare` out as flat arrays: *cells* (an (image, category) pair with at least one ground
truth or detection) in (category, image position) order, the detections of a cell in descending score order cut to the
largest budget, the ground truth of a cell in its original order, and per category the permutation that sorts its detections
over all images by descending score (stable: image position in params.imgIds, then rank).  `run` makes one upload (one
pinned staging buffer), launches, and fetches precision | scores | recall in one transfer; `counters` counts what happens.
With records=True the match records and IoU tables of every cell come back too (the tests compare them with the host's).

A request for this engine without a GPU is an error: there is no fallback."""
import ctypes

import numpy as np
import torch

from .. import _hip

counters = {"host_syncs": 0, "d2h_transfers": 0, "h2d_transfers": 0}
last_timing = {}  # of the last `run(..., timing=True)`: pack excluded; upload_ms, kernel_ms (device events), fetch_ms

_PTRS = ("cell_dt_off", "cell_gt_off", "cell_iou_off", "cell_cat", "dt_area", "dt_score", "dt_box", "dt_row", "dt_marea",
         "gt_area", "gt_box", "gt_crowd", "gt_col", "gt_marea", "inter", "perm", "cat_dt_off", "area_rng", "iou_thrs",
         "rec_thrs", "max_dets")
_WS_PARTS = ("iou", "flags", "sflags", "sscore", "gt_order", "gt_ignore", "n_valid", "taken", "cell_valid", "path")


class _Problem(ctypes.Structure):
    """Mirror of U2CocoEvalProblem (include/u2seg_hip.h)."""

    _fields_ = ([(n, ctypes.c_void_p) for n in _PTRS]
                + [(n, ctypes.c_longlong) for n in ("n_cells", "n_dt", "n_gt", "iou_entries")]
                + [(n, ctypes.c_int) for n in ("K", "A", "T", "R", "M", "mask_form", "max_rank", "pad_")])


MAX_LANES = 40  # (area range, IoU threshold) pairs one wave serves
MAX_AREAS = 8
MAX_REC = 256


def lds_iou_entries():
    """Largest D' * G of a cell whose IoU table the matching kernel keeps in LDS."""
    return int(_hip.call_nostream("u2_cocoeval_lds_iou_entries"))


def lds_max_gt():
    """Largest G of a cell whose taken-flags the matching kernel keeps in registers."""
    return int(_hip.call_nostream("u2_cocoeval_lds_max_gt"))


def scan_chunk():
    """Detections per chunk of the accumulation kernel's scans."""
    return int(_hip.call_nostream("u2_cocoeval_scan_chunk"))


def workspace_bytes(n_dt, n_gt, iou_entries, n_cells, K, A=4, T=10):
    return int(_hip.call_nostream("u2_cocoeval_workspace_bytes", int(n_dt), int(n_gt), int(iou_entries), int(n_cells), int(K),
                                  int(A), int(T)))


class Packed:
    """What `pack` returns: the flat arrays (attributes named as in U2CocoEvalProblem), the ids they stand for (img_ids,
    cat_ids, cell_img / cell_cat positions, dt_id, gt_id) and the sizes."""

    def cell_dets(self, c):
        return slice(int(self.cell_dt_off[c]), int(self.cell_dt_off[c + 1]))

    def cell_gts(self, c):
        return slice(int(self.cell_gt_off[c]), int(self.cell_gt_off[c + 1]))

    def cell_key(self, c):
        return self.img_ids[int(self.cell_img[c])], self.cat_ids[int(self.cell_cat[c])]


def _f64(values, n, width=None):
    a = np.array(values, dtype=np.float64)
    return a.reshape(n) if width is None else a.reshape(n, width)


def _runs(keys):
    """first index of the run every entry of the ascending `keys` belongs to"""
    n = keys.size
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    new = np.r_[True, keys[1:] != keys[:-1]]
    return np.flatnonzero(new)[np.cumsum(new) - 1]


def pack(gts, dts, params, pair_counts=None, rows=None):
    """gts, dts: the groups of `cocoeval.prepare`.  pair_counts (mask form): `cocoeval.host_pair_counts`' tables; rows: row
    of result k (detection id k + 1) in its image's table."""
    img_ids, cat_ids = list(params.imgIds), list(params.catIds)
    if len(set(img_ids)) != len(img_ids) or len(set(cat_ids)) != len(cat_ids):
        raise ValueError("image ids and category ids must be unique")
    NI, K = len(img_ids), len(cat_ids)
    A, T, R, M = len(params.areaRng), len(params.iouThrs), len(params.recThrs), len(params.maxDets)
    if K < 1 or A < 1 or T < 1 or M < 1 or R < 1:
        raise ValueError("no categories, area ranges, IoU thresholds, budgets or recall thresholds to evaluate")
    if A * T > MAX_LANES or A > MAX_AREAS or R > MAX_REC:
        raise ValueError("%d area ranges x %d IoU thresholds, %d recall thresholds: the device engine serves at most %d pairs, "
                         "%d ranges, %d recall thresholds" % (A, T, R, MAX_LANES, MAX_AREAS, MAX_REC))
    max_dets = [int(v) for v in params.maxDets]
    if any(v < 0 or v >= 2 ** 23 for v in max_dets):
        raise ValueError("detection budgets must lie in [0, 2^23), got %r" % (params.maxDets,))
    rec = np.asarray(params.recThrs, dtype=np.float64)
    if np.any(np.diff(rec) < 0):
        raise ValueError("recall thresholds must ascend")
    img_pos = {v: i for i, v in enumerate(img_ids)}
    cat_pos = {v: i for i, v in enumerate(cat_ids)}
    last = max_dets[-1]
    mask_form = pair_counts is not None
    if mask_form and rows is None:
        raise ValueError("the mask form needs the row of every result in its image's table")

    # detections: stable descending score inside a cell, the cut, cells in (category, image) order
    dkeys = [k for k in dts if dts[k]]
    flat = [d for k in dkeys for d in dts[k]]
    n = len(flat)
    d_cell = np.repeat(np.array([cat_pos[c] * NI + img_pos[i] for i, c in dkeys], dtype=np.int64).reshape(len(dkeys)),
                       np.array([len(dts[k]) for k in dkeys], dtype=np.int64).reshape(len(dkeys)))
    score = _f64([d["score"] for d in flat], n)
    if not np.isfinite(score).all():
        raise ValueError("detection scores must be finite")
    order = np.lexsort((-score, d_cell))
    rank = np.arange(n, dtype=np.int64) - _runs(d_cell[order])
    order = order[rank < last]
    rank = rank[rank < last]
    n_dt = int(order.size)
    d_cell, score = d_cell[order], score[order]
    dt_area = _f64([d["area"] for d in flat], n)[order]
    dt_id = np.array([d["id"] for d in flat], dtype=np.int64).reshape(n)[order]
    if not mask_form:
        try:
            dt_box = _f64([d["bbox"] for d in flat], n, 4)[order]
        except (TypeError, ValueError):
            raise ValueError("every detection needs a bbox of four numbers") from None
        if not np.isfinite(dt_box).all():
            raise ValueError("detection boxes must be finite")
    if not np.isfinite(dt_area).all():
        raise ValueError("detection areas must be finite")

    # ground truth: original order inside a cell
    gkeys = [k for k in gts if gts[k]]
    gflat = [g for k in gkeys for g in gts[k]]
    ng = len(gflat)
    g_cell = np.repeat(np.array([cat_pos[c] * NI + img_pos[i] for i, c in gkeys], dtype=np.int64).reshape(len(gkeys)),
                       np.array([len(gts[k]) for k in gkeys], dtype=np.int64).reshape(len(gkeys)))
    g_order = np.argsort(g_cell, kind="stable")
    g_cell = g_cell[g_order]
    gt_area = _f64([g["area"] for g in gflat], ng)[g_order]
    gt_crowd = np.array([bool(g["iscrowd"]) for g in gflat], dtype=np.uint8).reshape(ng)[g_order]
    gt_ignore = np.array([bool(g["ignore"]) for g in gflat], dtype=np.uint8).reshape(ng)[g_order]
    if not np.array_equal(gt_crowd, gt_ignore):
        raise ValueError('ground truth must be ignored exactly where it is a crowd region ("ignore" == "iscrowd")')
    gt_id = np.array([g["id"] for g in gflat], dtype=np.int64).reshape(ng)[g_order]
    if (gt_id == 0).any():
        raise ValueError("annotation id 0: a match with it counts as no match; use positive ids")
    if not np.isfinite(gt_area).all():
        raise ValueError("ground-truth areas must be finite")
    if not mask_form:
        try:
            gt_box = _f64([g["bbox"] for g in gflat], ng, 4)[g_order]
        except (TypeError, ValueError):
            raise ValueError("every annotation needs a bbox of four numbers") from None
        if not np.isfinite(gt_box).all():
            raise ValueError("ground-truth boxes must be finite")

    cells = np.unique(np.concatenate([d_cell, g_cell]))
    C = int(cells.size)
    p = Packed()
    p.img_ids, p.cat_ids, p.n_cells, p.n_dt, p.n_gt = img_ids, cat_ids, C, n_dt, ng
    p.K, p.A, p.T, p.R, p.M, p.mask_form = K, A, T, R, M, int(mask_form)
    p.cell_cat, p.cell_img = (cells // NI).astype(np.int32), (cells % NI).astype(np.int64)
    dt_cell, gt_cell = np.searchsorted(cells, d_cell), np.searchsorted(cells, g_cell)
    p.dt_cell, p.gt_cell = dt_cell, gt_cell
    D, G = np.bincount(dt_cell, minlength=C).astype(np.int64), np.bincount(gt_cell, minlength=C).astype(np.int64)
    p.cell_dt_off = np.r_[0, np.cumsum(D)].astype(np.int64)
    p.cell_gt_off = np.r_[0, np.cumsum(G)].astype(np.int64)
    p.cell_iou_off = np.r_[0, np.cumsum(D * G)].astype(np.int64)
    p.iou_entries = int(p.cell_iou_off[-1])
    p.max_rank = int(D.max()) if C else 0
    dt_cat = p.cell_cat[dt_cell].astype(np.int64)
    p.cat_dt_off = np.r_[0, np.cumsum(np.bincount(dt_cat, minlength=K))].astype(np.int64)
    p.perm = np.lexsort((-score, dt_cat)).astype(np.int32)
    p.dt_score, p.dt_area, p.dt_id, p.dt_rank = score, dt_area, dt_id, rank
    p.gt_area, p.gt_crowd, p.gt_id = gt_area, gt_crowd, gt_id
    p.area_rng = np.asarray(params.areaRng, dtype=np.float64).reshape(A, 2)
    p.iou_thrs = np.asarray(params.iouThrs, dtype=np.float64).reshape(T)
    p.rec_thrs, p.max_dets = rec.reshape(R), np.asarray(max_dets, dtype=np.int32)
    if not mask_form:
        p.dt_box, p.gt_box = np.ascontiguousarray(dt_box), np.ascontiguousarray(gt_box)
        return p

    # mask form: the images' tables end to end; a detection knows where its row starts, a ground truth its column
    tab_off, ncols = np.full(NI, -1, dtype=np.int64), np.zeros(NI, dtype=np.int64)
    a_off, g_off = np.zeros(NI, dtype=np.int64), np.zeros(NI, dtype=np.int64)
    nrows = np.zeros(NI, dtype=np.int64)
    inters, ads, ags, colmap = [], [], [], {}
    to = ao = go = 0
    for img, pc in pair_counts.items():
        i = img_pos.get(img)
        if i is None:
            continue
        ad = np.asarray(pc["area_dt"], dtype=np.int64).reshape(-1)
        ag = np.asarray(pc["area_gt"], dtype=np.int64).reshape(-1)
        if len(pc["gt_ids"]) != ag.size:
            raise ValueError("image %s: %d ground-truth ids for %d ground-truth areas" % (img, len(pc["gt_ids"]), ag.size))
        inters.append(np.asarray(pc["inter"], dtype=np.int64).reshape(ad.size, ag.size).reshape(-1))
        ads.append(ad)
        ags.append(ag)
        tab_off[i], ncols[i], nrows[i], a_off[i], g_off[i] = to, ag.size, ad.size, ao, go
        to, ao, go = to + ad.size * ag.size, ao + ad.size, go + ag.size
        for j, gid in enumerate(pc["gt_ids"]):
            colmap[img, gid] = j
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
    inter, area_dt, area_gt = cat(inters), cat(ads), cat(ags)
    dt_img, gt_img = p.cell_img[dt_cell], p.cell_img[gt_cell]
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    row = rows[dt_id - 1]
    have = tab_off[dt_img] >= 0
    if (have & ((row < 0) | (row >= nrows[dt_img]))).any():
        raise ValueError("a result's row lies outside its image's pair-count table")
    gt_col = np.array([colmap.get((img_ids[int(i)], int(g)), -1) for i, g in zip(gt_img, gt_id)], dtype=np.int64).reshape(ng)
    both = (D > 0) & (G > 0)
    if (both[dt_cell] & ~have).any():
        k = int(np.flatnonzero(both[dt_cell] & ~have)[0])
        raise KeyError("image %s has detections and ground truth but no pair counts" % (img_ids[int(dt_img[k])],))
    if (both[gt_cell] & (gt_col < 0)).any():
        k = int(np.flatnonzero(both[gt_cell] & (gt_col < 0))[0])
        raise KeyError("annotation %d of image %s is not in its image's pair counts" % (int(gt_id[k]), img_ids[int(gt_img[k])]))
    p.dt_row = np.where(have, tab_off[dt_img] + row * ncols[dt_img], 0).astype(np.int64)
    p.dt_marea = np.where(have, area_dt[np.where(have, a_off[dt_img] + row, 0)] if area_dt.size else 0, 0).astype(np.int64)
    ok = gt_col >= 0
    p.gt_col = np.where(ok, gt_col, 0).astype(np.int64)
    p.gt_marea = np.where(ok, area_gt[np.where(ok, g_off[gt_img] + gt_col, 0)] if area_gt.size else 0, 0).astype(np.int64)
    p.inter = inter
    return p


def unpack(packed):
    """The groups back, for checking `pack`: {(image, category): {"dt_ids": in score order, cut; "dt_scores"; "gt_ids"}} over
    the cells, and {category: detection ids of its list in accumulation order}."""
    cells = {}
    for c in range(packed.n_cells):
        d, g = packed.cell_dets(c), packed.cell_gts(c)
        cells[packed.cell_key(c)] = {"dt_ids": packed.dt_id[d].tolist(), "dt_scores": packed.dt_score[d].tolist(),
                                     "gt_ids": packed.gt_id[g].tolist()}
    lists = {}
    for k, cat in enumerate(packed.cat_ids):
        lists[cat] = packed.dt_id[packed.perm[int(packed.cat_dt_off[k]): int(packed.cat_dt_off[k + 1])]].tolist()
    return cells, lists


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError('the "device" engine of COCO AP needs a GPU: there is no fallback to the host engine; ask for '
                           '"host" on a machine without one')


def _align16(n):
    return (int(n) + 15) // 16 * 16


def run(packed, device=None, records=False, timing=False, ious=False):
    """{"precision", "scores" [T, R, K, A, M], "recall" [T, K, A, M], "counts"} as `cocoeval.accumulate` returns them.
    records=True adds "records": rec_match int32 / rec_ignore uint8 [n_dt, A * T], the workspace parts "iou" (float64,
    cell after cell [D', G]), "gt_order" int32 and "gt_ignore" uint8 ([A, G] per cell), "cell_valid" int32 [C, A],
    "path" uint8 [C] (0: LDS, 1: global memory).  ious=True (without records): "records" holds "iou" alone, one more transfer."""
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    p = packed
    names = [n for n in _PTRS if getattr(p, n, None) is not None]
    arrays = [np.ascontiguousarray(getattr(p, n)) for n in names]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += _align16(a.nbytes)
    t_up = torch.cuda.Event(enable_timing=True) if timing else None
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3)) if timing else (None, None, None)
    with torch.cuda.device(dev):
        if timing:
            t_up.record()
        host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for a, o in zip(arrays, offs):
            view[o: o + a.nbytes] = a.reshape(-1).view(np.uint8)
        counters["h2d_transfers"] += 1
        stage = host.to(dev, non_blocking=True)
        prob = _Problem()
        base = stage.data_ptr()
        for n, a, o in zip(names, arrays, offs):
            setattr(prob, n, base + o)
        prob.n_cells, prob.n_dt, prob.n_gt, prob.iou_entries = p.n_cells, p.n_dt, p.n_gt, p.iou_entries
        prob.K, prob.A, prob.T, prob.R, prob.M, prob.mask_form, prob.max_rank = p.K, p.A, p.T, p.R, p.M, p.mask_form, p.max_rank
        layout = (ctypes.c_longlong * 10)()
        ws_bytes = int(_hip.call_nostream("u2_cocoeval_workspace_layout", p.n_dt, p.n_gt, p.iou_entries, p.n_cells, p.K, p.A,
                                          p.T, ctypes.addressof(layout)))
        if ws_bytes < 0:
            raise RuntimeError("u2_cocoeval_workspace_layout refused the sizes")
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        AT = p.A * p.T
        rec_match = torch.zeros(max(p.n_dt * AT, 1), dtype=torch.int32, device=dev) if records else None
        rec_ignore = torch.zeros(max(p.n_dt * AT, 1), dtype=torch.uint8, device=dev) if records else None
        n_rec, n_prec = p.T * p.K * p.A * p.M, p.T * p.R * p.K * p.A * p.M
        out = torch.empty(2 * n_prec + n_rec, dtype=torch.float64, device=dev)
        if timing:
            e0.record()
        _hip.call("u2_cocoeval_match", ctypes.addressof(prob), ws, ws_bytes, rec_match, rec_ignore)
        _hip.call("u2_cocoeval_accumulate", ctypes.addressof(prob), ws, ws_bytes, out, out[n_prec:], out[2 * n_prec:])
        if timing:
            e1.record()
        counters["host_syncs"] += 1
        counters["d2h_transfers"] += 1
        res = out.cpu().numpy()
        if timing:
            e2.record()
            e2.synchronize()
            last_timing.update(upload_ms=t_up.elapsed_time(e0), kernel_ms=e0.elapsed_time(e1), fetch_ms=e1.elapsed_time(e2),
                               workspace_bytes=ws_bytes, upload_bytes=total)
        del host
        shape = (p.T, p.R, p.K, p.A, p.M)
        acc = {"precision": res[:n_prec].reshape(shape).copy(), "scores": res[n_prec: 2 * n_prec].reshape(shape).copy(),
               "recall": res[2 * n_prec:].reshape(p.T, p.K, p.A, p.M).copy(), "counts": [p.T, p.R, p.K, p.A, p.M]}
        if records:
            w = ws.cpu().numpy()
            o = dict(zip(_WS_PARTS, (int(v) for v in layout)))
            acc["records"] = {
                "rec_match": rec_match.cpu().numpy()[: p.n_dt * AT].reshape(p.n_dt, AT),
                "rec_ignore": rec_ignore.cpu().numpy()[: p.n_dt * AT].reshape(p.n_dt, AT),
                "iou": w[o["iou"]: o["iou"] + 8 * p.iou_entries].view(np.float64).copy(),
                "gt_order": w[o["gt_order"]: o["gt_order"] + 4 * p.A * p.n_gt].view(np.int32).copy(),
                "gt_ignore": w[o["gt_ignore"]: o["gt_ignore"] + p.A * p.n_gt].copy(),
                "cell_valid": w[o["cell_valid"]: o["cell_valid"] + 4 * p.A * p.n_cells].view(np.int32).reshape(p.n_cells, p.A).copy(),
                "path": w[o["path"]: o["path"] + p.n_cells].copy()}
        elif ious:
            o = int(layout[0])
            counters["d2h_transfers"] += 1
            acc["records"] = {"iou": ws[o: o + 8 * p.iou_entries].cpu().numpy().view(np.float64)}
    return acc


def cell_ious(packed, records, c):
    """[D', G] float64 IoU table of cell c."""
    d, g = packed.cell_dets(c), packed.cell_gts(c)
    o = int(packed.cell_iou_off[c])
    D, G = d.stop - d.start, g.stop - g.start
    return records["iou"][o: o + D * G].reshape(D, G)


def cell_record(packed, records, c, a):
    """The match record of cell c for area range a in `cocoeval._match_image`'s form: (matched annotation id or 0 [T, D'],
    detection ignored [T, D'] bool, scores [D'], ground truth ignored [G] bool in the order used)."""
    d, g = packed.cell_dets(c), packed.cell_gts(c)
    T, G = packed.T, g.stop - g.start
    col = records["rec_match"][d, a * T: (a + 1) * T].T.astype(np.int64)
    ids = np.concatenate([np.zeros(1, dtype=np.int64), packed.gt_id[g]])
    ign = records["gt_ignore"][packed.A * g.start + a * G: packed.A * g.start + (a + 1) * G].astype(bool)
    return ids[col], records["rec_ignore"][d, a * T: (a + 1) * T].T.astype(bool), packed.dt_score[d].copy(), ign


def evaluate(gts, dts, params, pair_counts=None, rows=None, records=False, timing=False, ious=False):
    """pack + run.  The returned dict also carries "packed"."""
    require_gpu()
    packed = pack(gts, dts, params, pair_counts, rows)
    acc = run(packed, records=records, timing=timing, ious=ious)
    acc["packed"] = packed
    return acc
