"""The one thing panoptic quality takes from the pixels of an image: how many pixels every (ground-truth segment, predicted
segment) pair shares.  counts int32 [G + 2, P]: row 0 = ground-truth void (id 0), rows 1..G = the ids of the ground truth's
segments_info in ascending order (`gt_table`), row G + 1 = every other id of the ground-truth png (pq.py skips those: they
are neither void nor a segment); column p = predicted id p, P = largest id of the prediction's segments_info + 1.

Two paths with identical results.  Host: `host_pair_counts`, searchsorted + bincount in numpy, which is the definition.
Device (csrc/panopticeval.hip, taken when the id maps live on a GPU): `pair_counts_batch` reads the id map where
u2_panoptic_merge wrote it, forms the ground-truth ids from the png's colour bytes there, and brings back the tables of the
whole batch.  One call costs one host-to-device copy (ground truth + id tables, from one pinned staging buffer), one host
synchronisation and one device-to-host transfer whatever the number of images; `counters` counts them where they happen.

evaluation/pq.py:accumulate_counts computes PQ from such a table."""
import ctypes

import numpy as np
import torch

from .. import _hip

counters = {"host_syncs": 0, "d2h_transfers": 0, "h2d_transfers": 0}


class _PairImage(ctypes.Structure):
    """Mirror of U2PanopticPairImage (include/u2seg_hip.h)."""

    _fields_ = [("pred", ctypes.c_void_p), ("gt", ctypes.c_void_p), ("gt_table", ctypes.c_void_p), ("counts", ctypes.c_void_p),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("G", ctypes.c_int), ("P", ctypes.c_int),
                ("gt_is_ids", ctypes.c_int), ("pad_", ctypes.c_int)]


def lds_table_ints():
    """Largest (G + 2) * P the kernel accumulates in LDS; a larger table is accumulated in global memory."""
    return int(_hip.call_nostream("u2_panoptic_pair_lds_ints"))


def _out_of_range(name, value=None):
    what = "segment id %d" % value if value is not None else "a segment id"
    return KeyError("%s: %s is in the predicted png but not in segments_info" % (name, what))


def _checked_gt(gt, shape, name):
    """The ground truth as a contiguous array: [H, W, 3] uint8 (the png's pixels) or [H, W] int32 (ids)."""
    gt = gt.numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
    if not ((gt.ndim == 3 and gt.shape[2] == 3 and gt.dtype == np.uint8) or (gt.ndim == 2 and gt.dtype == np.int32)):
        raise ValueError("%s: ground truth of shape %s and type %s; expected the png's [H, W, 3] uint8 pixels or an [H, W] int32 "
                         "id map" % (name, tuple(gt.shape), gt.dtype))
    if tuple(gt.shape[:2]) != tuple(shape):
        raise ValueError("%s: ground truth of size %s, prediction of size %s" % (name, tuple(gt.shape[:2]), tuple(shape)))
    return np.ascontiguousarray(gt)


def _checked_table(table, name):
    t = np.asarray(table, dtype=np.int64).reshape(-1)
    if t.size and (np.any(np.diff(t) <= 0) or t[0] < -2 ** 31 or t[-1] >= 2 ** 31):
        raise ValueError("%s: the ground-truth id table must be strictly ascending int32 ids" % name)
    return t


def host_pair_counts(pred_map, gt_ids, gt_table, num_pred_cols, name="image"):
    """The table in numpy.  gt_ids: [H, W] integer ids, or the png's [H, W, 3] uint8 pixels."""
    pred = (pred_map.cpu().numpy() if isinstance(pred_map, torch.Tensor) else np.asarray(pred_map)).astype(np.int64)
    gt = gt_ids.numpy() if isinstance(gt_ids, torch.Tensor) else np.asarray(gt_ids)
    if gt.ndim == 3:
        if gt.shape[2] != 3 or gt.dtype != np.uint8:
            raise ValueError("%s: ground truth of shape %s and type %s; expected the png's [H, W, 3] uint8 pixels or an "
                             "[H, W] id map" % (name, tuple(gt.shape), gt.dtype))
        g = gt.astype(np.int64)
        gt = g[..., 0] + 256 * g[..., 1] + 65536 * g[..., 2]  # data/pseudo_panoptic.py:rgb2id
    elif gt.ndim != 2 or gt.dtype.kind not in "iu":
        raise ValueError("%s: ground truth of shape %s and type %s; expected the png's [H, W, 3] uint8 pixels or an [H, W] id "
                         "map" % (name, tuple(gt.shape), gt.dtype))
    if gt.shape != pred.shape:
        raise ValueError("%s: ground truth of size %s, prediction of size %s" % (name, tuple(gt.shape), tuple(pred.shape)))
    gt = gt.astype(np.int64).reshape(-1)
    pred = pred.reshape(-1)
    table = _checked_table(gt_table, name)
    G, P = int(table.size), int(num_pred_cols)
    assert P >= 1, P
    bad = (pred < 0) | (pred >= P)
    if bad.any():
        raise _out_of_range(name, int(pred[bad][0]))
    if G:
        at = np.minimum(np.searchsorted(table, gt), G - 1)
        row = np.where(table[at] == gt, at + 1, G + 1)
    else:
        row = np.full(gt.shape, 1, dtype=np.int64)
    row = np.where(gt == 0, 0, row)
    return np.bincount(row * P + pred, minlength=(G + 2) * P).reshape(G + 2, P).astype(np.int32)


def _align16(n):
    return (int(n) + 15) // 16 * 16


class _Prepared:
    """A batch laid out for the launcher: descriptors + the tensors they point into."""

    def __init__(self, pred_maps, gts, gt_tables, num_pred_cols, names=None):
        n = len(pred_maps)
        assert len(gts) == n and len(gt_tables) == n and len(num_pred_cols) == n, "one entry per image"
        names = list(names) if names is not None else ["image %d of the batch" % i for i in range(n)]
        self.dev = dev = pred_maps[0].device
        self.names, self.preds, self.shapes, stage_parts = names, [], [], []
        stage_bytes = out_ints = 0
        for i in range(n):
            p = pred_maps[i]
            assert p.is_cuda and p.device == dev and p.dim() == 2, (p.shape, p.device)
            p = p.to(torch.int32).contiguous()
            self.preds.append(p if p.data_ptr() % 16 == 0 else p.clone())
            gt = _checked_gt(gts[i], p.shape, names[i])
            table = _checked_table(gt_tables[i], names[i]).astype(np.int32)
            P = int(num_pred_cols[i])
            assert P >= 1, P
            gt_off = stage_bytes
            tab_off = gt_off + _align16(gt.nbytes)
            stage_bytes = tab_off + _align16(table.nbytes)
            stage_parts.append((gt, gt_off, table, tab_off))
            self.shapes.append((int(table.size) + 2, P, out_ints))
            out_ints += (int(table.size) + 2) * P
        self.n, self.stage_parts, self.stage_bytes, self.out_ints = n, stage_parts, stage_bytes, out_ints

    def upload(self):
        """Ground truth and id tables of the batch: one pinned staging buffer, one copy."""
        host = torch.empty(max(self.stage_bytes, 16), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for gt, gt_off, table, tab_off in self.stage_parts:
            view[gt_off : gt_off + gt.nbytes] = gt.reshape(-1).view(np.uint8)
            view[tab_off : tab_off + table.nbytes] = table.view(np.uint8)
        counters["h2d_transfers"] += 1
        self.host_stage = host  # alive until the fetch has synchronised
        self.stage = host.to(self.dev, non_blocking=True)
        # [out-of-range counters of the n images | the tables]; the launcher clears it
        self.out = torch.empty(self.n + self.out_ints, dtype=torch.int32, device=self.dev)
        self.descs = (_PairImage * max(self.n, 1))()
        base, obase = self.stage.data_ptr(), self.out.data_ptr() + 4 * self.n
        for i, (gt, gt_off, table, tab_off) in enumerate(self.stage_parts):
            d, (rows, P, ooff) = self.descs[i], self.shapes[i]
            d.pred, d.gt, d.gt_table, d.counts = self.preds[i].data_ptr(), base + gt_off, base + tab_off, obase + 4 * ooff
            d.H, d.W, d.G, d.P, d.gt_is_ids = int(gt.shape[0]), int(gt.shape[1]), rows - 2, P, int(gt.ndim == 2)

    def launch(self):
        _hip.call("u2_panoptic_pair_counts", self.descs, self.n, self.out)

    def fetch(self):
        counters["host_syncs"] += 1
        counters["d2h_transfers"] += 1
        host = self.out.cpu().numpy()
        bad = np.flatnonzero(host[: self.n])
        if bad.size:
            raise _out_of_range(self.names[int(bad[0])])
        return [host[self.n + o : self.n + o + rows * P].reshape(rows, P).copy() for rows, P, o in self.shapes]


def pair_counts_batch(pred_maps, gts, gt_tables, num_pred_cols, names=None):
    """pred_maps: per image the [H, W] int32 id map on one GPU (as u2_panoptic_merge writes it: 0 = void, ids < P);
    gts: per image the ground-truth png's pixels [H, W, 3] uint8 (numpy, as PIL decodes them) or an [H, W] int32 id map;
    gt_tables: per image the ids of the ground truth's segments_info, ascending; num_pred_cols: per image P.
    Returns per image counts int32 [G + 2, P] (see the module text).  A predicted id outside [0, P) is the KeyError of the host
    path; `names` (default: the position in the batch) is what the errors call the images."""
    if not len(pred_maps):
        return []
    batch = _Prepared(pred_maps, gts, gt_tables, num_pred_cols, names)
    batch.upload()
    batch.launch()
    return batch.fetch()
