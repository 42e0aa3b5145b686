"""Segment-pair count tables on the GPU (u2seg_amd/csrc/panopticeval.hip through evaluation/panoptic_ops.pair_counts_batch)
against the numpy definition (host_pair_counts), and the panoptic evaluator fed device tensors against the same evaluator on
the host and against the file route.  Integers throughout: every comparison is ==.  No case here reads or writes out of
bounds on purpose: an out-of-range predicted id is a counted condition that the kernel checks before it indexes."""
import json

import numpy as np
import pytest
import torch

from tests import panoptic_pq_cases as cases
from u2seg_amd.data.pseudo_panoptic import id2rgb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def O():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.evaluation import panoptic_ops

    _hip.load()
    return panoptic_ops


def runs_map(rs, h, w, values, mean_run):
    """[h, w] map of runs (in row-major order, across row ends) of values drawn from `values`."""
    n = h * w
    lengths = rs.geometric(1.0 / mean_run, size=n)[: max(1, n)]
    lengths = lengths[: int(np.searchsorted(np.cumsum(lengths), n)) + 1]
    return np.repeat(rs.choice(values, size=len(lengths)), lengths)[:n].reshape(h, w).astype(np.int64)


def check(O, preds, gts, tables, cols, as_ids=(False, True)):
    """The batch on the device, with the ground truth as png pixels and as int32 ids, == the host, image by image."""
    want = [O.host_pair_counts(p, g, t, c) for p, g, t, c in zip(preds, gts, tables, cols)]
    dev_preds = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)).to(DEV) for p in preds]
    for ids in as_ids:
        dev_gts = [g.astype(np.int32) if ids else id2rgb(g) for g in gts]
        got = O.pair_counts_batch(dev_preds, dev_gts, tables, cols)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == np.int32 and a.shape == b.shape, (k, a.shape, b.shape)
            assert np.array_equal(a, b), (k, preds[k].shape, int(np.abs(a.astype(np.int64) - b).sum()))
    return want


def test_library_exports_the_entry_point(O):
    from u2seg_amd import _hip

    declared, lib = _hip.declared_symbols(), _hip.load()
    for name in ("u2_panoptic_pair_counts", "u2_panoptic_pair_lds_ints"):
        assert name in declared and getattr(lib, name) is not None
    assert O.lds_table_ints() == 15 * 1024


def test_corner_shapes(O):
    """Every H x W of {1, 2, 3, 63, 64, 65} x {1, 5, 67, 1333} (every misalignment of a row of 3-byte pixels, images shorter
    than one 16-pixel piece, pieces that straddle rows) in one ragged batch; all-void maps, one segment covering everything,
    G = 0 and P = 1."""
    rs = np.random.RandomState(11)
    table = [3, 70000, 1 << 20, (1 << 24) - 1]
    preds, gts, tables, cols = [], [], [], []
    for h in (1, 2, 3, 63, 64, 65):
        for w in (1, 5, 67, 1333):
            preds.append(runs_map(rs, h, w, np.arange(6), 9))
            gts.append(runs_map(rs, h, w, [0] + table + [77], 7))
            tables.append(table)
            cols.append(6)
    check(O, preds, gts, tables, cols)
    for h, w in ((3, 5), (65, 67), (64, 1333)):
        zeros, ones = np.zeros((h, w), dtype=np.int64), np.ones((h, w), dtype=np.int64)
        want = check(O, [zeros, ones, ones, zeros, zeros], [zeros, ones * 70000, ones * 70000, ones * 70000, zeros],
                     [table, table, [], table, []], [6, 2, 2, 1, 1])
        assert want[0][0, 0] == h * w and want[1][2, 1] == h * w and want[2][1, 1] == h * w and want[3][2, 0] == h * w
        assert want[4].shape == (2, 1)


def test_no_runs_to_merge(O):
    """A two-id checkerboard and one-pixel stripes: every pixel is a change of pair for the thread that walks it."""
    h, w = 97, 131
    yy, xx = np.indices((h, w))
    board = (yy + xx) % 2
    table = [70000, 1 << 23]
    gt_board = np.where(board == 0, table[0], table[1])
    preds = [board + 1, 2 - board, xx % 2 + 1, yy % 2 + 1, board + 1, np.ones((h, w), dtype=np.int64)]
    gts = [gt_board, gt_board, gt_board, np.where(xx % 2 == 0, table[0], 0), np.full((h, w), table[1]), np.where(yy % 2 == 0, 5, table[0])]
    want = check(O, preds, gts, [table] * 6, [3] * 6)
    assert want[0][1, 1] == (board == 0).sum() and want[0][1, 2] == 0 and want[1][1, 2] == (board == 0).sum()


def test_colour_bytes_unlisted_ids_and_a_table_of_255(O):
    rs = np.random.RandomState(12)
    table = sorted(rs.choice(np.arange(1, 1 << 24), size=255, replace=False).tolist())
    assert len(table) == 255 and sum(1 for t in table if t > 65535 and t & 0xff and (t >> 8) & 0xff) > 200
    unlisted = [t + 1 for t in table[::16] if t + 1 not in table]
    h, w = 120, 333
    gt = runs_map(rs, h, w, [0] + table + unlisted, 11)
    pred = runs_map(rs, h, w, np.arange(40), 13)
    want = check(O, [pred], [gt], [table], [40])
    assert want[0][-1].sum() == np.isin(gt, unlisted).sum() > 0 and (want[0][1:-1].sum(axis=1) > 0).sum() > 200
    # the colour bytes one by one
    for value in (0x0000ff, 0x00ff00, 0xff0000, 0x010203, 0xfffefd):
        g = np.full((5, 7), value, dtype=np.int64)
        want = check(O, [np.ones((5, 7), dtype=np.int64)], [g], [[value]], [2])
        assert want[0][1, 1] == 35


def test_lds_form_and_global_form(O):
    """(G + 2) * P just under the limit of the LDS form, just over it (the same kernel then accumulates straight in the
    output), and an id table longer than the part of it that is searched in LDS."""
    limit = O.lds_table_ints()
    rs = np.random.RandomState(13)
    h, w = 200, 301
    table = sorted(rs.choice(np.arange(1, 1 << 24), size=254, replace=False).tolist())
    gt = runs_map(rs, h, w, [0] + table + [table[-1] - 1 if table[-1] - 1 not in table else 0], 9)
    assert 256 * 60 == limit
    pred = runs_map(rs, h, w, np.arange(60), 9)
    under = check(O, [pred], [gt], [table], [60])[0]      # 15 360 entries: LDS
    over = check(O, [pred], [gt], [table], [61])[0]       # 15 616 entries: global
    assert under.size == limit and over.size == limit + 256 and np.array_equal(over[:, :60], under) and not over[:, 60].any()
    long_table = sorted(rs.choice(np.arange(1, 1 << 24), size=1500, replace=False).tolist())
    gt = runs_map(rs, h, w, [0] + long_table, 5)
    check(O, [pred[:, :], pred % 3], [gt, gt], [long_table, long_table], [60, 3])  # 90 120 entries: global; 4 506: LDS, table global
    # both forms in one launch
    check(O, [pred, pred, pred % 3], [gt, gt, gt], [table, long_table, table[:5]], [61, 60, 3])


def ragged_batch(rs, n):
    preds, gts, tables, cols = [], [], [], []
    for k in range(n):
        h, w = int(rs.randint(1, 140)), int(rs.randint(1, 300))
        g = int(rs.randint(0, 30))
        table = sorted(rs.choice(np.arange(1, 1 << 24), size=g, replace=False).tolist())
        p = int(rs.randint(1, 50))
        preds.append(runs_map(rs, h, w, np.arange(p), 20))
        gts.append(runs_map(rs, h, w, [0, 9] + table, 20))
        tables.append(table)
        cols.append(p)
    return preds, gts, tables, cols


def test_ragged_batch_of_32_in_one_synchronisation(O):
    rs = np.random.RandomState(14)
    preds, gts, tables, cols = ragged_batch(rs, 32)
    dev_preds = [torch.from_numpy(p.astype(np.int32)).to(DEV) for p in preds]
    torch.cuda.synchronize()
    before = dict(O.counters)
    got = O.pair_counts_batch(dev_preds, [id2rgb(g) for g in gts], tables, cols)
    spent = {k: O.counters[k] - before[k] for k in before}
    assert spent == {"host_syncs": 1, "d2h_transfers": 1, "h2d_transfers": 1}
    for a, p, g, t, c in zip(got, preds, gts, tables, cols):
        assert np.array_equal(a, O.host_pair_counts(p, g, t, c))
    # more images than one launch takes (groups of 32), a prediction that is a view at an odd offset, an empty image
    preds, gts, tables, cols = ragged_batch(rs, 41)
    preds[7], gts[7] = np.zeros((0, 5), dtype=np.int64), np.zeros((0, 5), dtype=np.int64)
    dev_preds = [torch.from_numpy(p.astype(np.int32)).to(DEV) for p in preds]
    flat = torch.zeros(preds[3].size + 1, dtype=torch.int32, device=DEV)
    flat[1:] = dev_preds[3].reshape(-1)
    dev_preds[3] = flat[1:].view(preds[3].shape)
    assert dev_preds[3].data_ptr() % 16 != 0
    got = O.pair_counts_batch(dev_preds, [id2rgb(g) for g in gts], tables, cols)
    for a, p, g, t, c in zip(got, preds, gts, tables, cols):
        assert np.array_equal(a, O.host_pair_counts(p, g, t, c))
    assert got[7].shape == (len(tables[7]) + 2, cols[7]) and not got[7].any()


def test_out_of_range_ids_and_bad_ground_truth(O):
    rs = np.random.RandomState(15)
    preds, gts, tables, cols = ragged_batch(rs, 6)
    names = ["img%d.png" % k for k in range(6)]
    dev_preds = [torch.from_numpy(p.astype(np.int32)).to(DEV) for p in preds]
    rgb = [id2rgb(g) for g in gts]
    bad = [p.clone() for p in dev_preds]
    bad[4][-1, -1] = cols[4]         # one past the last column
    with pytest.raises(KeyError, match="img4.png.*not in segments_info"):
        O.pair_counts_batch(bad, rgb, tables, cols, names)
    bad[4] = dev_preds[4]
    bad[2][0, 0] = -1
    with pytest.raises(KeyError, match="img2.png"):
        O.pair_counts_batch(bad, rgb, tables, cols, names)
    with pytest.raises(KeyError):
        O.host_pair_counts(bad[2], gts[2], tables[2], cols[2])
    got = O.pair_counts_batch(dev_preds, rgb, tables, cols, names)  # the next call: nothing is left behind
    for a, p, g, t, c in zip(got, preds, gts, tables, cols):
        assert np.array_equal(a, O.host_pair_counts(p, g, t, c))
    with pytest.raises(ValueError, match="img1.png.*size"):
        O.pair_counts_batch(dev_preds, rgb[:1] + [rgb[1][:, :-1] if rgb[1].shape[1] > 1 else rgb[1][:, :0]] + rgb[2:], tables, cols, names)
    with pytest.raises(ValueError, match="img0.png.*type"):
        O.pair_counts_batch(dev_preds, [gts[0]] + rgb[1:], tables, cols, names)  # int64 ids


@pytest.fixture(scope="module")
def merged():
    assert torch.cuda.is_available()
    sizes = [(800, 1333), (480, 640), (800, 1333), (480, 640)]
    out = cases.seeded_merge(sizes, 40, 1333, DEV)
    assert all(len(info) > 8 for _, info in out)
    return out


def test_maps_of_the_real_merge(O, merged):
    inst_map, sem_map = cases.seeded_mappings()
    preds, gts, tables, cols = [], [], [], []
    for pan, info in merged:
        gt, segs = cases.derived_ground_truth(pan.cpu().numpy(), info, inst_map, sem_map)
        preds.append(pan)
        gts.append(id2rgb(gt))
        tables.append(cases.gt_table_of(segs))
        cols.append(cases.num_pred_cols(info))
    got = O.pair_counts_batch(preds, gts, tables, cols)
    for a, p, g, t, c in zip(got, preds, gts, tables, cols):
        assert np.array_equal(a, O.host_pair_counts(p, g, t, c)) and int(a.sum()) == p.numel()


def test_evaluator_device_host_files(O, merged, tmp_path, monkeypatch):
    """COCOPanopticEvaluator(pq="counts") fed the merge's device tensors == fed the same tensors on the host == pq="files",
    at 800 x 1333 and 480 x 640, in eval mode with unmapped clusters (erased segments)."""
    from u2seg_amd.evaluation import COCOPanopticEvaluator
    from u2seg_amd.evaluation import pq as pqmod

    inst_map, sem_map = cases.seeded_mappings()
    name = "pq_real_" + tmp_path.name
    images, inputs = [], []
    for k, (pan, info) in enumerate(merged):
        gt, segs = cases.derived_ground_truth(pan.cpu().numpy(), info, inst_map, sem_map)
        images.append((k + 1, "%06d.png" % (k + 1), gt, segs))
        inputs.append({"image_id": k + 1, "file_name": "%06d.jpg" % (k + 1), "height": pan.shape[0], "width": pan.shape[1]})
    cases.write_dataset(str(tmp_path), name, images, cases.SEEDED_CATEGORIES, cases.THING_IDS)
    monkeypatch.chdir(tmp_path)
    cases.write_mapping_files({"instance_mapping_file": inst_map, "semantic_mapping_file": sem_map})
    assert any((inst_map if s["isthing"] else sem_map)[str(s["category_id"])] == -1 for _, info in merged for s in info)

    def run(kind, device, out_dir):
        ev = COCOPanopticEvaluator(name, str(tmp_path / out_dir), pq=kind)
        assert ev.mode == "eval"
        outs = [{"panoptic_seg": (pan.to(device), [dict(s) for s in info])} for pan, info in merged]
        before = dict(O.counters)
        ev.process(inputs[:3], outs[:3])
        ev.process(inputs[3:], outs[3:])
        spent = O.counters["host_syncs"] - before["host_syncs"]
        return ev.evaluate()["panoptic_seg"], spent

    (dev, dev_syncs), (host, host_syncs), (files, _) = run("counts", DEV, "dev"), run("counts", "cpu", "host"), run("files", DEV, "files")
    assert dev_syncs == 2 and host_syncs == 0  # one synchronisation per batch of images on the device path
    keys = ("PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st")
    for key in keys:
        assert dev[key] == host[key] == files[key], key
    assert 0 < dev["PQ"] < 100 and dev["pq_implementation"] == "u2seg_amd.evaluation.pq (device counts)"
    assert cases.read_tree(tmp_path / "dev") == cases.read_tree(tmp_path / "host") == cases.read_tree(tmp_path / "files")
    # and the statistics behind the nine numbers, with at least one of every outcome
    stat = pqmod.PQStat()
    cats = {c["id"]: c for c in cases.SEEDED_CATEGORIES}
    pred = {a["image_id"]: a for a in json.load(open(dev["predictions_json"]))["annotations"]}
    samples = []
    for image_id, file_name, gt, segs in images:
        pan = merged[image_id - 1][0].cpu().numpy()
        kept = {s["id"] for s in pred[image_id]["segments_info"]}
        zeroed = np.where(np.isin(pan, sorted(kept)), pan, 0)
        samples.append((gt, segs, zeroed, pred[image_id]["segments_info"]))
        pqmod.accumulate_image(stat, gt, segs, zeroed, pred[image_id]["segments_info"], cats)
    assert min(cases.outcome_counts(stat, samples)) >= 1, cases.outcome_counts(stat, samples)
