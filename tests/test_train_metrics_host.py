"""Host side of the training metrics: EventStorage / JSONWriter semantics by known answers, the map from an integer counter
row to the reference's scalars (against tests/golden/train_metrics_golden.*, which the reference itself produced), the
averaging over ranks under gloo and the non-finite check.  No GPU."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from u2seg_amd.engine import metrics
from u2seg_amd.utils import events
from u2seg_amd.utils.events import EventStorage, JSONWriter, get_event_storage, has_event_storage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    arrays = np.load(os.path.join(GOLDEN, "train_metrics_golden.npz"))
    with open(os.path.join(GOLDEN, "train_metrics_golden.json")) as f:
        return arrays, json.load(f)


# ---- storage ------------------------------------------------------------------------------------
def test_storage_is_current_only_inside_its_block():
    assert not has_event_storage()
    with pytest.raises(Exception):
        get_event_storage()
    with EventStorage(7) as st:
        assert has_event_storage() and get_event_storage() is st and st.iter == 7
        with EventStorage(0) as inner:
            assert get_event_storage() is inner
        assert get_event_storage() is st
    assert not has_event_storage()
    assert events.step_counters() is None and events.stage_counters() is None


def test_start_iter_step_and_explicit_iteration():
    with EventStorage(100) as st:
        st.put_scalar("a", 1)
        st.step()
        st.put_scalar("a", 2.5)
        st.put_scalar("a", 4, cur_iter=250)
        st.iter = 300
        st.put_scalars(b=1, c=2)
    assert st.history("a").values() == [(1.0, 100), (2.5, 101), (4.0, 250)]
    assert st.latest() == {"a": (4.0, 250), "b": (1.0, 300), "c": (2.0, 300)}
    assert st.history("a").latest() == 4.0
    with pytest.raises(KeyError):
        st.history("missing")


def test_name_scope_nesting():
    with EventStorage() as st:
        st.put_scalar("x", 0)
        with st.name_scope("stage1"):
            st.put_scalar("fast_rcnn/cls_accuracy", 1)
            with st.name_scope("inner/"):      # the reference's rule: the inner scope replaces the outer one ...
                st.put_scalar("y", 2)
            st.put_scalar("z", 3)              # ... and the outer one is back afterwards
        st.put_scalar("w", 4)
    assert sorted(st.latest()) == ["inner/y", "stage1/fast_rcnn/cls_accuracy", "stage1/z", "w", "x"]


def test_median_over_the_last_20_iterations():
    with EventStorage() as st:
        for it in range(50):
            st.put_scalar("every", float(it), cur_iter=it)           # window 30 .. 49: median 39.5
            if it % 7 == 0:
                st.put_scalar("some", float(it), cur_iter=it)        # put at 0, 7, ..., 49; window 30 .. 49 holds 35, 42, 49
            st.put_scalar("lr", 0.5 * it, smoothing_hint=False, cur_iter=it)
        st.put_scalar("early", 3.0, cur_iter=4)
        st.put_scalar("early", 9.0, cur_iter=5)                      # its own last 20 iterations: both values
    out = st.latest_with_smoothing_hint(20)
    assert out["every"] == (39.5, 49)
    assert out["some"] == (42.0, 49)
    assert out["lr"] == (24.5, 49)
    assert out["early"] == (6.0, 5)
    assert st.count_samples("some", 20) == 3 and st.count_samples("every", 20) == 20
    assert st.latest_with_smoothing_hint(1)["every"] == (49.0, 49)
    with EventStorage() as st2:
        st2.put_scalar("a", 1, smoothing_hint=False)
        with pytest.raises(AssertionError):
            st2.put_scalar("a", 1, smoothing_hint=True)


def _three_periods(st, writer, first):
    """Iterations first .. first + 59; `loss` in every one, `acc` not in the last iteration of the second period; the writer
    runs after every 20."""
    for it in range(first, first + 60):
        st.put_scalar("loss", float(it), cur_iter=it)
        st.put_scalar("lr", 0.01, smoothing_hint=False, cur_iter=it)
        if it != first + 39:
            st.put_scalar("stage0/acc", 1.0 / (it + 1), cur_iter=it)
        if (it - first) % 20 == 19:
            writer.write(st)


def test_json_writer_three_periods_and_resume(tmp_path):
    path = str(tmp_path / "metrics.json")
    with EventStorage(0) as st:
        w = JSONWriter(path)
        w.write()           # nothing put yet: nothing written
        _three_periods(st, w, 0)
        w.write(st)         # nothing new
        w.close()
    text = open(path).read()
    lines = text.splitlines()
    rows = [json.loads(x) for x in lines]
    # one line per iteration that has new scalars: 19, then 38 (acc was last put there) and 39, then 59
    assert [r["iteration"] for r in rows] == [19, 38, 39, 59]
    assert rows[0] == {"iteration": 19, "loss": 9.5, "lr": 0.01, "stage0/acc": float(np.median([1.0 / (i + 1) for i in range(20)]))}
    assert rows[1] == {"iteration": 38, "stage0/acc": float(np.median([1.0 / (i + 1) for i in range(19, 39)]))}
    assert rows[2] == {"iteration": 39, "loss": 29.5, "lr": 0.01}
    assert rows[3]["loss"] == 49.5 and rows[3]["stage0/acc"] == float(np.median([1.0 / (i + 1) for i in range(40, 60) ]))
    for line, row in zip(lines, rows):
        assert line == json.dumps(row, sort_keys=True)
        assert list(json.loads(line).keys()) == sorted(row.keys())   # "iteration" is sorted in among the names
    # resume: a new storage that starts at 60 and a new writer on the same file append
    with EventStorage(60) as st:
        assert st.iter == 60
        w = JSONWriter(path)
        _three_periods(st, w, 60)
        w.close()
    again = open(path).read()
    assert again.startswith(text)
    assert [json.loads(x)["iteration"] for x in again.splitlines()] == [19, 38, 39, 59, 79, 98, 99, 119]


# ---- counters -> scalars ------------------------------------------------------------------------
def cls_counts(logits, labels):
    """The five counters of u2_softmax_ce_stats from their definition (numpy's argmax takes the first of equal maxima)."""
    pred = logits.argmax(axis=1)
    bg = logits.shape[1] - 1
    fg = (labels >= 0) & (labels < bg)
    return [int(labels.size), int((pred == labels).sum()), int(fg.sum()), int((fg & (pred == labels)).sum()),
            int((fg & (pred == bg)).sum())]


def mask_counts(z, t):
    wrong = (z > 0) != t
    return [int((wrong & ~t).sum()), int((wrong & t).sum()), int(t.sum()), int(t.size)]


def test_counter_row_reproduces_the_reference_scalars():
    arrays, want = golden()
    for stage, case in enumerate(["cls_mixed", "cls_no_fg", "cls_wide"]):
        row = [0] * events.N_COUNTERS
        base = events.STAGE_SLOTS[stage]
        row[base:base + 5] = cls_counts(arrays[case + "_logits"], arrays[case + "_labels"])
        got = metrics.scalars_from_counters(row, 2)
        mine = {k[len("stage%d/" % stage):]: v for k, v in got.items() if k.startswith("stage%d/fast_rcnn" % stage)}
        assert mine == want[case], case                                  # the names AND the values, exactly
        assert not any(k.startswith("mask_rcnn") for k in got)            # no mask rows: none of the three
        others = [s for s in range(3) if s != stage]
        assert not any(k.startswith("stage%d/fast_rcnn" % s) for s in others for k in got)   # rows == 0: nothing
    assert sorted(want["cls_no_fg"]) == ["fast_rcnn/cls_accuracy"]       # (the fixture does hold the num_fg == 0 case)
    z = arrays["mask_logits"][np.arange(5), arrays["mask_classes"]]
    row = [0] * events.N_COUNTERS
    row[events.MASK_SLOT:events.MASK_SLOT + 4] = mask_counts(z, arrays["mask_targets"])
    got = metrics.scalars_from_counters(row, 2)
    assert {k: v for k, v in got.items() if k.startswith("mask_rcnn")} == {k: v for k, v in want["mask"].items() if k != "loss"}


def test_sample_counts_per_image():
    row = [0] * events.N_COUNTERS
    row[0:2] = [30, 482]
    row[2:7] = [1024, 900, 101, 50, 20]
    row[7:12] = [1024, 0, 77, 0, 0]
    got = metrics.scalars_from_counters(row, 2)
    assert got["rpn/num_pos_anchors"] == 15.0 and got["rpn/num_neg_anchors"] == 241.0
    assert got["roi_head/num_fg_samples"] == 50.5 and got["roi_head/num_bg_samples"] == 461.5
    assert got["stage1/roi_head/num_fg_samples"] == 38.5 and got["stage1/roi_head/num_bg_samples"] == 473.5
    assert got["stage2/roi_head/num_fg_samples"] == 0.0 and got["stage2/roi_head/num_bg_samples"] == 0.0
    assert got["stage0/fast_rcnn/false_negative"] == 20 / 101 and got["stage1/fast_rcnn/fg_cls_accuracy"] == 0.0
    assert "stage2/fast_rcnn/cls_accuracy" not in got


# ---- ring (CPU tensors) -------------------------------------------------------------------------
def test_ring_on_cpu_rows_iterations_and_non_finite():
    names = ["loss_a", "loss_b"]
    ring = metrics.MetricsRing("cpu", period=2)
    with EventStorage(10) as st:
        for it, vals in [(10, [1.0, 2.0]), (11, [3.0, 5.0]), (12, [0.5, 0.25])]:
            ring.begin_step(st, it)
            st.counters[events.STAGE_SLOTS[0]:events.STAGE_SLOTS[0] + 5] += torch.tensor([4, 2, 2, 1, 1], dtype=torch.int32) * (it - 9)
            ring.end_step(st, torch.tensor(vals), names, it, 0.02, 0.1 if it > 10 else 0.0, 0.01, 2)
            st.step()
            if it == 11:
                assert ring.collect(st)
        assert not ring.collect(st)
        ring.start_readout()
        assert ring.collect(st)
    assert st.history("total_loss").values() == [(3.0, 10), (8.0, 11), (0.75, 12)]
    assert st.history("loss_b").values() == [(2.0, 10), (5.0, 11), (0.25, 12)]
    # iteration 12 reused iteration 10's row: it was zeroed in between
    assert st.history("roi_head/num_fg_samples").values() == [(1.0, 10), (2.0, 11), (3.0, 12)]
    assert st.history("stage0/fast_rcnn/cls_accuracy").values() == [(0.5, 10), (0.5, 11), (0.5, 12)]
    assert st.history("time").values() == [(0.1, 11), (0.1, 12)]
    assert st.smoothing_hints()["lr"] is False and st.smoothing_hints()["total_loss"] is True
    ring = metrics.MetricsRing("cpu", period=2)
    with EventStorage(0) as st:
        for it, vals in [(0, [1.0, 2.0]), (1, [float("nan"), 1.0])]:
            ring.begin_step(st, it)
            ring.end_step(st, torch.tensor(vals), names, it, 0.02, 0.0, 0.0, 2)
            st.step()
        with pytest.raises(FloatingPointError, match=r"Loss became infinite or NaN at iteration=1!\nloss_dict = "):
            ring.collect(st)
    with pytest.raises(FloatingPointError, match="iteration=7!"):
        metrics.check_rows_finite([[1.0, 2.0], [float("inf"), 0.0]], [6, 7], names)


def test_ring_restarted_iterations_and_a_step_that_raised():
    """A second storage that starts again at an earlier iteration on the same ring, and a step that never reached end_step:
    the step's row is zeroed before it is handed out, and the rows still waiting are read out, not lost."""
    names = ["loss_a", "loss_b"]
    ring = metrics.MetricsRing("cpu", period=4)
    add = torch.tensor([4, 2, 2, 1, 1], dtype=torch.int32)
    base = events.STAGE_SLOTS[0]

    def step(st, it, times, finish=True):
        ring.begin_step(st, it)
        st.counters[base:base + 5] += add * times
        if finish:
            ring.end_step(st, torch.tensor([1.0, 2.0]), names, it, 0.02, 0.0, 0.0, 2)
            st.step()

    with EventStorage(0) as first:
        step(first, 0, 1)
        step(first, 1, 1)
    with EventStorage(0) as st:
        step(st, 0, 3)                       # row 0 holds the first run's counts: zeroed; its two rows are read out
        assert ring.collect(st)
        step(st, 1, 3, finish=False)         # raised in the middle: the row keeps what was added
        step(st, 1, 5)                       # the same iteration again
        ring.start_readout()
        assert ring.collect(st)
    assert st.history("roi_head/num_fg_samples").values() == [(1.0, 0), (1.0, 1), (3.0, 0), (5.0, 1)]
    # a restart while a full period was read out but not collected: the pending rows are collected into the new storage
    ring = metrics.MetricsRing("cpu", period=2)
    with EventStorage(0) as first:
        step(first, 0, 1)
        step(first, 1, 1)
        step(first, 2, 1)
        assert ring.pending is not None
    with EventStorage(10) as st:
        step(st, 10, 7)
        assert ring.pending is not None      # iteration 2, read out when the new run began
        assert ring.collect(st)
    assert st.history("roi_head/num_fg_samples").values() == [(1.0, 0), (1.0, 1), (1.0, 2)]


# ---- ranks --------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_block(rank):
    block = torch.arange(3 * 4, dtype=torch.float32).reshape(3, 4) * (rank + 1)   # 3 rows, 3 losses + the data time
    block[:, -1] = torch.tensor([0.5, 0.1, 0.3]) if rank == 0 else torch.tensor([0.2, 0.4, 0.3])
    return block


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = metrics.reduce_over_ranks(_rank_block(rank), world)
    out[rank] = got.tolist()
    dist.destroy_process_group()


def test_losses_averaged_and_data_time_maximised_over_two_ranks():
    port = _free_port()
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
        want = (_rank_block(0) + _rank_block(1)) / 2
        want[:, -1] = torch.tensor([0.5, 0.4, 0.3])
        assert out[0] == want.tolist() and out[1] == want.tolist()
    one = _rank_block(0)
    assert metrics.reduce_over_ranks(one, 1) is one
