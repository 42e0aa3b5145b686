"""Training metrics from counters kept on the device.

The reference logs ~25 scalars per step with one `.item()` each (rpn.py:396-403, roi_heads.py:290-300, cascade_rcnn.py:243-255,
fast_rcnn.py:88-115, mask_head.py:90-102, train_loop.py:376-421).  Here the loss kernels add integer counts to one row of a
ring on the device, the step's stacked losses are copied into the same row of a second ring, and every `period` steps both
rings go to a pinned mirror with one non-blocking copy; the host waits for that copy's event once, where the training loop
waits for the device anyway, and derives the scalars from the integer rows with Python float division.

The layout of a counter row is in utils/events.py.
"""
import math
import time

import torch

from ..layers import functional as F
from ..utils.events import MASK_SLOT, N_COUNTERS, RPN_SLOT, STAGE_SLOTS

PERIOD = 20   # the reference's writer period (engine/defaults.py:build_writers)
RPN, STAGE, MASK = RPN_SLOT, STAGE_SLOTS, MASK_SLOT


def scalars_from_counters(row, num_images):
    """One step's integer counter row -> {name: float}, the names and the subset the reference puts:
      rpn/num_pos_anchors, rpn/num_neg_anchors                       counts / images
      roi_head/num_fg_samples, roi_head/num_bg_samples               stage 0: fg / images, (rows - fg) / images
      stage{1,2}/roi_head/num_fg_samples|num_bg_samples              the same from stage 1 and 2
      stage{k}/fast_rcnn/cls_accuracy (rows > 0), fg_cls_accuracy and false_negative (fg > 0)
      mask_rcnn/accuracy, false_positive, false_negative             only in a step with mask rows
    The stage-k sample counts: cascade_rcnn.py:243-244 counts the matcher's label 1 over all boxes of the stage, and
    cascade_rcnn.py:231-236 gives exactly those boxes a class below num_classes and every other box num_classes (the
    matcher of a cascade stage has no ignore label), so (fg, rows - fg) of the stage's classification loss are the same
    two numbers; for stage 0, roi_heads.py:290-300 counts gt_classes == num_classes over the sampled rows, which never
    hold -1, and that is rows - fg again.
    Naming: the classification scalars are always stage{k}/fast_rcnn/..., the cascade's names.  A box head outside a cascade
    has no name scope and counts into stage 0's slots, where the reference would log plain fast_rcnn/...; only the cascade
    configuration ships."""
    row = [int(v) for v in row]
    n = max(int(num_images), 1)
    out = {"rpn/num_pos_anchors": row[RPN] / n, "rpn/num_neg_anchors": row[RPN + 1] / n}
    for k, base in enumerate(STAGE):
        rows, acc, fg, fg_acc, fn = row[base:base + 5]
        prefix = "" if k == 0 else "stage%d/" % k
        out[prefix + "roi_head/num_fg_samples"] = fg / n
        out[prefix + "roi_head/num_bg_samples"] = (rows - fg) / n
        if rows > 0:
            out["stage%d/fast_rcnn/cls_accuracy" % k] = acc / rows
            if fg > 0:
                out["stage%d/fast_rcnn/fg_cls_accuracy" % k] = fg_acc / fg
                out["stage%d/fast_rcnn/false_negative" % k] = fn / fg
    false_pos, false_neg, pos, total = row[MASK:MASK + 4]
    if total > 0:
        out["mask_rcnn/accuracy"] = 1 - (false_pos + false_neg) / max(total, 1.0)
        out["mask_rcnn/false_positive"] = false_pos / max(total - pos, 1.0)
        out["mask_rcnn/false_negative"] = false_neg / max(pos, 1.0)
    return out


def reduce_over_ranks(block, world_size, group=None):
    """train_loop.py:395-421 for a whole period at once.  block: float32 [rows, n + 1] of this rank, columns 0 .. n-1 the
    losses, column n the data time.  Returns the same shape: the losses averaged over the ranks, the data time maximised.
    One collective (an all-gather of the block)."""
    if world_size <= 1:
        return block
    import torch.distributed as dist

    parts = [torch.empty_like(block) for _ in range(world_size)]
    dist.all_gather(parts, block.contiguous(), group=group)
    every = torch.stack(parts)
    out = every.sum(dim=0) / world_size
    out[:, -1] = every[:, :, -1].max(dim=0).values
    return out


def _world_size():
    import torch.distributed as dist

    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def check_rows_finite(loss_rows, iterations, names):
    """Raises the reference's FloatingPointError (train_loop.py:411-415) for the first row whose total is not finite."""
    for vals, it in zip(loss_rows, iterations):
        total = sum(vals)
        if not math.isfinite(total):
            raise FloatingPointError("Loss became infinite or NaN at iteration={}!\nloss_dict = {}".format(
                it, dict(zip(names, vals))))


class MetricsRing:
    """`period` rows of counters and of losses on the device, their pinned mirror, and the host-side values of each row
    (iteration, lr, step time, data time, images)."""

    def __init__(self, device, period=PERIOD):
        self.device, self.period = torch.device(device), int(period)
        self.counters = torch.zeros((self.period, N_COUNTERS), dtype=torch.int32, device=self.device)
        pin = self.device.type == "cuda"
        self.counters_host = torch.zeros((self.period, N_COUNTERS), dtype=torch.int32, pin_memory=pin)
        self.losses = self.losses_host = self.data_time_host = None   # sized by the first step's loss dict
        self.names = None
        self.rows = []          # rows filled since the last read-out: (row, iteration, lr, time, data_time, images)
        self.pending = None     # (rows, event) of a read-out whose copy was started and not yet collected
        self._row = None
        self._begun = None      # the iteration begin_step was last called for

    def begin_step(self, storage, iteration):
        """The counter slice of this step.  Its row was zeroed at allocation or by end_step of the step before; where the
        iteration does not follow the last one begun (another storage on the same trainer, or a step that raised before its
        end_step), the rows still waiting are read out first (after collecting a read-out that is still pending) and the
        step's own row is zeroed here, on the stream every stream of the step starts from."""
        row = iteration % self.period
        if self._begun is not None and iteration != self._begun + 1:
            if iteration != self._begun:   # (the same iteration again: a step that raised; its earlier rows just stay queued)
                if self.pending is not None:   # a read-out nobody collected: the mirror is taken, so it is collected here
                    self.collect(storage, world_size=_world_size())   # (a wait, but on a restart, not in the training loop)
                self.start_readout(_world_size())
            self.counters[row].zero_()
        self._begun, self._row = iteration, row
        storage.counters = self.counters[row]

    def end_step(self, storage, stacked_losses, names, iteration, lr, step_time, data_time, images):
        """Behind the optimizer step: the loss row, the read-out when the ring is full, and the zeroing of the next step's row.
        Everything here is stream-ordered device work; nothing waits."""
        if self.losses is None:
            self.names = list(names)
            n = len(self.names) + 1   # (one more column: the data time, filled only where several ranks exchange the block)
            self.losses = torch.zeros((self.period, n), dtype=torch.float32, device=self.device)
            pin = self.device.type == "cuda"
            self.losses_host = torch.zeros((self.period, n), dtype=torch.float32, pin_memory=pin)
            self.data_time_host = torch.zeros((self.period,), dtype=torch.float32, pin_memory=pin)
        assert list(names) == self.names, "the loss dict changed its keys"
        row = self._row
        self.losses[row, :-1].copy_(stacked_losses.detach())
        self.rows.append((row, iteration, lr, step_time, data_time, images))
        storage.counters = None
        # the semantic and the mask head ran on side streams: their counts and the next step's zeroing meet on this stream
        if self.device.type == "cuda":
            F.join_all_streams()
        if row == self.period - 1:
            self.start_readout(_world_size())
        self.counters[(row + 1) % self.period].zero_()

    def start_readout(self, world_size=1):
        """One non-blocking copy of both rings to the pinned mirror and an event behind it."""
        if not self.rows:
            return
        if self.pending is not None:
            raise RuntimeError("the previous read-out was not collected: call collect() once per period")
        losses = self.losses
        if world_size > 1:
            for row, _, _, _, data_time, _ in self.rows:
                self.data_time_host[row] = data_time
            self.losses[:, -1].copy_(self.data_time_host, non_blocking=True)
            losses = reduce_over_ranks(self.losses, world_size)
        self.counters_host.copy_(self.counters, non_blocking=True)
        self.losses_host.copy_(losses, non_blocking=True)
        event = None
        if self.device.type == "cuda":
            event = torch.cuda.Event()
            event.record()
        self.pending, self.rows = (self.rows, event), []

    def collect(self, storage, write=True, world_size=1):
        """The one wait: for the read-out's event.  Then the scalars of every row go to `storage` under the row's iteration.
        write=False (ranks other than 0): the rows are dropped after the finiteness check."""
        if self.pending is None:
            return False
        rows, event = self.pending
        self.pending = None
        if event is not None:
            event.synchronize()
        counters = self.counters_host.tolist()
        losses = self.losses_host.tolist()
        check_rows_finite([losses[r[0]][:-1] for r in rows], [r[1] for r in rows], self.names)
        if not write:
            return True
        for row, iteration, lr, step_time, data_time, images in rows:
            vals = losses[row]
            if world_size > 1:
                data_time = vals[-1]
            for name, value in scalars_from_counters(counters[row], images).items():
                storage.put_scalar(name, value, cur_iter=iteration)
            storage.put_scalar("data_time", data_time, cur_iter=iteration)
            storage.put_scalar("total_loss", sum(vals[:-1]), cur_iter=iteration)
            if len(self.names) > 1:
                storage.put_scalars(cur_iter=iteration, **dict(zip(self.names, vals[:-1])))
            storage.put_scalar("lr", lr, smoothing_hint=False, cur_iter=iteration)
            if step_time > 0:   # (the first step of a run has no step before it to measure from)
                storage.put_scalar("time", step_time, cur_iter=iteration)
        return True


class StepClock:
    """Host time from one step's start to the next (the steady-state step time of an asynchronous loop)."""

    def __init__(self):
        self._t = None

    def lap(self):
        now = time.perf_counter()
        dt = 0.0 if self._t is None else now - self._t
        self._t = now
        return dt
