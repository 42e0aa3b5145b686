"""Scalar storage for training metrics with the contract of detectron2's EventStorage / JSONWriter
(utils/events.py:60-139, 317-537), written from that contract.

An EventStorage keeps, per scalar name, the list of (value, iteration) pairs that were put, the latest pair and whether the
scalar asks for smoothing.  It is made current with `with EventStorage(start_iter) as storage:`; code that logs asks
get_event_storage() (raises outside such a block) or has_event_storage() (never raises).  JSONWriter appends one JSON object
per iteration that has scalars not written yet.

One addition: `storage.counters`, the int32 slice of device memory the loss kernels of the running step add their counts to
(engine/metrics.py sets it; None = nobody collects them)."""
import json
import os
from contextlib import contextmanager

_STORAGES = []

# Layout of `storage.counters`, one step's int32 counter row (engine/metrics.py keeps `period` of them):
#   [0] rpn anchors labelled 1        [1] rpn anchors labelled 0                                   (u2_count_labels_i8)
#   [2 + 5 k ...] cascade stage k:    rows, pred == gt, fg, fg and pred == gt, fg and pred == bg    (u2_softmax_ce_stats)
#   [17 ...] mask head:               false positive, false negative, positive, positions         (u2_mask_predict_bce_stats)
RPN_SLOT = 0
STAGE_SLOTS = (2, 7, 12)
MASK_SLOT = 17
N_COUNTERS = 24   # 21 used; rows stay multiples of 32 bytes


def step_counters():
    """The running step's counter row, or None when no storage is active or nobody collects counters."""
    return _STORAGES[-1].counters if _STORAGES else None


def stage_counters():
    """The five counters of the box stage whose name scope is active ("stage1/..." -> stage 1; no scope: stage 0), or None."""
    row = step_counters()
    if row is None:
        return None
    name = _STORAGES[-1]._prefix.rstrip("/")
    k = int(name[5:]) if name.startswith("stage") and name[5:].isdigit() else 0
    return row[STAGE_SLOTS[k]:STAGE_SLOTS[k] + 5] if k < len(STAGE_SLOTS) else None


def has_event_storage():
    return len(_STORAGES) > 0


def get_event_storage():
    if not _STORAGES:
        raise RuntimeError("no EventStorage is active: open one with `with EventStorage(start_iter):` around the training loop")
    return _STORAGES[-1]


def _median(values):
    v = sorted(values)
    n = len(v)
    return v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2])  # numpy's median: the mean of the two middle values


class History:
    """The (value, iteration) pairs of one scalar, oldest first."""

    def __init__(self):
        self._data = []

    def update(self, value, iteration):
        self._data.append((value, iteration))

    def values(self):
        return self._data

    def latest(self):
        return self._data[-1][0]

    def median(self, window_size):
        return _median([v for v, _ in self._data[-window_size:]])


class EventStorage:
    def __init__(self, start_iter=0):
        self._history = {}
        self._hints = {}
        self._latest = {}
        self._iter = int(start_iter)
        self._prefix = ""
        self.counters = None

    def put_scalar(self, name, value, smoothing_hint=True, cur_iter=None):
        name = self._prefix + name
        it = self._iter if cur_iter is None else cur_iter
        value = float(value)
        self._history.setdefault(name, History()).update(value, it)
        self._latest[name] = (value, it)
        hint = self._hints.setdefault(name, smoothing_hint)
        assert hint == smoothing_hint, "Scalar {} was put with a different smoothing_hint!".format(name)

    def put_scalars(self, *, smoothing_hint=True, cur_iter=None, **kwargs):
        for k, v in kwargs.items():
            self.put_scalar(k, v, smoothing_hint=smoothing_hint, cur_iter=cur_iter)

    def history(self, name):
        if name not in self._history:
            raise KeyError("No history metric available for {}!".format(name))
        return self._history[name]

    def histories(self):
        return self._history

    def latest(self):
        return self._latest

    def smoothing_hints(self):
        return self._hints

    def count_samples(self, name, window_size=20):
        """How many values of `name` were put in the `window_size` iterations that end with its latest one."""
        data = self._history[name].values()
        first = data[-1][1] - window_size
        n = 0
        for _, it in reversed(data):
            if it <= first:
                break
            n += 1
        return n

    def latest_with_smoothing_hint(self, window_size=20):
        """latest(), with the value replaced by the median over the last `window_size` ITERATIONS (however many values were put
        in them) for the scalars that ask for smoothing."""
        out = {}
        for name, (value, it) in self._latest.items():
            if self._hints[name]:
                value = self._history[name].median(self.count_samples(name, window_size))
            out[name] = (value, it)
        return out

    def step(self):
        self._iter += 1

    @property
    def iter(self):
        return self._iter

    @iter.setter
    def iter(self, value):
        self._iter = int(value)

    def __enter__(self):
        _STORAGES.append(self)
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        assert _STORAGES[-1] is self
        _STORAGES.pop()

    @contextmanager
    def name_scope(self, name):
        """Scalars put inside are named `name/...`.  As in the reference an inner scope replaces the outer one for its duration
        (it is not appended to it), and the outer one is back afterwards."""
        old = self._prefix
        self._prefix = name.rstrip("/") + "/"
        try:
            yield
        finally:
            self._prefix = old


class JSONWriter:
    """One line per iteration that has new scalars: {"iteration": it, name: value, ...} with sorted keys, appended to
    `json_file`.  Smoothed scalars are written as their median over the last `window_size` iterations."""

    def __init__(self, json_file, window_size=20):
        self._file = open(json_file, "a")
        self._window_size = window_size
        self._last_write = -1

    def write(self, storage=None):
        storage = get_event_storage() if storage is None else storage
        lines = {}
        for name, (value, it) in storage.latest_with_smoothing_hint(self._window_size).items():
            if it > self._last_write:
                lines.setdefault(it, {})[name] = value
        if lines:
            self._last_write = max(lines)
        for it in sorted(lines):   # (ascending; the reference writes them in the order its dict met them)
            scalars = lines[it]
            scalars["iteration"] = it
            self._file.write(json.dumps(scalars, sort_keys=True) + "\n")
        self._file.flush()
        os.fsync(self._file.fileno())

    def close(self):
        self._file.close()
