"""The streams a training step runs on beside the one it was called on: the weight-gradient side stream, the further compute
streams of independent branches, where the stream-K form of the tile kernel may run beside them, and the queue that hands a
branch's forward pieces to the host-bound stretches of the main chain.

All mutable stream state lives here and nowhere else (layers/functional.py re-exports the functions, never the variables).
"""
import os

import torch
import torch.distributed as dist

from .. import _hip


def _world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


# --------------------------------------------------------------------------------------------
# weight gradients on a second stream
# --------------------------------------------------------------------------------------------
# Nothing in the backward pass reads a weight gradient, so the wgrad kernels of all convolutions run on a side stream:
# they overlap with the data-gradient convs and - more usefully, MFMA work beside HBM-bound work - with the norm /
# ROI backward passes of the main stream, and one fills the other's partially occupied tail rounds.  The side stream
# waits for the main stream at every launch (its operands are produced there); the main stream waits for the side stream
# once, in a callback that autograd runs when the backward pass ends (so `.grad` is complete when backward() returns),
# and wherever gradients are consumed earlier (solver.FlatSGD: the all-reduce of the arena's tail starts inside backward).
_WGRAD_SIDE = os.environ.get("U2_WGRAD_SIDE_STREAM", "1") != "0"
_AUX_ENABLED = True
_side_streams = {}
_side_dirty = {}
_aux_streams = {}


def set_stream_overlap(on):
    """Switch the side stream (weight gradients) and the second compute stream (semantic head) on / off at run time; off =
    every kernel of the step in one stream, one after the other (bench.py times its kernels that way)."""
    global _WGRAD_SIDE, _AUX_ENABLED
    _WGRAD_SIDE = bool(on) and os.environ.get("U2_WGRAD_SIDE_STREAM", "1") != "0"
    _AUX_ENABLED = bool(on)


def _side_stream(device):
    s = _side_streams.get(device)
    if s is None:
        s = _side_streams[device] = torch.cuda.Stream(device=device, priority=int(os.environ.get("U2_SIDE_PRIORITY", "0")))
    return s


def _cuda_device(device):
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def aux_stream(device, index=0):
    """A further compute stream for an independent branch of the model (None when switched off: U2_AUX_STREAM=0).
    index 0: the semantic head; index 1: the mask head beside the box cascade."""
    if not _AUX_ENABLED or os.environ.get("U2_AUX_STREAM", "1") == "0":
        return None
    key = (_cuda_device(device), index)
    s = _aux_streams.get(key)
    if s is None:
        s = _aux_streams[key] = torch.cuda.Stream(device=key[0], priority=int(os.environ.get("U2_AUX_PRIORITY", "0")))
    return s


def join_aux_stream(device, index=0):
    """The current stream waits for everything queued on that further compute stream."""
    if not torch.cuda.is_available() or torch.device(device).type != "cuda":
        return
    s = _aux_streams.get((_cuda_device(device), index))
    if s is not None:
        torch.cuda.current_stream(s.device).wait_stream(s)


def join_all_streams():
    """The current stream waits for the side stream and every further compute stream: used where gradients are consumed
    (optimizer step, gradient all-reduce - also the one of the arena's tail that starts inside the backward pass, when
    the heads' parameter gradients may still be in flight on the streams their branches ran on)."""
    join_wgrad_stream()
    for (dev, _index), s in _aux_streams.items():
        torch.cuda.current_stream(dev).wait_stream(s)


def producer_streams(device):
    """Every stream of this module that may hold gradient-producing work for `device` (weight-gradient side stream, the
    further compute streams); the caller adds the stream it runs the step on."""
    device = _cuda_device(device)
    out = [s for dev, s in _side_streams.items() if _cuda_device(dev) == device]
    out += [s for (dev, _index), s in _aux_streams.items() if dev == device]
    return out


def join_wgrad_stream(device=None):
    """Make the current stream wait for every weight-gradient launch issued so far."""
    for dev, s in _side_streams.items():
        if device is None or dev == torch.device(device):
            _side_dirty[dev] = False
            torch.cuda.current_stream(dev).wait_stream(s)


def _run_wgrad(device, operands, launch):
    """launch() (kernel launches + torch ops) on the side stream; `operands` were produced on the current stream."""
    if not _WGRAD_SIDE:
        launch()
        return
    main = torch.cuda.current_stream(device)
    side = _side_stream(device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        launch()
    for t in operands:
        t.record_stream(side)  # their memory may be released on the main stream while the side stream still reads it
    _side_dirty[device] = True

    def _join():  # runs when the backward pass has finished (queued once per launch: the first one to run does the work)
        if _side_dirty.get(device):
            _side_dirty[device] = False
            torch.cuda.current_stream(device).wait_stream(side)  # the stream backward() was called on

    torch.autograd.Variable._execution_engine.queue_callback(_join)


# ---- where the stream-K form of the tile kernel may be used (round 6) ----
# Recorded in profiles/r06_hang_hunt.txt: the driver's bench command hung in 4 of 23 runs (the chip never finished; the host sat in the
# step's first synchronisation), in 0 of 24 with the stream-K form forbidden, in 0 of 40 with the branch streams (semantic head, mask
# head) switched off, and still in 3 of 30 with the stream-K launches of different streams ordered behind each other by events.  So
# ONE stream-K launch - whose owners spin for peers that the dispatcher has yet to place on a CU, conv_tile.hip - can stall for good
# while kernels of a branch stream compete for the CUs; the mechanism is not understood (the weight-gradient side stream beside
# stream-K launches: 0 of 20).  Until it is, the product path asks for the stream-K form only where no branch stream has work in
# flight: inside the bottom-up backbone (forward: nothing else has been launched yet; backward: the heads' streams have been
# joined by the FPN's gradient fan-in), and anywhere when the branch streams are off (set_stream_overlap(False)).  Elsewhere the
# calls carry U2_CV_STREAMK_FORBID of the conv word (include/u2seg_hip.h: whole tiles).  U2_STREAMK_EVERYWHERE=1 restores the old
# behaviour.
_NO_STREAMK = _hip.K.CV_STREAMK_FORBID
_SK_REGION = [0]


class streamk_region:
    """with streamk_region(): the convolutions created inside (and their backward passes) may take the stream-K form."""

    def __enter__(self):
        _SK_REGION[0] += 1

    def __exit__(self, *exc):
        _SK_REGION[0] -= 1
        return False


def _conv_variant():
    if os.environ.get("U2_STREAMK_EVERYWHERE", "0") == "1" or "U2_CONV_VARIANT" in os.environ:
        return 0   # (U2_CONV_VARIANT: tests and A/B runs steer the library's dispatch themselves; it only applies to variant 0)
    if _world() > 1:
        # the gradient exchange of the arena's tail (RCCL kernels on their own stream, solver/build.py:begin_all_reduce_tail) runs
        # beside the backbone's backward pass: another stream competing for the CUs - never measured, so not risked
        return _NO_STREAMK
    if _SK_REGION[0] > 0 or not _AUX_ENABLED or os.environ.get("U2_AUX_STREAM", "1") == "0":
        return 0
    return _NO_STREAMK


# ---- an independent branch issued in pieces where the main chain is host-bound (round 6) ----
# The proposal bookkeeping of the ROI heads (match / relabel / sample between the cascade stages: ~40 tiny launches and one host
# synchronisation each) leaves the chip idle for 0.6-1.3 ms at a time while the host catches up (tools/step_idle.py: 3.7 ms of a 58 ms
# step).  A branch that only shares the FPN maps with it - the semantic head - is therefore not launched as a whole beside the RPN
# but handed over as a list of pieces; the bookkeeping code calls issue_branch_piece() right before it becomes host-bound, and the
# piece's kernels (on the branch's own stream) run while the host synchronises and launches the small stuff.
_branch_pieces = []


def queue_branch_pieces(pieces):
    """Queue closures (each launches one piece of an independent branch on that branch's stream)."""
    _branch_pieces.extend(pieces)


def issue_branch_piece(n=1):
    """Launch the next n queued pieces (no-op when nothing is queued)."""
    while n > 0 and _branch_pieces:
        _branch_pieces.pop(0)()
        n -= 1


def flush_branch_pieces():
    """Launch whatever is still queued (the owner of the branch calls this before it joins the branch's stream)."""
    issue_branch_piece(len(_branch_pieces))


def clear_branch_pieces():
    """Drop queued pieces (a forward pass that raised midway must not leave its pieces to the next one)."""
    del _branch_pieces[:]
