"""layers/deferred.py: the registry of gradients that a backward node leaves to another node behind a zero placeholder.  None of
it needs a GPU: a placeholder is a slice of a zero tensor, and expand() / data_ptr() behave on CPU tensors as on device tensors."""
import pytest
import torch

from u2seg_amd.layers import deferred as D

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def empty_registry():
    D.drain()
    yield
    D.drain()


def in_pool(ph):
    """The placeholder is one of the SLOTS bf16 elements of its (pool) storage."""
    off = ph.data_ptr() - ph.untyped_storage().data_ptr()
    return ph.untyped_storage().nbytes() == 2 * D.SLOTS and 0 <= off < 2 * D.SLOTS and off % 2 == 0


def test_post_returns_a_zero_placeholder_of_the_shape():
    ph = D.post(D.BN_APPLY, CPU, (2, 5, 7, 32), ("dz", "y", "coef"))
    assert tuple(ph.shape) == (2, 5, 7, 32) and ph.dtype == torch.bfloat16 and ph.device == CPU
    assert float(ph.float().abs().sum()) == 0.0 and in_pool(ph)
    assert ph.untyped_storage().data_ptr() == D.post(D.TAIL, CPU, (3,), None).untyped_storage().data_ptr()   # one pool per device
    assert D.pending() == {D.BN_APPLY: 1, D.ROI_GATHER: 0, D.TAIL: 1}


def test_take_answers_the_right_kind_once():
    payload = (object(), 3)
    ph = D.post(D.ROI_GATHER, CPU, (4, 8), payload)
    assert D.take(D.BN_APPLY, ph) is None and D.take(D.TAIL, ph) is None        # another kind: nothing, and nothing changes
    assert D.holds(D.ROI_GATHER, ph) and not D.holds(D.TAIL, ph) and D.pending()[D.ROI_GATHER] == 1
    other = D.post(D.BN_APPLY, CPU, (4, 8), "other")                            # (makes the other kinds' lookups reach the store)
    assert D.take(D.BN_APPLY, ph) is None and D.holds(D.ROI_GATHER, ph)
    assert D.take(D.ROI_GATHER, torch.zeros(4, 8, dtype=torch.bfloat16)) is None   # a foreign tensor
    assert D.holds(D.ROI_GATHER, ph, ph) and not D.holds(D.ROI_GATHER, ph, other)  # the very tensor that was posted
    assert D.take(D.ROI_GATHER, ph) is payload
    assert D.take(D.ROI_GATHER, ph) is None and not D.holds(D.ROI_GATHER, ph)      # exactly once
    assert D.pending() == {D.BN_APPLY: 1, D.ROI_GATHER: 0, D.TAIL: 0}
    assert D.take(D.BN_APPLY, other) == "other"


def test_a_summed_placeholder_is_not_recognised():
    """What autograd does to a conv output with two consumers: the sum is the other gradient, at another address."""
    ph = D.post(D.BN_APPLY, CPU, (2, 3, 32), "payload")
    g = torch.randn(2, 3, 32).bfloat16()
    total = ph + g
    assert torch.equal(total, g)
    assert not D.holds(D.BN_APPLY, total) and D.take(D.BN_APPLY, total) is None
    assert not D.holds(D.BN_APPLY, total, ph)                 # the guard hook's comparison
    assert D.holds(D.BN_APPLY, ph, ph) and D.pending()[D.BN_APPLY] == 1


def test_live_entries_never_share_a_slot():
    phs = [D.post(D.KINDS[i % 3], CPU, (2, 2), i) for i in range(D.SLOTS - 1)]
    assert len({p.data_ptr() for p in phs}) == D.SLOTS - 1 and all(in_pool(p) for p in phs)
    assert D.take(D.KINDS[5 % 3], phs[5]) == 5
    last = D.post(D.TAIL, CPU, (1,), "last")
    again = D.post(D.TAIL, CPU, (1,), "again")                # the pool is full but for the slot that was taken
    assert again.data_ptr() == phs[5].data_ptr() != last.data_ptr()
    assert last.data_ptr() not in {p.data_ptr() for p in phs}
    assert sum(D.pending().values()) == D.SLOTS
    assert D.take(D.TAIL, phs[5]) == "again"                  # the address now answers for its new entry
    for i, p in enumerate(phs):
        if i != 5:
            assert D.take(D.KINDS[i % 3], p) == i


def test_a_full_pool_raises_and_empties_the_store():
    for i in range(D.SLOTS):
        D.post(D.KINDS[i % 3], CPU, (1,), i)
    with pytest.raises(RuntimeError, match="%d deferred gradients were not consumed by their consumers" % D.SLOTS):
        D.post(D.BN_APPLY, CPU, (1,), "one more")
    assert D.pending() == {D.BN_APPLY: 0, D.ROI_GATHER: 0, D.TAIL: 0}
    assert float(D.post(D.BN_APPLY, CPU, (3,), None).float().abs().sum()) == 0.0   # and it works again


def test_drain_and_the_checks_at_the_ends_of_a_step():
    from u2seg_amd.layers import functional as F

    def fill():
        D.post(D.BN_APPLY, CPU, (1,), None)
        for _ in range(2):
            D.post(D.ROI_GATHER, CPU, (1,), None)
        for _ in range(3):
            D.post(D.TAIL, CPU, (1,), None)

    empty = {D.BN_APPLY: 0, D.ROI_GATHER: 0, D.TAIL: 0}
    fill()
    assert D.drain() == {D.BN_APPLY: 1, D.ROI_GATHER: 2, D.TAIL: 3}
    assert D.pending() == empty and D.drain() == empty
    F.reset_deferred_gradients()          # nothing pending: silent
    F.assert_no_deferred_gradients()
    fill()
    with pytest.raises(RuntimeError, match="6 deferred gradients of an earlier backward pass were never consumed"):
        F.reset_deferred_gradients()
    assert D.pending() == empty
    fill()
    F.reset_deferred_gradients(strict=False)
    assert D.pending() == empty
    fill()
    with pytest.raises(RuntimeError, match="1 deferred batch-norm gradients .* 2 deferred ROIAlign gathers .* 3 residual-tail"):
        F.assert_no_deferred_gradients()
    assert D.pending() == empty


def test_an_empty_registry_asks_for_no_address():
    """take() runs in every convolution's and fan-out node's backward: with nothing pending it must not cost a data_ptr()."""

    class NoAddress:
        device = CPU

        def data_ptr(self):
            raise AssertionError("data_ptr() called with nothing pending")

    g = NoAddress()
    for kind in D.KINDS:
        assert D.take(kind, g) is None and not D.holds(kind, g)
    D.post(D.TAIL, CPU, (1,), None)       # another kind pending: still none for these
    assert D.take(D.BN_APPLY, g) is None and D.take(D.ROI_GATHER, g) is None
    with pytest.raises(AssertionError):
        D.take(D.TAIL, g)
