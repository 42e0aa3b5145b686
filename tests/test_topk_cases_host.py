"""The case builders of tests/topk_cases.py without a GPU: every builder's premise assertions run (they sit in the builders),
every case is consistent with tests/float64_refs.py:topk_rows_ref, and the helpers the premises lean on - the ordered key of
select.hip's header comment and the sweep trace - are held against the reference themselves."""
import numpy as np
import pytest
import torch

from tests import float64_refs as R
from tests import topk_cases as C


def _check_outputs(c):
    ev, ei, ec = C.expect(c)
    rows, k = c["rows"], c["k"]
    assert tuple(ev.shape) == tuple(ei.shape) == (rows, k) and tuple(ec.shape) == (rows,)
    assert ev.dtype == torch.float32 and ei.dtype == torch.int32 and ec.dtype == torch.int32
    real = torch.arange(k)[None] < ec[:, None]
    fill = float("-inf") if c["largest"] else float("inf")
    assert bool((ei[~real] == 0).all()) and bool((ev[~real] == fill).all())
    assert bool((ei >= 0).all()) and bool((ei < 1 << 24).all())
    bits = ev.contiguous().view(torch.int32)
    assert not bool((bits == -0x80000000).any()) and bool((bits[torch.isnan(ev)] == C.QNAN32).all())


@pytest.mark.parametrize("builder", ["digit_edge_cases", "tie_run_cases", "all_equal_cases", "value_class_cases", "k_n_edge_cases",
                                     "view_cases", "carried_cases", "mixed_launch_cases"])
def test_builders_hold_their_premises(builder):
    cases = getattr(C, builder)()
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        if c["k"] > 0 and c["rows"] > 0:
            _check_outputs(c)


def test_ordered_key_ranks_as_the_reference_does():
    """The 64-bit key of the builders' premises (value key : ~index), sorted descending, is the reference's order: on the
    special values of both types, in both directions."""
    for bf16, special in ((False, C.SPECIAL_BITS32), (True, C.SPECIAL_BITS16)):
        bits = np.repeat(np.asarray(special, dtype=np.uint64), 3)
        np.random.default_rng(1).shuffle(bits)
        v = C.from_bits(bits, bf16)[None]
        for largest in (1, 0):
            keys = C.key64(bits, np.arange(len(bits)), largest, bf16)
            assert len(set(keys.tolist())) == len(bits)
            order = np.argsort(keys)[::-1]
            assert R.topk_rows_ref(v, len(bits), bool(largest))[1][0].tolist() == order.tolist()
            ok = C.ordered_key(bits, largest, bf16)
            back = C.ordered_key(C.bits_from_key(ok, largest, bf16), largest, bf16)
            assert (back == ok).all()


def test_sweep_trace_on_rows_worked_by_hand():
    # four keys, distinct top bytes: the 2nd largest is separated in the first sweep
    keys = np.asarray([0x10, 0x20, 0x30, 0x40], dtype=np.uint64) << np.uint64(56)
    assert C.sweep_trace(keys, 2, False) == [(0x30, True)]
    # the two best share the top byte and k = 1: a second sweep has to part them
    keys = (np.asarray([0x4000, 0x4001, 0x3000], dtype=np.uint64) << np.uint64(48))
    assert C.sweep_trace(keys, 1, False) == [(0x40, False), (0x01, True)]
    assert C.sweep_trace(keys, 2, False) == [(0x40, True)]
    assert C.sweep_trace(keys, 3, False) is None
    # equal values, indices 5 and 6 (~index in the low bytes): all seven sweeps for fp32, five for bf16
    keys = np.asarray([0xFFFFFFFF - 5, 0xFFFFFFFF - 6], dtype=np.uint64)
    assert [t[1] for t in C.sweep_trace(keys, 1, False)] == [False] * 6 + [True]
    assert C.sweep_trace(keys, 1, True) == [(0, False), (0, False), (0xFF, False), (0xFF, False), (0xFA, True)]


def test_wide_pairs_and_seams():
    for wide, plain in C.wide_pairs():
        assert wide["dtype"] == 2 and plain["dtype"] == 0 and C.bits_of(wide["store"]).tolist() == C.bits_of(plain["store"]).tolist()
        for a, b in zip(C.expect(wide), C.expect(plain)):
            assert torch.equal(a, b)
    from u2seg_amd.layers.select import _topk_segments
    seen = set()
    for sp, segs in C.seam_specs():
        v = sp["vals"]
        n = sp.get("n") or v.shape[1]
        assert n >= 32768 and _topk_segments(v.shape[0], n, sp.get("group", 1), sp.get("pitch", 1), v[0].numel(), sp["k"]) == segs > 1
        seen.add(segs)
    assert {2, 4, 8} <= seen


@pytest.mark.parametrize("group,pitch,bf16,largest", C.BIG_VIEWS)
def test_big_view_case_is_right_by_construction(group, pitch, bf16, largest):
    """The 2^24 - 1 case states its answer by construction; the same builder at 2^12 - 1 (also a multiple of 3, 5 and 15) is
    small enough to hold that construction against the reference.  The full-size case is built too: its positions lie on both
    sides of 2^23 and reach the last element."""
    c = C.big_view_case(group, pitch, bf16, largest, log2n=12)
    for a, b in zip(C.expect(c), C.expect(dict(c, expect=None))):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    big = C.big_view_case(group, pitch, bf16, largest)
    idx = big["expect"][1][0]
    assert big["n"] == (1 << 24) - 1 and int(idx.max()) == big["n"] - 1 and int(idx.min()) == 0
    assert bool((idx < 1 << 23).any()) and int(((idx >= (1 << 23) - 2 * group) & (idx <= (1 << 23) + 2 * group)).sum()) == 7


def test_rpn_chain_runs_on_the_reference():
    inp = C.rpn_inputs()
    res = C.rpn_chain(inp, C.ref_topk, C.ref_topk_multi)
    v, i, c = res["level 0"]
    ties = sum(int((v[r, 1:] == v[r, :-1]).sum()) for r in range(C.RPN_B))
    assert ties > 50                                                        # quantised logits: the order is mostly the index's
    assert res["level 2"][2].tolist() == [72, 72] and res["score sort"][2].max() < inp["kmax"]
    assert int(res["post top-k"][2].min()) == C.RPN_POST
    assert res["positive draw"][2].tolist()[0] == 24 and res["positive draw"][2].tolist()[1] < 24
