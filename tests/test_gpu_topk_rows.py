"""The row top-k selection kernel of u2seg_amd/csrc/select.hip (topk_rows_kernel behind u2_topk_rows / u2_topk_rows_multi, and
the two-launch wrapper of u2seg_amd/layers/select.py) at the places where a radix selection decides: the digit of the k-th key
on a bucket edge, the early exit, tie runs that straddle k and need one, two or three index sweeps, NaNs, infinities and zeros
of both signs, k and n at the block, unroll and LDS limits, the (group, pitch) gather up to the accepted n = 2^24 - 1, carried
indices and counts, several segments per launch, the refusals, and the segment / merge seams.

Reference: tests/float64_refs.py:topk_rows_ref (numpy, written from the contract, held against torch.sort and the sorted fallback
by tests/test_float64_refs_host.py).  Inputs: tests/topk_cases.py, whose builders assert their own premises (run without a GPU
by tests/test_topk_cases_host.py).  Everything is an integer or a bit pattern: indices and counts are compared with ==, values
as int32 views - the contract returns +0.0 for either zero and the quiet NaN 0x7fc00000 for every NaN, and the reference states
exactly that - and positions past the count are compared too (index 0, -inf / +inf).  No tolerance, no element left out."""
import pytest
import torch

from tests import float64_refs as R
from tests import topk_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32 = torch.int32
SENTINEL = 0x5A5A5A5A      # what every output buffer holds before a launch: a finite float, an index no row has


class Env:
    pass


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional
    from u2seg_amd.layers.select import _TopkSeg

    e = Env()
    e.hip, e.F, e.Seg, e.lib = _hip, functional, _TopkSeg, _hip.load()
    return e


def first_diff(name, got, want):
    """Every element equal; the message names the first (row, position) that is not."""
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            name, int(bad.sum()), bad.numel(), i, got[i].item(), want[i].item()))


def same(name, got, want):
    """(values, indices, counts) against (values, indices, counts): values by bit pattern; a part that was not asked for (None on
    the left) is not compared."""
    for what, g, w in zip(("values", "indices", "counts"), got, want):
        if g is None:
            continue
        g, w = g.cpu().contiguous(), w.cpu().contiguous()
        if what == "values":
            assert g.dtype == w.dtype == torch.float32
            g, w = g.view(I32), w.view(I32)
        first_diff("%s: %s" % (name, what), g.to(I32), w.to(I32))


class Launch:
    """The cases of one u2_topk_rows_multi call: device copies of the inputs, sentinel-filled outputs, the U2TopkSeg array."""

    def __init__(self, E, cases, uploaded=None):
        assert 1 <= len(cases) <= 9
        self.cases, self.bufs, segs = cases, [], []
        uploaded = {} if uploaded is None else uploaded

        def dev(t):
            if t is None:
                return None
            if id(t) not in uploaded:
                uploaded[id(t)] = (t, t.to(DEV))       # the CPU tensor is kept so that its id stays its own
            return uploaded[id(t)][1]

        for c in cases:
            store = dev(c["store"])
            assert store.data_ptr() % 8 == 0
            rows, k = c["rows"], c["k"]
            shape = (max(rows, 1), max(k, 1))
            out_v = torch.full(shape, SENTINEL, dtype=I32, device=DEV).view(torch.float32)
            out_i = torch.full(shape, SENTINEL, dtype=I32, device=DEV)
            out_c = torch.full((shape[0],), SENTINEL, dtype=I32, device=DEV)
            mask, idx_in, cnt = dev(c["mask"]), dev(c["idx_in"]), dev(c["cnt"])
            self.bufs.append((store, mask, idx_in, cnt, out_v, out_i, out_c))
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            segs.append(E.Seg(store.data_ptr() + c["offset"] * store.element_size(), ptr(mask), ptr(idx_in), ptr(cnt),
                              out_v.data_ptr() if c["want_vals"] else None, out_i.data_ptr(), out_c.data_ptr() if c["want_cnt"] else None,
                              c["row_stride"], c["dtype"], rows, c["n"], c["group"], c["pitch"], c["mask_value"], k, c["largest"],
                              c["cnt_group"], c["idx_mod"], c["idx_mul"], 0))
        self.segs = segs
        self.E = E

    def run(self, nseg=None):
        arr = (self.E.Seg * len(self.segs))(*self.segs)
        rc = self.E.lib.u2_topk_rows_multi(arr, len(self.segs) if nseg is None else nseg, self.E.hip.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def outputs(self, j):
        """(values or None, indices, counts or None) of case j, on the CPU."""
        c, (_, _, _, _, out_v, out_i, out_c) = self.cases[j], self.bufs[j]
        return (out_v.cpu() if c["want_vals"] else None, out_i.cpu(), out_c.cpu() if c["want_cnt"] else None)

    def untouched(self, j):
        _, _, _, _, out_v, out_i, out_c = self.bufs[j]
        return all(bool((t.view(I32) == SENTINEL).all()) for t in (out_v, out_i, out_c))


def run_cases(E, cases, check=True):
    """Eight cases per launch; every output against C.expect.  Returns the outputs."""
    uploaded, outs = {}, []
    for at in range(0, len(cases), 8):
        part = cases[at: at + 8]
        la = Launch(E, part, uploaded)
        assert la.run() == 0, [c["name"] for c in part]
        for j, c in enumerate(part):
            got = la.outputs(j)
            outs.append(got)
            if check:
                same(c["name"], got, C.expect(c))
            # an output that was not asked for is not written
            assert c["want_vals"] or bool((la.bufs[j][4].view(I32) == SENTINEL).all()), c["name"]
            assert c["want_cnt"] or bool((la.bufs[j][6] == SENTINEL).all()), c["name"]
    return outs


# (a) ---------------------------------------------------------------------------------------------------------------------------
def test_digit_edges_of_the_kth_key(E):
    """The k-th key's digit in bucket 0 and in bucket 255 of every value sweep with all sweeps running, and the chosen bucket
    holding exactly `want` keys (the early exit) in every value sweep; fp32 and bf16, both directions."""
    run_cases(E, C.digit_edge_cases())


# (b) ---------------------------------------------------------------------------------------------------------------------------
def test_tie_runs_straddling_k(E):
    """The k-th value shared by a run of indices inside one 256-block, across a multiple of 256 and across 65 536 (n = 70 000),
    the k-th element on either side of the boundary: three, two and one index sweeps."""
    run_cases(E, C.tie_run_cases())


def test_all_equal_rows(E):
    """One value in the whole row - bf16 zeros, an fp32 constant, zeros of mixed sign: the answer is 0 .. k - 1 for k in
    {1, 255, 256, 257, 4464, 16384} in both directions, and +0.0 for every zero."""
    run_cases(E, C.all_equal_cases())


# (c) ---------------------------------------------------------------------------------------------------------------------------
def test_value_classes(E):
    """+-inf, +-max, +-denormal, +-0 and NaNs of both signs and several payloads, fp32 and bf16, unmasked and masked (a real
    -inf / +inf takes part next to elements that do not), both directions: every NaN is the greatest value and comes back as
    the quiet NaN, among NaNs and among zeros the index decides."""
    run_cases(E, C.value_class_cases())


# (d) ---------------------------------------------------------------------------------------------------------------------------
def test_k_and_n_edges(E):
    """k in {1 .. 5, 1023 .. 1025, 16383, 16384} x n in {1, 2, 63 .. 65, 1023 .. 1025, 8191 .. 8193}: k < n, k = n, k > n,
    fewer participants than k under the mask, none at all; outputs compared past the count; out_vals or out_cnt null."""
    run_cases(E, C.k_n_edge_cases())


# (e) ---------------------------------------------------------------------------------------------------------------------------
def test_group_pitch_views(E):
    """group 1 .. 5 at pitch 8 and 32 (2, 3, 4: the 8-byte grouped path on an aligned row; 1, 5, a misaligned row or n not a
    multiple of group: the generic one), pixel counts around 1024 and 4 x 1024, fp32 views; decoys in everything the view does
    not address.  A case and its twin one element past the 8-byte boundary hold the same rows: same answer."""
    cases = C.view_cases()
    outs = run_cases(E, cases)
    twins = 0
    for j in range(0, len(cases), 2):
        a, b = cases[j], cases[j + 1]
        assert (a["offset"], b["offset"]) == (0, 1) and torch.equal(a["real"].float(), b["real"].float())
        same(b["name"] + " against its aligned twin", outs[j + 1], outs[j])
        twins += 1
    assert twins == len(cases) // 2


@pytest.mark.parametrize("group,pitch,bf16,largest", C.BIG_VIEWS)
def test_view_at_the_accepted_limit(E, group, pitch, bf16, largest):
    """One row of n = 2^24 - 1 elements, the longest the launcher accepts, behind a view: planted values at the first and the
    last element and around the multiples of group next to 2^22, 2^23, 3 * 2^22 and 2^24, decoys beside them.  Pins the element
    -> (pixel, column) division at every magnitude of i the contract admits."""
    c = C.big_view_case(group, pitch, bf16, largest)
    run_cases(E, [c])


# (f) ---------------------------------------------------------------------------------------------------------------------------
def test_carried_indices_and_counts(E):
    """idx_in (a non-monotone permutation; sparse indices up to 1.3e7), idx_in with cnt_in / cnt_group (last groups 0, 1, full),
    idx_mod / idx_mul on rows that are segments of a longer row, through the C ABI."""
    run_cases(E, C.carried_cases())


def test_bf16_keys_in_fp32_storage(E):
    """dtype 2 (two value sweeps over the high halves) gives what dtype 0 (four sweeps) gives on fp32 storage of bf16 values."""
    for wide, plain in C.wide_pairs():
        (w,), (p,) = run_cases(E, [wide]), run_cases(E, [plain])
        same(wide["name"] + " against dtype 0", w, p)


def test_eight_segments_in_one_launch(E):
    """k = 2 next to k = 16384, all dtypes, masks, a view, carried indices, a segment without rows and one with k = 0 in the
    middle: every result as if it had been asked for alone, the skipped segments' outputs untouched."""
    cases = C.mixed_launch_cases()
    la = Launch(E, cases)
    assert la.run() == 0
    for j, c in enumerate(cases):
        if c["rows"] == 0 or c["k"] == 0:
            assert la.untouched(j), c["name"]
            continue
        same(c["name"] + " in the mixed launch", la.outputs(j), C.expect(c))
        same(c["name"] + " against itself alone", la.outputs(j), run_cases(E, [c])[0])


# (g) ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(E):
    """What the launcher refuses comes back as -1 with nothing launched: the outputs of every segment of the call, the valid
    ones included, still hold what they held.  The last accepted values next to each refusal run in the other tests (k = 16384,
    n = 2^24 - 1) and here (an index offset that reaches 2^24 - 1)."""
    g = torch.Generator().manual_seed(43)
    n = 64
    v = C.quantised((2, n), g, False)
    big = torch.zeros(1 << 24, dtype=torch.bfloat16)          # real storage behind the refused n: nothing may be read, and if it were
    cnt = torch.full((2, 10), 3, dtype=I32)
    good = C.make_case("good", v, 2, n, 5, 1)
    bad = dict(
        n_2_24=dict(C.make_case("n", big, 1, (1 << 24) - 1, 5, 1), n=1 << 24),
        k_16385=dict(good, k=16385),
        pitch_below_group=dict(C.make_case("pitch", v, 2, n, 5, 1, group=4, pitch=4), pitch=3),
        dtype_3=dict(good, dtype=3),
        cnt_group_not_dividing_n=dict(good, cnt=cnt, cnt_group=7),
        index_offset_past_2_24=dict(good, idx_mod=2, idx_mul=(1 << 24) - n + 1),
    )
    for name, c in bad.items():
        for cases in ([c], [good, c, good]):
            la = Launch(E, cases)
            assert la.run() == -1, name
            assert all(la.untouched(j) for j in range(len(cases))), name
    for field in ("vals", "out_idx"):
        la = Launch(E, [good, good])
        setattr(la.segs[1], field, None)
        assert la.run() == -1 and la.untouched(0) and la.untouched(1), field
    la = Launch(E, [good] * 9)
    assert la.run() == -1 and all(la.untouched(j) for j in range(9))
    la = Launch(E, [good])
    assert la.run(nseg=0) == 0 and la.untouched(0)
    assert E.lib.u2_topk_rows_multi(None, 0, E.hip.stream_ptr()) == 0
    # accepted: eight segments; the largest index offset (the reported indices reach 2^24 - 1)
    run_cases(E, [good] * 8)
    edge = dict(good, name="index offset up to 2^24 - 1", idx_mod=2, idx_mul=(1 << 24) - n)
    (got,) = run_cases(E, [edge])
    assert int(got[1].max()) > (1 << 24) - n


# (h) ---------------------------------------------------------------------------------------------------------------------------
def test_segment_and_merge_seams(E):
    """F.topk_rows on rows long enough to be cut (n >= 32768), with tie runs and NaNs laid across the seams: equal to the
    reference, to the same rows through the C ABI in one launch, and to the sorted fallback on the device, bit for bit."""
    seen = set()
    for sp, segs in C.seam_specs():
        v = sp["vals"]
        rows, n = v.shape[0], sp.get("n") or v.shape[1]
        group, pitch = sp.get("group", 1), sp.get("pitch", 1)
        name = "seams: rows %d n %d k %d, %d segments" % (rows, n, sp["k"], segs)
        assert E.F._topk_segments(rows, n, group, pitch, v[0].numel(), sp["k"]) == segs > 1, name
        seen.add(segs)
        on_dev = dict(sp, vals=v.to(DEV), mask=None if sp.get("mask") is None else sp["mask"].to(DEV))
        got = E.F.topk_rows(**on_dev)
        torch.cuda.synchronize()
        want = R.topk_rows_ref(**sp)
        same(name + ", wrapper against the reference", got, want)
        one = C.make_case(name, v, rows, n, sp["k"], sp["largest"], row_stride=v[0].numel(), group=group, pitch=pitch,
                          mask=sp.get("mask"))
        same(name + ", wrapper against one launch", got, run_cases(E, [one])[0])
        fv, fi, fc = E.F._topk_rows_sorted(on_dev)
        same(name + ", fallback against the kernel", (fv, fi, fc), got)
    assert {2, 4, 8} <= seen


# (i) ---------------------------------------------------------------------------------------------------------------------------
def test_rpn_composition_at_toy_size(E):
    """Per-level top-k from three 32-wide bf16 maps with quantised logits, the masked score sort (k = n), the masked top-k over
    an image's rows, and the two sampler draws (ascending, masked by label value, no values): the chain on the kernel against
    the same chain on the reference, every intermediate result."""
    inp = C.rpn_inputs()
    on_dev = dict((k, [m.to(DEV) for m in v] if k == "maps" else v.to(DEV) if torch.is_tensor(v) else v) for k, v in inp.items())
    got = C.rpn_chain(on_dev, E.F.topk_rows, E.F.topk_rows_multi)
    want = C.rpn_chain(inp, C.ref_topk, C.ref_topk_multi)
    assert list(got) == list(want)
    for name in want:
        same("rpn chain, " + name, got[name], want[name])
