"""u2_knn (u2seg_amd/csrc/knn.hip: knn_select_kernel<32, 10> of knn_select.h + knn_refine_kernel) against float64, every query row
and every column, none sampled.  The kernel is called through the C ABI so that the test owns the buffers: a workspace of exactly
u2_knn_workspace_ints words with every byte 0xFF (a NaN as a float, -1 as an int: nothing may count on a cleared one), outputs
prefilled with a canary and followed by canary words that must survive.

References: tests/float64_refs.py (knn_ref, knn_key_bound, knn_decidable, lattice_rows - plain torch in float64, held by
tests/test_float64_refs_host.py).  With u = 2^-24 and gamma_n = n u / (1 - n u) (R.gamma32):

A. exact inputs (integer coordinates in [-8, 8], every train row next to its negation so that the column mean is exactly 0): the
   translation is the identity and every key and distance an integer below 2^24, exact in fp32 in any order.  ind_knn equals the
   stable float64 arg-sort and d_knn has the bits of the float64 distance.  Integer distances tie massively: this is the test of
   the (value, index) order through the threshold, the queue, the insertion sort and the refine stage.

B. random inputs.  The refine stage computes sum_d (x - y)^2 in the difference form: one rounding for the difference, one for the
   square, D - 1 for the sum in any order, so |d_knn - d64| <= gamma_(D+1) d64 <= gamma_(D+2) d64.  Per row: indices
   distinct and in range; d_knn ascending, equal values in index order; |d_knn[i, c] - d64(i, ind[i, c])| <= gamma_(D+2) d64; a
   query that is a train row finds itself first at distance exactly 0.  For DECIDABLE rows (R.knn_decidable with R.knn_key_bound:
   the K + 4 candidates provably contain the true top K) also |d64(i, ind[i, c]) - d_sorted64[i, c]| <= 2 gamma_(D+2) d_sorted64[i, c]
   at every c: two rows can only change places where fp32 cannot tell their distances apart.  No row of these cases may be
   undecidable, which is asserted on the reference before the kernel's output is looked at.

C. the spare candidates: a clump of K + 4 train rows at distance 100 from the data mean, where the keys (about -10^4) have a spacing
   of 2^-10 while the clump's distances from a query are 1e-5 apart: the select stage cannot order them, the four spares must.

D. non-finite rows and refusals.

No tolerance here was found by running the kernel."""
import ctypes
import functools

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
CANARY_D = -12345.0
CANARY_I = -777
TAIL = 1024     # canary words behind Nq * K


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


# ----------------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------------
def workspace_ints(H, nq, nt, d, k):
    n = ctypes.c_longlong(-1)
    assert H.call_nostream("u2_knn_workspace_ints", nq, nt, d, k, ctypes.addressof(n)) == 0
    return n.value


def call_knn(H, xq, xt, k, nq=None, nt=None, d=None, ws="exact"):
    """u2_knn through the C ABI -> (status, d_knn [Nq, K], ind_knn [Nq, K]); asserts that the canaries behind Nq * K survive."""
    nq = xq.shape[0] if nq is None else nq
    nt = xt.shape[0] if nt is None else nt
    d = xq.shape[1] if d is None else d
    if isinstance(ws, str):
        ws = torch.full((workspace_ints(H, nq, nt, d, k),), -1, dtype=torch.int32, device=DEV)     # every byte 0xFF
    rows = max(nq, 0) * max(k, 0)
    dk = torch.full((rows + TAIL,), CANARY_D, dtype=torch.float32, device=DEV)
    ik = torch.full((rows + TAIL,), CANARY_I, dtype=torch.int64, device=DEV)
    rc = H.call_nostream("u2_knn", xq, xt, ws, dk, ik, nq, nt, d, k, H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((dk[rows:] == CANARY_D).all()) and bool((ik[rows:] == CANARY_I).all()), "u2_knn wrote beyond Nq * K"
    return rc, dk[:rows].view(max(nq, 0), max(k, 0)), ik[:rows].view(max(nq, 0), max(k, 0))


def run_knn(H, xq, xt, k):
    rc, dk, ik = call_knn(H, xq, xt, k)
    assert rc == 0
    return dk, ik


def same_bits(name, got, want):
    """Every fp32 element has the bits of the reference's; a NaN matches any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            name, int(bad.sum()), bad.numel(), i, got[i].item(), want[i].item()))


def same_ints(name, got, want):
    bad = got != want
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d indices differ; first at %s: got %d, want %d (row: got %s, want %s)" % (
            name, int(bad.sum()), bad.numel(), i, int(got[i]), int(want[i]), got[i[0]].tolist(), want[i[0]].tolist()))


def check_exact(H, name, xt, xq, k, same=False):
    """Lattice inputs: indices equal the stable float64 arg-sort, distances have the bits of the float64 distance."""
    R.assert_lattice(xt, xq)
    xt = xt.to(DEV).contiguous()
    xq = xt if same else xq.to(DEV).contiguous()
    d64, ind64, dist = R.knn_ref(xt, xq, k)
    assert float(dist.max()) < R.TWO24 and torch.equal(dist, dist.round())
    dk, ik = run_knn(H, xq, xt, k)
    same_ints(name + " ind_knn", ik, ind64)
    same_bits(name + " d_knn", dk, d64.float())
    return dist


def refine_gamma(d):
    return float(R.gamma32(d + 2))


def check_rows(name, xt, xq, k, dk, ik, dist, self_index=None):
    """The per-row assertions of B on every row -> d64(i, ind[i, c]) [Nq, K]."""
    nq, nt, g = xq.shape[0], xt.shape[0], refine_gamma(xt.shape[1])
    assert dk.shape == ik.shape == (nq, k)
    assert bool(((ik >= 0) & (ik < nt)).all()), name + ": an index out of range (or a slot that was never written)"
    srt = ik.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), name + ": a train row listed twice"
    assert bool((dk[:, 1:] >= dk[:, :-1]).all()), name + ": d_knn is not ascending"
    tie = dk[:, 1:] == dk[:, :-1]
    assert bool((ik[:, 1:] > ik[:, :-1])[tie].all()), name + ": equal distances out of index order"
    d_at = torch.gather(dist, 1, ik)
    err = (dk.to(F64) - d_at).abs()
    over = ~(err <= g * d_at)
    assert not bool(over.any()), "%s: %d distances beyond gamma_(D+2) d64; first at %s" % (
        name, int(over.sum()), tuple(int(v) for v in over.nonzero()[0]))
    if self_index is not None:
        rows = torch.arange(self_index.numel(), device=ik.device)
        assert bool((dist[rows, self_index] == 0).all())
        assert bool((dk[rows, 0] == 0).all()) and torch.equal(ik[rows, 0], self_index), name + ": a train row does not find itself first"
    return d_at


def check_top_k(name, d_at, d_sorted, d):
    """Decidable rows (every row, where this is called): the true distances of the returned rows are the true sorted distances up to
    what fp32 cannot resolve."""
    over = ~((d_at - d_sorted).abs() <= 2 * refine_gamma(d) * d_sorted)
    assert not bool(over.any()), "%s: %d entries are not the true top K; first at %s" % (
        name, int(over.sum()), tuple(int(v) for v in over.nonzero()[0]))


# ----------------------------------------------------------------------------------------------------------------------------
# A. exact inputs
# ----------------------------------------------------------------------------------------------------------------------------
EX_D = [16, 32, 48, 64]              # the pipeline's prologue only, one prefetch, the first steady-state iteration, one more
EX_NT = ["K", "K+3", 31, 32, 33, 319, 320, 321, 641]   # fewer rows than candidate slots, the 32-row tile, the 320-row pass, two passes + 1
EX_NQ = [1, 127, 128, 129, 257]      # the 128 query rows of a work-group
EX_K = [1, 2, 20, 27, 28]


def _nt(spec, k):
    return {"K": k, "K+3": k + 3}.get(spec, spec)


# every (D, Nt) pair once; Nq and K walk through their lists at different paces, so that every value meets several of the others
# (the four cases of an Nt take four consecutive K of the cyclic list: a short list and a long one among them)
EXACT = [(d, nt, EX_NQ[(4 * ni + di) % 5], EX_K[(ni + di) % 5]) for ni, nt in enumerate(EX_NT) for di, d in enumerate(EX_D)]
EXACT += [(16, 320, 128, 28), (64, 641, 257, 28), (48, "K", 129, 28), (32, "K+3", 1, 1), (16, 321, 127, 27)]


def test_the_exact_grid_covers_what_it_claims():
    assert len(set(EXACT)) == len(EXACT) == 41
    assert {(c[0], c[1]) for c in EXACT} == {(d, n) for d in EX_D for n in EX_NT}
    assert {c[2] for c in EXACT} == set(EX_NQ) and {c[3] for c in EXACT} == set(EX_K)
    for spec in EX_NT:                                          # every Nt with a short and a long list
        ks = {c[3] for c in EXACT if c[1] == spec}
        assert min(ks) <= 2 and max(ks) >= 20, (spec, ks)


@pytest.mark.parametrize("d,nt_spec,nq,k", EXACT, ids=["D%d-Nt%s-Nq%d-K%d" % c for c in EXACT])
def test_exact_lattice(H, d, nt_spec, nq, k):
    nt = _nt(nt_spec, k)
    g = torch.Generator().manual_seed(1000 * d + 10 * nt + k)
    check_exact(H, "D=%d Nt=%d Nq=%d K=%d" % (d, nt, nq, k), R.lattice_rows(nt, d, g), R.lattice_rows(nq, d, g), k)


@pytest.mark.parametrize("d,n,k", [(16, 321, 20), (64, 641, 28), (32, 33, 1), (48, 129, 27)])
def test_exact_lattice_query_is_train(H, d, n, k):
    """The same buffer as query and train set (partitioned_kNN): every row finds itself, or its lowest-numbered copy, first."""
    xt = R.lattice_rows(n, d, torch.Generator().manual_seed(n + d))
    dist = check_exact(H, "self D=%d N=%d K=%d" % (d, n, k), xt, xt, k, same=True)
    assert bool((dist.diagonal() == 0).all())


@pytest.mark.parametrize("d,nt,nq", [(16, 7 * 46, 129), (48, 7 * 92, 257)])
def test_exact_lattice_blocks_of_duplicates(H, d, nt, nq):
    """Every distinct row 7 times, the copies scattered over the tiles, K = 20: blocks of 7 equal distances straddle the 20th place
    and the 24th, the end of the candidate list.  The queries are train rows: 7 zeros lead every list."""
    g = torch.Generator().manual_seed(nt)
    base = R.lattice_rows(nt // 7, d, g)
    xt = base.repeat(7, 1)[torch.randperm(nt, generator=g)]
    xq = xt[torch.randperm(nt, generator=g)[:nq]]
    dist = check_exact(H, "dup D=%d" % d, xt, xq, 20)
    srt = dist.sort(dim=1).values
    assert bool((srt[:, 6] == 0).all()) and bool((srt[:, 14] == srt[:, 20]).all()) and bool((srt[:, 21] == srt[:, 27]).all())


@pytest.mark.parametrize("order", ["decreasing", "increasing"])
@pytest.mark.parametrize("d,nt,nq,k", [(64, 641, 129, 28), (32, 321, 128, 20), (16, 641, 1, 1)])
def test_exact_lattice_ordered_train_rows(H, d, nt, nq, k, order):
    """Train rows in the order of decreasing distance from the queries (all queries are one point, so the order holds for each):
    every row beats the running threshold - 32 survivors per row and tile, every insertion at the head of the list, shifting all
    of it.  In increasing order nothing beats it once the list is full.  Asserted on the float64 distances: the order is monotone
    and at least 2 steps in 3 are strict (integer distances tie)."""
    g = torch.Generator().manual_seed(d + nt)
    xt = R.lattice_rows(nt, d, g)
    q = torch.randint(-8, 9, (1, d), generator=g).float()
    d0 = R.knn_dists(xt, q)[0]
    xt = xt[torch.sort(d0, descending=order == "decreasing", stable=True).indices]     # a permutation: still closed under negation
    d0 = R.knn_dists(xt, q)[0]
    step = d0[1:] - d0[:-1] if order == "increasing" else d0[:-1] - d0[1:]
    assert bool((step >= 0).all()) and float((step > 0).double().mean()) >= 2 / 3
    check_exact(H, "%s D=%d Nt=%d" % (order, d, nt), xt, q.repeat(nq, 1), k)


# ----------------------------------------------------------------------------------------------------------------------------
# B. random inputs
# ----------------------------------------------------------------------------------------------------------------------------
KINDS = ["unit768", "raw768", "normal16", "normal48", "offset32", "affine768"]
NQ, NSELF = 301, 100


def _clustered(n, d, g, clusters=40):
    centers = torch.randn((clusters, d), generator=g)
    return centers[torch.randint(0, clusters, (n,), generator=g)] + 0.4 * torch.randn((n, d), generator=g)


@functools.lru_cache(maxsize=None)
def random_case(kind, nt):
    """(x_train, x_query, self_index [NSELF], reference of k = 28 (d, ind, dist), E) on the device; the first NSELF queries are
    train rows.  Computed once per (kind, Nt) and shared by the K; nobody writes to it."""
    g = torch.Generator().manual_seed(KINDS.index(kind) * 7919 + nt)
    d = int(kind[-3:]) if kind[-3:].isdigit() else int(kind[-2:])
    n = nt + NQ - NSELF
    if kind == "unit768":
        pool = torch.nn.functional.normalize(_clustered(n, d, g), dim=1)
    elif kind == "raw768":
        pool = _clustered(n, d, g)
    elif kind == "affine768":
        pool = torch.nn.functional.normalize(_clustered(n, d, g), dim=1) * 3 + 5
    elif kind == "offset32":
        pool = torch.randn((n, d), generator=g) + 100
    else:
        pool = torch.randn((n, d), generator=g)
    xt = pool[:nt].contiguous().to(DEV)
    self_index = torch.randperm(nt, generator=g)[:NSELF].to(DEV)
    xq = torch.cat([xt[self_index], pool[nt:].to(DEV)]).contiguous()
    return xt, xq, self_index, R.knn_ref(xt, xq, 28), R.knn_key_bound(xt, xq)


@pytest.mark.parametrize("k", [1, 20, 28])
@pytest.mark.parametrize("nt", [641, 1200])
@pytest.mark.parametrize("kind", KINDS)
def test_random_inputs(H, kind, nt, k):
    xt, xq, self_index, (d_sorted, _, dist), e = random_case(kind, nt)
    undecidable = int((~R.knn_decidable(dist, k, e)).sum())
    assert undecidable == 0, "%d of %d rows are undecidable: the case does not test what it is there for" % (undecidable, NQ)
    dk, ik = run_knn(H, xq, xt, k)
    name = "%s Nt=%d K=%d" % (kind, nt, k)
    d_at = check_rows(name, xt, xq, k, dk, ik, dist, self_index)
    check_top_k(name, d_at, d_sorted[:, :k], xt.shape[1])


# ----------------------------------------------------------------------------------------------------------------------------
# C. the spare candidates
# ----------------------------------------------------------------------------------------------------------------------------
def clump_case(k, members, nq=130, nt=641, d=32, seed=0):
    """`members` train rows P + tau_m e_0, tau_m = 1 + 5e-6 m, P = 100 e_1, at random places and in random order among nt - members
    rows of N(0, I); the queries P - sigma_i e_0, sigma_i in [0, 0.2]: the distance of query i from member m is (tau_m + sigma_i)^2,
    between 1 and 1.5, from one member to the next at least 1e-5 apart - above twice the refine stage's bound gamma_34 * 1.5 = 3e-6,
    so the difference form orders them - while E is about 3 gamma_35 * 10^4 = 0.06: the keys, about -10^4 with an fp32 spacing of
    2^-10, cannot tell the members apart at all (the whole clump spans 2e-4), and ties go by train index, not by distance."""
    g = torch.Generator().manual_seed(seed + k + members)
    xt = torch.randn((nt, d), generator=g)
    where = torch.randperm(nt, generator=g)[:members].sort().values
    tau = 1 + 5e-6 * torch.randperm(members, generator=g).to(F64)
    xt[where] = 0.0
    xt[where, 0] = tau.float()
    xt[where, 1] = 100.0
    xq = torch.zeros((nq, d))
    xq[:, 0] = -0.2 * torch.rand(nq, generator=g)
    xq[:, 1] = 100.0
    return xt.to(DEV), xq.to(DEV)


@pytest.mark.parametrize("k", [1, 20, 28])
def test_spare_candidates_are_needed(H, k):
    """A clump of exactly K + 4: every row is decidable, and in every row (at least half are asked for) a row outside the true top K
    lies within 2 E of the K-th - the select stage may rank it above a member of the top K, and only the spares keep that member."""
    xt, xq = clump_case(k, k + R.KN_SPARE)
    d_sorted, _, dist = R.knn_ref(xt, xq, k + 1)
    e = R.knn_key_bound(xt, xq)
    assert bool(R.knn_decidable(dist, k, e).all())
    gaps = d_sorted[:, 1:] - d_sorted[:, :-1] if k > 1 else d_sorted[:, 1:] - d_sorted[:, :1]
    assert float(gaps.min()) > 2 * refine_gamma(32) * float(d_sorted.max())          # the refine stage resolves neighbours
    needed = d_sorted[:, k] <= d_sorted[:, k - 1] + 2 * e
    assert int(needed.sum()) * 2 >= xq.shape[0]
    dk, ik = run_knn(H, xq, xt, k)
    d_at = check_rows("clump K=%d" % k, xt, xq, k, dk, ik, dist)
    check_top_k("clump K=%d" % k, d_at, d_sorted[:, :k], 32)


@pytest.mark.parametrize("k", [1, 20, 28])
def test_more_near_ties_than_spares(H, k):
    """A clump of K + 12: K + 12 rows lie within 2 E of the K-th, every row is undecidable, and the true top K is not promised.
    The per-row assertions hold all the same, and the K-th returned distance is at most (d_(K) + 2 E)(1 + gamma_(D+2)): either
    every row of the true top K is a candidate, or one is not and then all K + 4 candidates have keys no larger than its computed
    key, hence distances <= d_(K) + 2 E; either way K candidates lie that low, and the refine stage adds its own rounding."""
    xt, xq = clump_case(k, k + 12)
    d_sorted, _, dist = R.knn_ref(xt, xq, k)
    e = R.knn_key_bound(xt, xq)
    assert not bool(R.knn_decidable(dist, k, e).any())
    dk, ik = run_knn(H, xq, xt, k)
    check_rows("big clump K=%d" % k, xt, xq, k, dk, ik, dist)
    limit = (d_sorted[:, k - 1] + 2 * e) * (1 + refine_gamma(32))
    assert bool((dk[:, k - 1].to(F64) <= limit).all())


# ----------------------------------------------------------------------------------------------------------------------------
# D. non-finite rows and refusals
# ----------------------------------------------------------------------------------------------------------------------------
BAD_VALUES = [float("nan"), float("inf"), float("-inf")]


def finite_case(kind, nt, nq, d, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "lattice":
        return R.lattice_rows(nt, d, g).to(DEV), R.lattice_rows(nq, d, g).to(DEV)
    return torch.randn((nt, d), generator=g).to(DEV), torch.randn((nq, d), generator=g).to(DEV)


@pytest.mark.parametrize("kind,nt,nq,d,k", [("lattice", 321, 257, 16, 20), ("normal", 641, 301, 48, 28), ("normal", 33, 130, 64, 1)])
def test_non_finite_query_rows(H, kind, nt, nq, d, k):
    """A query row with a NaN, +Inf or -Inf element has no ranked neighbour: its row of d_knn / ind_knn is not written (cluster/knn.py
    prefills NaN / -1).  Every other row is, bit for bit, what the run without those rows gives."""
    xt, xq = finite_case(kind, nt, nq, d, 11)
    dk0, ik0 = run_knn(H, xq, xt, k)
    assert bool(torch.isfinite(dk0).all()) and bool((ik0 >= 0).all())
    bad_rows = [0, 5, 127, 128, nq - 1, 64, 65, 66]
    xb = xq.clone()
    for n, r in enumerate(bad_rows):
        xb[r, (7 * n) % d] = BAD_VALUES[n % 3]
    xb[64] = float("nan")
    xb[65], xb[66, ::2] = float("inf"), float("-inf")
    dk, ik = run_knn(H, xb, xt, k)
    good = torch.ones(nq, dtype=torch.bool, device=DEV)
    good[bad_rows] = False
    assert bool((dk[~good] == CANARY_D).all()) and bool((ik[~good] == CANARY_I).all()), "a non-finite query row was ranked"
    same_bits("d_knn", dk[good], dk0[good])
    same_ints("ind_knn", ik[good], ik0[good])
    from u2seg_amd.cluster import knn as KN

    ind_w, d_w = KN.kNN(xt, xb, K=k)                           # the wrapper: NaN / -1
    assert bool(torch.isnan(d_w[~good]).all()) and bool((ind_w[~good] == -1).all())
    same_bits("wrapper d_knn", d_w[good], dk0[good])


def with_bad_train_rows(xt, at, values, zero_rest):
    """xt with one new row per entry of `at` (ascending positions in the result), element 3 n of the n-th one set to values[n]
    -> (new train set, index map new -> old with -1 at the new rows' places)."""
    nt, d = xt.shape
    keep = torch.ones(nt + len(at), dtype=torch.bool)
    keep[at] = False
    out = torch.empty((nt + len(at), d), device=xt.device)
    out[keep.to(xt.device)] = xt
    for n, r in enumerate(at):
        out[r] = 0.0 if zero_rest else xt[(r * 7) % nt] * 0.5
        out[r, (3 * n) % d] = values[n]
    old = torch.full((nt + len(at),), -1, dtype=torch.int64)
    old[keep] = torch.arange(nt)
    return out.contiguous(), old.to(xt.device)


@pytest.mark.parametrize("kind,nt,nq,d,k", [("lattice", 321, 257, 16, 20), ("lattice", 640, 129, 64, 28), ("normal", 641, 301, 48, 28),
                                            ("normal", 33, 130, 64, 1), ("lattice", 1200, 300, 768, 20)])
@pytest.mark.parametrize("values", [BAD_VALUES[:1], BAD_VALUES[1:2], BAD_VALUES[2:], BAD_VALUES], ids=["nan", "inf", "-inf", "all"])
def test_non_finite_train_rows_are_never_ranked(H, kind, nt, nq, d, k, values):
    """Train rows with a NaN, +Inf or -Inf element among at least K finite ones: every query's list is the list of the run with
    those rows deleted, bit for bit, indices mapped - what torch.sort in the oracle and Kmin_argKmin in the reference give.  (The
    select stage's keys move with the translation point, which the deletion moves; the lists cannot: on lattice inputs the bad
    rows are zero elsewhere, the mean stays exactly 0 and everything is exact; on the random inputs every row is decidable in both
    runs, so both candidate sets contain the true top K, the refine stage's fp32 distance of a pair of rows does not depend on
    the rest, and no row beyond the K-th is close enough to it - 2 gamma_(D+2) relative - for its fp32 distance to come out
    lower, whichever spare candidates a run happens to hold.  All of that is asserted on the reference.)"""
    xt, xq = finite_case(kind, nt, nq, d, 32)      # a seed whose data meets the conditions below: they concern the data alone
    at = sorted([0, 100 % nt, nt + len(values) - 1][: len(values)]) if len(values) > 1 else [(31 * len(str(values[0]))) % nt]
    xb, old = with_bad_train_rows(xt, at, values, zero_rest=kind == "lattice")
    d_sorted, ind64, dist = R.knn_ref(xt, xq, k + 1)
    ind64 = ind64[:, :k].contiguous()
    if kind == "lattice":
        R.assert_lattice(xb.cpu(), xq.cpu())
    else:
        assert bool(R.knn_decidable(dist, k, R.knn_key_bound(xb, xq)).all()) and bool(R.knn_decidable(dist, k, R.knn_key_bound(xt, xq)).all())
        assert float(((d_sorted[:, k] - d_sorted[:, k - 1]) / d_sorted[:, k]).min()) > 2 * refine_gamma(d)
    assert torch.equal(old[R.knn_ref(xb, xq, k)[1]], ind64)                               # the reference itself ranks them last
    dk0, ik0 = run_knn(H, xq, xt, k)
    dk, ik = run_knn(H, xq, xb, k)
    assert bool((ik >= 0).all()), "a slot was never written: the bad train row reached the other rows' keys"
    same_ints("ind_knn", old[ik], ik0)
    same_bits("d_knn", dk, dk0)
    if kind == "lattice":
        same_ints("ind_knn against float64", ik0, ind64)


def test_fewer_finite_train_rows_than_k(H):
    """Nt >= K but only F < K finite train rows: the first F slots of every row hold them, the rest are not written (cluster/knn.py
    prefills NaN / -1).  Column 2 holds +Inf in one bad row and -Inf in another, so for any query one of the two has a key of +Inf
    rather than NaN: neither kind is a neighbour."""
    nt, nq, d, k, f = 40, 130, 32, 28, 19
    xt, xq = finite_case("normal", nt, nq, d, 5)
    bad = torch.arange(nt, device=DEV)[torch.randperm(nt, generator=torch.Generator().manual_seed(1))[: nt - f].to(DEV)]
    for n, r in enumerate(bad.tolist()):
        xt[r, 2 if n < 2 else (5 * n) % d] = BAD_VALUES[(n + 1) % 3]          # +Inf, -Inf, NaN, ...
    finite = torch.isfinite(xt).all(1)
    assert int(finite.sum()) == f and xt[bad[0], 2] == float("inf") and xt[bad[1], 2] == float("-inf")
    d_sorted, ind64, dist = R.knn_ref(xt, xq, k)
    assert bool(finite[ind64[:, :f]].all()) and bool(torch.isfinite(d_sorted[:, :f]).all()) and not bool(torch.isfinite(d_sorted[:, f:]).any())
    dk, ik = run_knn(H, xq, xt, k)
    assert bool((dk[:, f:] == CANARY_D).all()) and bool((ik[:, f:] == CANARY_I).all())
    same_ints("ind_knn", ik[:, :f], ind64[:, :f])
    d_at = check_rows("finite part", xt, xq, f, dk[:, :f].contiguous(), ik[:, :f].contiguous(), dist)
    check_top_k("finite part", d_at, d_sorted[:, :f], d)


def test_refusals_write_nothing(H):
    """D that is no multiple of 16 (8, 24), K outside [1, 28], fewer train rows than K, no workspace: the status and not one word of
    either output; Nq = 0 answers 0."""
    xt, xq = finite_case("normal", 64, 40, 48, 3)
    ws = torch.full((1 << 16,), -1, dtype=torch.int32, device=DEV)

    def status(nq, nt, d, k, w=ws):
        rc, dk, ik = call_knn(H, xq, xt, k, nq=nq, nt=nt, d=d, ws=w)
        assert bool((dk == CANARY_D).all()) and bool((ik == CANARY_I).all())
        assert w is None or bool((w == -1).all())
        return rc

    assert status(40, 64, 8, 5) == -1 and status(40, 64, 24, 5) == -1
    assert status(40, 64, 48, 0) == -1 and status(40, 64, 48, 29) == -1
    assert status(40, 19, 48, 20) == -2 and status(40, 27, 16, 28) == -2
    assert status(40, 64, 48, 5, None) == -1
    assert status(0, 64, 48, 5) == 0
    n = ctypes.c_longlong(-1)
    for k in (0, 29):
        assert H.call_nostream("u2_knn_workspace_ints", 40, 64, 48, k, ctypes.addressof(n)) == -1 and n.value == -1
    assert workspace_ints(H, 40, 64, 48, 5) == 64 + 40 * 9 + 65 * 48
