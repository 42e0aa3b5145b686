"""The k-means M step (u2_kmeans_update + u2_kmeans_finalize, u2seg_amd/csrc/kmeans.hip) per element against float64 on both of
its forms, and the E step on non-finite centroids.  u2_kmeans_update is called through the C ABI so that the test picks the form:
a workspace of u2_kmeans_update_workspace_floats gives the segmented form (histogram, scan, scatter, km_segsum_kernel<DPT>),
None the privatised-LDS form (kmeans_update_kernel<64 | 32 | 16>) that production Python reaches only for D > 2048.

References: tests/float64_refs.py (kmeans_update_ref, kmeans_argmin_ref - plain torch in float64, held against the oracle by
tests/test_float64_refs_host.py).  Two kinds of input for every M-step case, every cluster and dimension checked, none sampled:

A. exact inputs: integer-valued x in [-64, 64], at most 2^17 rows per cluster (N <= 70 000), so every partial sum is an integer
   below 2^24 - an fp32 number in any order of summation.  csum, counts and centroids equal the reference bit for bit (NaN == NaN);
   the centroid is the one correctly rounded quotient of two fp32 numbers (rounding the float64 quotient again is innocuous for
   division, and the build has no fast-math).

B. random inputs: randn with a tenth of the rows x 1e3 and a tenth x 1e-3.  fp32 summation of n terms in any order and association,
   atomics included, obeys |fl(sum) - sum| <= gamma_(n-1) sum|x|, gamma_m = m 2^-24 / (1 - m 2^-24).  So
     |csum - ref_sum| <= gamma_(n_j) sum_abs            and   |c - ref_c| <= gamma_(n_j) sum_abs / n_j + 2^-24 |ref_c|
   elementwise (the second: the sum's error divided by the exact count, plus the division's rounding).  Nothing here is measured."""
import functools

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


# ----------------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------------
def workspace(H, n, d, k):
    """A workspace of the size the library asks for, every word -1 (not zero: the kernels must not count on a cleared one; as an
    int32 -1 is what they treat as "no entry")."""
    return torch.full((H.call_nostream("u2_kmeans_update_workspace_floats", n, d, k),), -1, dtype=torch.int32, device=DEV).view(torch.float32)


def run_update(H, x, labels, k, form, csum=None, counts=None, ws=None):
    """u2_kmeans_update in the given form ("seg" / "priv") into csum / counts (fresh zeros unless given) -> (csum, counts)."""
    n, d = x.shape
    if csum is None:
        csum, counts = torch.zeros((k, d), device=DEV), torch.zeros(k, device=DEV)
    if form == "seg" and ws is None:
        ws = workspace(H, n, d, k)
    H.call("u2_kmeans_update", x, labels, csum, counts, n, d, k, ws if form == "seg" else None)
    return csum, counts


CANARY = -12345.0


def run_finalize(H, csum, counts):
    """u2_kmeans_finalize into a buffer with 1024 canary floats behind K * D, which must survive."""
    k, d = csum.shape
    out = torch.full((k * d + 1024,), CANARY, device=DEV)
    H.call("u2_kmeans_finalize", csum, counts, out, d, k)
    assert bool((out[k * d:] == CANARY).all()), "u2_kmeans_finalize wrote beyond K * D"
    return out[: k * d].view(k, d)


def same_bits(name, got, want):
    """Every fp32 element has the bits of the reference's (so -0.0 is not +0.0); a NaN matches any NaN."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (
            name, int(bad.sum()), bad.numel(), i, got[i].item(), want[i].item()))


def within(name, got, want, bound):
    """Where the float64 reference is finite: |got - want| <= bound; where it is not: the same NaN / the same infinity."""
    g = got.to(F64)
    fin = torch.isfinite(want)
    odd = ~fin & ~((torch.isnan(g) & torch.isnan(want)) | (g == want))
    assert not bool(odd.any()), "%s: %d non-finite reference elements not matched; first at %s" % (
        name, int(odd.sum()), tuple(int(v) for v in odd.nonzero()[0]))
    err = torch.where(fin, (g - torch.where(fin, want, 0.0)).abs(), 0.0)
    over = fin & ~(err <= bound)          # a NaN where a number belongs fails here
    if bool(over.any()):
        i = tuple(int(v) for v in over.nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond their bound; first at %s: got %r, want %r, bound %.3g" % (
            name, int(over.sum()), over.numel(), i, got[i].item(), want[i].item(), float(bound[i])))


def check_exact(H, name, x, labels, k, csum, counts):
    s, n, _ = R.kmeans_update_ref(x, labels, k)
    xf = x[torch.isfinite(x)]
    assert int(n.max()) <= 1 << 17 and float(xf.abs().max()) <= 64 and torch.equal(xf, xf.round())   # partial sums below 2^23
    same_bits(name + " counts", counts, n.float())
    same_bits(name + " csum", csum, s.float())
    same_bits(name + " centroids", run_finalize(H, csum, counts), (s / n.to(F64)[:, None]).float())


def centroid_bound(n, sum_abs, ref_c):
    """gamma_(n_j) sum_abs / n_j + 2^-24 |ref_c|; an empty cluster is 0 / 0 = NaN on both sides and its bound is never looked at."""
    nn = n.to(F64)[:, None]
    return torch.nan_to_num(R.gamma32(nn) * sum_abs / nn, nan=0.0, posinf=0.0) + R.U24 * ref_c.abs()


def check_random(H, name, x, labels, k, csum, counts):
    s, n, a = R.kmeans_update_ref(x, labels, k)
    same_bits(name + " counts", counts, n.float())
    within(name + " csum", csum, s, R.gamma32(n.to(F64))[:, None] * a)
    ref_c = s / n.to(F64)[:, None]
    within(name + " centroids", run_finalize(H, csum, counts), ref_c, centroid_bound(n, a, ref_c))


def make_x(kind, n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "exact":
        return torch.randint(-64, 65, (n, d), generator=g, device=DEV).float()
    x = torch.randn((n, d), generator=g, device=DEV)
    scale = torch.ones(n, device=DEV)
    scale[0::10] = 1e3
    scale[5::10] = 1e-3
    return x * scale[:, None]


def check_case(H, kind, form, n, d, k, pattern, seed):
    x = make_x(kind, n, d, seed)
    labels = R.kmeans_labels(pattern, n, k, torch.Generator().manual_seed(seed)).to(DEV)
    csum, counts = run_update(H, x, labels, k, form)
    name = "%s %s N=%d D=%d K=%d %s" % (form, kind, n, d, k, pattern)
    (check_exact if kind == "exact" else check_random)(H, name, x, labels, k, csum, counts)


# ----------------------------------------------------------------------------------------------------------------------------
# the case grids
# ----------------------------------------------------------------------------------------------------------------------------
# Segmented form.  D: every DPT of km_segsum_kernel (1, 2, 3, 4, 8) at its upper edge and just past the lower one, odd widths;
# N: around the 8 rows in flight, KM_SEG = 256 entries per work-group and KM_SCAT = 4096 points per scatter work-group, and many
# work-groups; K: around the scan's chunks of ceil(K / 256) labels per thread, and the 64 KB LDS tables (16384).
SEG_CASES = [
    (1, 1, 1, "first"), (7, 3, 2, "uniform"), (8, 16, 2, "rr"), (9, 255, 1, "first"), (255, 256, 255, "rr"),
    (256, 257, 256, "rr"), (257, 300, 257, "rr"), (4095, 512, 300, "uniform"), (4096, 513, 511, "sorted"),
    (4097, 768, 513, "uniform"), (8193, 769, 800, "rr"), (66003, 1024, 300, "uniform"), (8193, 1025, 2, "sorted"),
    (4097, 2047, 255, "holes"), (4096, 2048, 256, "uniform"), (66003, 16, 16384, "uniform"), (66003, 16, 16384, "rr"),
    (66003, 768, 300, "last"), (66003, 256, 800, "first"), (8193, 768, 300, "runs"), (4097, 257, 513, "runs"),
    (66003, 300, 800, "holes"), (8193, 1, 300, "rr"), (257, 2048, 2, "rr"), (4095, 3, 800, "sorted"),
    (256, 1025, 511, "uniform"), (255, 2047, 257, "holes"), (9, 16, 16384, "uniform"), (8193, 2048, 300, "sorted"),
    (4096, 769, 1, "first"), (66003, 513, 2, "rr"), (7, 1024, 255, "holes"), (8, 300, 256, "rr"),
    (4097, 16, 16384, "sorted"), (1, 2048, 800, "last"), (257, 255, 300, "runs"), (66003, 769, 511, "runs"),
    (4096, 1, 1, "first"), (8193, 512, 257, "last"), (255, 3, 2, "first"),
]

# Privatised form.  K: the switches DS 64 -> 32 -> 16 of (size_t)K * (DS + 1) * 4 <= 144 * 1024 (567 | 568, 1117 | 1118) and the
# last K served (2168); D: the scalar tail (D % 4 != 0), multiples of 4 that are no multiple of DS, several blockIdx.y;
# N: around one pass of the work-group (64 points at DS = 64) and around ppb = 8192 points per work-group.
PRIV_CASES = [
    (1, 1, 1, "first"), (63, 3, 300, "uniform"), (64, 4, 567, "rr"), (65, 60, 568, "uniform"), (8191, 64, 1117, "uniform"),
    (8192, 68, 1118, "rr"), (8193, 100, 2168, "uniform"), (20000, 770, 300, "uniform"), (20000, 2052, 567, "sorted"),
    (8193, 2052, 1, "first"), (20000, 100, 2168, "holes"), (8192, 770, 568, "last"), (8193, 3, 1118, "runs"),
    (20000, 60, 1117, "rr"), (65, 68, 2168, "uniform"), (8191, 1, 567, "sorted"), (20000, 4, 1, "first"), (64, 2052, 300, "rr"),
]


def _ids(cases):
    return ["N%d-D%d-K%d-%s" % c for c in cases]


def test_the_case_grids_cover_what_they_claim():
    """Every D, N, K and label pattern the grids are there for occurs (a case edited away would otherwise go unnoticed)."""
    n, d, k, p = (set(c[i] for c in SEG_CASES) for i in range(4))
    assert d == {1, 3, 16, 255, 256, 257, 300, 512, 513, 768, 769, 1024, 1025, 2047, 2048}
    assert n == {1, 7, 8, 9, 255, 256, 257, 4095, 4096, 4097, 8193, 66003}
    assert k == {1, 2, 255, 256, 257, 300, 511, 513, 800, 16384}
    assert p == {"uniform", "sorted", "rr", "first", "last", "runs", "holes"}
    assert {(dd + 255) // 256 for dd in d} == {1, 2, 3, 4, 5, 8} and all(c[1] == 16 for c in SEG_CASES if c[2] == 16384)
    n, d, k, p = (set(c[i] for c in PRIV_CASES) for i in range(4))
    assert k == {1, 300, 567, 568, 1117, 1118, 2168} and d == {1, 3, 4, 60, 64, 68, 100, 770, 2052}
    assert n == {1, 63, 64, 65, 8191, 8192, 8193, 20000}

    def ds(kk):
        s = 64
        while s > 16 and kk * (s + 1) * 4 > 144 * 1024:
            s >>= 1
        return s if kk * (s + 1) * 4 <= 144 * 1024 else None
    assert [ds(kk) for kk in (567, 568, 1117, 1118, 2168, 2169)] == [64, 32, 32, 16, 16, None]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", SEG_CASES, ids=_ids(SEG_CASES))
def test_segmented_update(H, case, kind):
    check_case(H, kind, "seg", *case, seed=1000 + SEG_CASES.index(case))


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", PRIV_CASES, ids=_ids(PRIV_CASES))
def test_privatised_update(H, case, kind):
    check_case(H, kind, "priv", *case, seed=2000 + PRIV_CASES.index(case))


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_update_through_python_reaches_the_privatised_form(H, kind):
    """D = 2052 > 2048: the one way production Python (KM.update, which always brings a workspace) runs kmeans_update_kernel."""
    from u2seg_amd.cluster import kmeans as KM

    n, d, k = 8193, 2052, 300
    x = make_x(kind, n, d, 31)
    labels = R.kmeans_labels("uniform", n, k, torch.Generator().manual_seed(31)).to(DEV)
    c, counts = KM.update(x, labels, k)
    KM._ws_cache.pop(str(x.device), None)
    s, cnt, a = R.kmeans_update_ref(x, labels, k)
    same_bits("counts", counts.contiguous(), cnt.float())
    nn = cnt.to(F64)[:, None]
    if kind == "exact":
        same_bits("centroids", c, (s / nn).float())
    else:
        within("centroids", c, s / nn, centroid_bound(cnt, a, s / nn))


# ----------------------------------------------------------------------------------------------------------------------------
# special rows
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("form,n,d,k", [("seg", 4097, 300, 300), ("seg", 8193, 1025, 40), ("priv", 4097, 300, 300), ("priv", 8193, 70, 1118)])
def test_special_rows(H, form, n, d, k, kind):
    """A NaN row, a row with +Inf in one dimension, a cluster whose rows sum to exactly 0 in one dimension (both forms skip the
    atomic of a partial sum that is 0), a cluster of one row of -0.0 (its sum is the +0 the buffer started with): exactly the
    struck cluster's struck dimensions are NaN / Inf, every other element keeps its bound."""
    x = make_x(kind, n, d, 77)
    labels = R.kmeans_labels("uniform", n, k - 1, torch.Generator().manual_seed(77)).to(DEV)     # cluster k - 1: the -0.0 row alone
    i_nan, i_inf, i_neg = 100, n - 3, n // 2
    labels[i_neg] = k - 1
    x[i_neg] = -0.0
    x[i_nan] = float("nan")
    x[i_inf, d // 2] = float("inf")
    j_nan, j_inf = int(labels[i_nan]), int(labels[i_inf])
    j_zero = next(j for j in range(k - 1) if j not in (j_nan, j_inf) and int((labels == j).sum()) >= 3)
    rows = torch.nonzero(labels == j_zero)[:, 0]
    dz = d - 1
    x[rows, dz] = 0.0
    x[rows[0], dz], x[rows[-1], dz] = 3.0, -3.0
    csum, counts = run_update(H, x, labels, k, form)
    s, cnt, a = R.kmeans_update_ref(x, labels, k)
    # the reference itself: what is struck and what is not
    nan_want = torch.zeros((k, d), dtype=torch.bool, device=DEV)
    nan_want[j_nan] = True
    inf_want = torch.zeros_like(nan_want)
    if j_inf != j_nan:
        inf_want[j_inf, d // 2] = True
    assert torch.equal(torch.isnan(s), nan_want) and torch.equal(torch.isinf(s), inf_want)
    assert float(s[j_zero, dz]) == 0.0 and float(a[j_zero, dz]) == 6.0 and int(cnt[k - 1]) == 1
    name = "%s %s special rows" % (form, kind)
    if kind == "exact":
        check_exact(H, name, x, labels, k, csum, counts)
    else:
        check_random(H, name, x, labels, k, csum, counts)
    assert float(csum[j_zero, dz]) == 0.0                                   # +3, -3 and zeros: exact in any order
    assert csum[k - 1].view(torch.int32).abs().max() == 0                    # +0.0 in every dimension, not -0.0
    assert torch.equal(torch.isnan(csum), nan_want) and torch.equal(torch.isinf(csum), inf_want)


# ----------------------------------------------------------------------------------------------------------------------------
# contracts
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n,d,k", [("seg", 8193, 300, 513), ("seg", 4097, 1025, 2), ("priv", 8193, 68, 568), ("priv", 20000, 3, 2168)])
def test_update_accumulates(H, form, n, d, k):
    """csum and counts are added to, never overwritten (update_sharded's partial sums depend on it): two calls on the two halves of
    x into one pair of buffers leave what one call on the whole leaves - bit for bit on exact inputs - which is the reference."""
    x = make_x("exact", n, d, 5)
    labels = R.kmeans_labels("uniform", n, k, torch.Generator().manual_seed(5)).to(DEV)
    whole = run_update(H, x, labels, k, form)
    h = n // 2 + 1
    csum, counts = run_update(H, x[:h].contiguous(), labels[:h].contiguous(), k, form)
    csum, counts = run_update(H, x[h:].contiguous(), labels[h:].contiguous(), k, form, csum, counts)
    same_bits("csum", csum, whole[0])
    same_bits("counts", counts, whole[1])
    check_exact(H, "%s accumulated" % form, x, labels, k, csum, counts)


def test_workspace_is_reused_across_shapes(H):
    """KM.update keeps one workspace per device and hands it to calls with other (N, K) as long as it is large enough: the tables'
    offsets inside it move with N and K, and what an earlier call left there must not matter."""
    from u2seg_amd.cluster import kmeans as KM

    KM._ws_cache.pop(str(torch.device(DEV)), None)
    first = None
    for n, d, k, pattern in ((8193, 64, 800, "uniform"), (4097, 64, 300, "rr"), (257, 300, 16, "sorted"), (8193, 64, 800, "holes")):
        x = make_x("exact", n, d, n + k)
        labels = R.kmeans_labels(pattern, n, k, torch.Generator().manual_seed(n)).to(DEV)
        c, counts = KM.update(x, labels, k)
        ws = KM._ws_cache[str(x.device)]
        first = ws if first is None else first
        assert ws is first                                    # the later, smaller calls ran in the first call's buffer
        s, cnt, _ = R.kmeans_update_ref(x, labels, k)
        same_bits("counts", counts.contiguous(), cnt.float())
        same_bits("centroids", c, (s / cnt.to(F64)[:, None]).float())
        # and the ABI with the same buffer
        csum, counts = run_update(H, x, labels, k, "seg", ws=ws)
        check_exact(H, "reused workspace", x, labels, k, csum, counts)
    KM._ws_cache.pop(str(torch.device(DEV)), None)


@pytest.mark.parametrize("k,d", [(3, 7), (5, 103), (1, 1), (300, 769), (2, 256)])
def test_finalize(H, k, d):
    """c = csum / counts elementwise, K * D not a multiple of the 256 threads of a block: the correctly rounded quotient; count 0
    with sum 0 gives NaN, count 0 with a sum gives the sum's infinity; nothing is written beyond K * D (run_finalize's canary)."""
    g = torch.Generator(device=DEV).manual_seed(k * d)
    csum = torch.randn((k, d), generator=g, device=DEV) * 100
    counts = torch.randint(1, 5000, (k,), generator=g, device=DEV).float()
    counts[0] = 0.0
    half = (d + 1) // 2
    csum[0, :half] = 0.0
    if d > 2:
        csum[0, half], csum[0, d - 1] = 5.0, -5.0
    c = run_finalize(H, csum, counts)
    same_bits("finalize", c, (csum.to(F64) / counts.to(F64)[:, None]).float())
    assert bool(torch.isnan(c[0, :half]).all()) and bool(torch.isinf(c[0, half:]).all()) and bool(torch.isfinite(c[1:]).all())
    if d > 2:
        assert float(c[0, half]) == float("inf") and float(c[0, d - 1]) == float("-inf")


def test_refusals_launch_nothing(H):
    """K beyond what a form serves answers -1 (no launch, nothing written); N = 0 answers 0 and leaves csum / counts alone."""
    d = 16
    x = torch.ones((8, d), device=DEV)
    labels = torch.zeros(8, dtype=torch.int64, device=DEV)

    def status(n, k, ws):
        csum, counts = torch.full((k, d), 7.0, device=DEV), torch.full((k,), 7.0, device=DEV)
        rc = H.call_nostream("u2_kmeans_update", x, labels, csum, counts, n, d, k, ws, H.stream_ptr())
        torch.cuda.synchronize()
        assert bool((csum == 7.0).all()) and bool((counts == 7.0).all())
        return rc

    assert status(8, 2169, None) == -1                        # 2169 * 17 * 4 bytes > 144 KB at the smallest DS
    assert status(8, 16385, workspace(H, 8, d, 16385)) == -1  # the [K] tables no longer fit 64 KB, nor does the privatised form
    assert status(0, 300, None) == 0 and status(0, 300, workspace(H, 8, d, 300)) == 0


@pytest.mark.parametrize("form", ["seg", "priv"])
def test_out_of_range_labels_belong_to_no_cluster(H, form):
    """Labels -1, K, K + 5 and 2^32 + 3 (whose low 32 bits are the valid label 3) among valid ones: sums and counts are those of
    the reference, which leaves such points out, bit for bit on exact inputs.  Both forms test the 64-bit value before any cast."""
    n, d, k = 4097, 68, 300
    x = make_x("exact", n, d, 13)
    labels = R.kmeans_labels("uniform", n, k, torch.Generator().manual_seed(13))
    for i, v in enumerate((-1, k, k + 5, (1 << 32) + 3, -(1 << 32), -(1 << 40) + 7)):
        labels[i::41][: 20] = v
        labels[n - 1 - i] = v
    labels = labels.to(DEV)
    out = int(((labels < 0) | (labels >= k)).sum())
    assert out >= 6 * 20
    csum, counts = run_update(H, x, labels, k, form)
    assert float(counts.sum()) == n - out
    check_exact(H, form + " out-of-range labels", x, labels, k, csum, counts)


# ----------------------------------------------------------------------------------------------------------------------------
# E step on a non-finite centroid
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def mixture(n, d, k, spare=()):
    """Well separated mixture data: centres N(0, 4 I), points centre + N(0, 0.25 I), centroids centre + N(0, 0.09 I); the
    components in `spare` have no points (a point whose own centroid is struck out would sit between two far ones, possibly at a tie)."""
    g = torch.Generator(device=DEV).manual_seed(17 * k + d)
    centers = torch.randn((k, d), generator=g, device=DEV) * 2
    used = torch.tensor([j for j in range(k) if j not in spare], device=DEV)
    x = centers[used[torch.randint(0, used.numel(), (n,), generator=g, device=DEV)]] + 0.5 * torch.randn((n, d), generator=g, device=DEV)
    return x, centers + 0.3 * torch.randn((k, d), generator=g, device=DEV)


def estep_cases(k):
    """name -> (rows set to NaN, rows set to 1e20)"""
    cases = {"one-nan": ([k // 2], []), "two-nan": ([k // 3 + 1, k // 2], []), "nan-first-last": ([0, k - 1], []),
             "far": ([], [k // 2]), "nan-and-far": ([k // 2 + 1], [1])}
    if k > 320:
        cases["nan-second-block"] = ([320 + 80], [])
    return cases


ESTEP = [(n, k, d, name) for n, k in ((5000, 40), (5000, 300), (66003, 641)) for d in (64, 256) for name in estep_cases(k)]


@pytest.mark.parametrize("n,k,d,name", ESTEP, ids=["N%d-K%d-D%d-%s" % e for e in ESTEP])
def test_assign_with_non_finite_centroids(monkeypatch, n, k, d, name):
    """KM.assign on centroids with NaN rows - what an empty cluster leaves behind, exactly as in the reference - and with a finite
    row at 1e20, whose |c|^2 overflows fp32: the exact kernel (exact=True), the two-level screen (K = 40, 300; called twice, the
    second call may run with the first pass switched off) and the blocks path (K = 641 over the 16-bit shadow) give
    kmeans_argmin_ref's label at EVERY point: the lowest NaN index where there is a NaN row (torch.argmin: NaN beats numbers),
    never the far row.  No point is excused: the float64 gap between a point's two nearest finite centroids is at least 1e-3 of
    the nearer distance (asserted on the reference alone), three orders above fp32 rounding of either formulation.
    Centroid rows with +-Inf entries are out of scope: the expanded form |c|^2 - 2 x.c gives Inf - Inf there, and the
    features this runs on are L2-normalised."""
    from u2seg_amd.cluster import kmeans as KM

    monkeypatch.setattr(KM, "SHADOW_MIN_POINTS", 256)
    struck = tuple(sorted(set(sum((a + b for a, b in estep_cases(k).values()), []))))    # the same data for every case of a shape
    x, c0 = mixture(n, d, k, struck)
    nan_rows, far_rows = estep_cases(k)[name]
    c = c0.clone()
    for r in nan_rows:
        c[r] = float("nan")
    for r in far_rows:
        c[r] = 1e20
    ref, gap = R.kmeans_argmin_ref(x, c)
    assert float(gap.min()) >= 1e-3
    if nan_rows:
        assert bool((ref == min(nan_rows)).all())
    else:
        assert not bool((ref == far_rows[0]).any()) and len(set(ref.tolist())) == k - len(struck)
    try:
        got = {"exact": KM.assign(x, c, exact=True)}
        KM._ws_cache.pop("assign:" + str(x.device), None)       # a fresh workspace: the first pass starts switched on
        KM.release_shadow()
        got["screened"] = KM.assign(x, c)
        assert KM.last_recheck_count(x.device) is not None      # it did screen
        got["screened again"] = KM.assign(x, c)
        for path, lab in got.items():
            assert torch.equal(lab, ref), "%s: %d of %d labels differ from the float64 arg-min" % (path, int((lab != ref).sum()), n)
    finally:
        KM.release_shadow()
        KM._ws_cache.pop("assign:" + str(x.device), None)


def test_lloyd_with_an_empty_cluster_follows_the_float64_loop(monkeypatch):
    """x holds a duplicated row and init picks both copies: the tie goes to the first, the second copy's cluster is empty after
    iteration 1 and its centroid a NaN row, which then wins every arg-min (the reference's behaviour, usl-imagenet.py:135).
    KM.kmeans(x, init, 3) == a float64 Lloyd loop of kmeans_argmin_ref and kmeans_update_ref: labels at every point, centroids
    within the M-step bound, NaN rows in the same places."""
    from u2seg_amd.cluster import kmeans as KM

    monkeypatch.setattr(KM, "SHADOW_MIN_POINTS", 256)
    n, d, k = 1000, 64, 9
    x, c0 = mixture(n, d, k - 1)
    x = x.clone()
    x[700] = x[40]
    comp = R.kmeans_argmin_ref(x, c0)[0].tolist()             # one initial centroid per mixture component, and the second copy
    reps = [comp.index(j) for j in range(k - 1) if j != comp[40]]
    init = torch.tensor(reps[:2] + [40] + reps[2:4] + [700] + reps[4:], device=DEV)
    assert init.numel() == k
    try:
        labels, c = KM.kmeans(x, init, 3)
    finally:
        KM.release_shadow()
        KM._ws_cache.pop("assign:" + str(x.device), None)
        KM._ws_cache.pop(str(x.device), None)
    rc = x[init].to(F64)
    nan_rows = []
    for it in range(3):
        rl, gap = R.kmeans_argmin_ref(x, rc)
        if it == 0:
            tied = (rl == 2)
            assert not bool((rl == 5).any()) and bool((gap[tied] == 0).all()) and float(gap[~tied].min()) >= 1e-3
        s, cnt, a = R.kmeans_update_ref(x, rl, k)
        rc = s / cnt.to(F64)[:, None]
        nan_rows.append(torch.isnan(rc).all(1).tolist())
    assert nan_rows[0] == [j == 5 for j in range(k)] and nan_rows[1] == [j != 5 for j in range(k)] and nan_rows[2] == [j != 0 for j in range(k)]
    assert torch.equal(labels, rl)
    within("centroids", c, rc, centroid_bound(cnt, a, rc))
    assert torch.equal(torch.isnan(c), torch.isnan(rc))
