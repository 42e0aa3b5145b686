"""The k-means E step (u2_kmeans_assign_shadow, u2seg_amd/csrc/kmeans.hip) against float64 at its screening margins, at every point
and on every path, and what u2_kmeans_prepare writes for the first pass.  References: tests/float64_refs.py (kmeans_key_bound,
kmeans_decision_ref, kmeans_rule_ok, kmeans_gap_ladder - plain torch in float64, held against a plain fp32 emulation on the CPU by
tests/test_float64_refs_host.py).  Nothing in this module is measured: every bound is derived below or in those docstrings.

The paths and the cases that reach them (KM.assign):
  exact kernel alone    kmeans_assign_kernel over every point: exact=True, or N < 256, or D % 32 != 0, or K = 1 -
                        test_exact_kernel (K = 40 / 300 / 641: one, ten and 10 + 10 + 1 centroid tiles; N = 1, 127, 129, 255; D = 16, 48; K = 1).
  two-level screen      no shadow (N below SHADOW_MIN_POINTS): kmeans_screen_kernel<1> over the leading bf16 pieces (margin 0.02 |x| max|c|),
                        kmeans_screen_kernel<3, true> over three split-bf16 products (margin 1e-4 |x| max|c|) on what it left, the exact
                        kernel over the list that leaves (`rows`); a first pass that leaves more than N / 4 undecided is switched off for
                        the next call, which sends every point to the three-product pass - test_two_level_screen, both calls.
  shadow path, K <= 320 SHADOW_MIN_POINTS patched to 256: kmeans_coarse_kernel over the fp16 shadow of x - mu (per-point margin from the
                        norms u2_kmeans_prepare stored, + 3e-4 |x| max|c|, + the distance bits given up to the index), persistent
                        work-groups (N = 66 003: 258 tiles of 256 points, more than the grid has work-groups), then the three-product pass
                        and the exact kernel - test_shadow_screen.
  blocks path           K in (320, 1280] over the shadow: the coarse pass once per block of 320 centroids, km_chunk_merge_kernel
                        rebuilding best and second best of all from the blocks' candidates, the exact kernel on the rest -
                        test_blocks_path (K = 321, 641: a last block of one centroid; K = 1280: four full blocks).

The decision rule, the same for every path and every point (float64_refs.kmeans_rule_ok; no point is sampled):
  E_i = gamma_(D+3) max_j (|c_j|^2 + 2 |x_i|.|c_j|), gamma_n = n 2^-24 / (1 - n 2^-24), bounds the error of the exact kernel's key
  fl(cn_j - 2 acc_ij) for every j: cn_j is a sum of D rounded squares in some order (gamma_D |c_j|^2), acc_ij an fma chain of length D
  (gamma_D |x_i|.|c_j|, absolute values inside the dot product), one final rounding, two spare (kmeans_key_bound's docstring).
  With the float64 distances d_i(1) <= d_i(2) <= ... of the difference form:
    decidable point    d_(2) - d_(1) > 2 E_i: the label is the float64 arg-min.  A screening pass may only ever decide a point whose
                       computed gap exceeds its margin, which is at least twice its own error: it cannot turn the order round either.
    undecidable point  the label l has d_il <= d_(1) + 2 E_i; where the centroid rows within that band have the same bits, the lowest index.
    NaN row of x       label 0 (torch.argmin on an all-NaN row; km_less).
  Rows of x with +-Inf are out of scope, as centroid rows with +-Inf are in test_gpu_kmeans_update_float64.py.

The inputs (kmeans_gap_ladder): a mixture with chosen centroid pairs 2^-m |c| apart, m in {2, 5, 8, 11}, at the places where two
candidates meet in the arg-min (neighbours, the same lane of neighbouring 16-blocks, across the 32-centroid tiles, the last two,
across the blocks of 320), and points between them whose gap runs down a ladder from 2^-2m |c|^2 to 2^-20 of that, on both sides.
The relative gap, gap / (|x_i| max|c|), is what the margins are proportional to; its bands (2 E_i / (|x_i| max|c|), 1e-4), [1e-4, 3e-3),
[3e-3, 2e-2), >= 2e-2 come from the margin_rel constants of u2_kmeans_assign_shadow: 1e-4 (three products), 3e-4 (the shadow pass,
which adds the dropped norms to it: 3e-3 is ten times it) and 0.02 (leading pieces).  Every band the arithmetic leaves room for
holds at least 32 decidable points and at most 0.4 of the points are undecidable (asserted on the reference before any kernel runs;
at D = 768 the lowest band is empty: 2 E_i alone is 2.8e-4 |x_i| max|c|).  Decidable ladder rows of the narrowest bands sit at rows 0,
127, 128, 255, 256 and N - 1.

u2_kmeans_prepare (test_prepare_writes_what_the_first_pass_reads), offsets from kmeans.hip's host code (km_shadow_words,
u2_kmeans_shadow_floats, u2_kmeans_prepare) in floats from the start of the buffer:
  0                            the shadow: km_shadow_words(N, D) = (D / 32) ceil(N / 256) 4096 floats of fp16 pairs laid out
                               [D / 32 steps][G = 16 ceil(N / 256) groups][64 lanes][8]; lane fg * 16 + fr of group g holds point
                               g * 16 + fr, dimensions step * 32 + fg * 4 + (0 .. 3) and step * 32 + 16 + fg * 4 + (0 .. 3); points >= N zero
  words                        xn[3][NP16], NP16 = 256 ceil(N / 256): |x - mu|, |(x - mu) - shadow / S|, |x|
  words + 3 NP16               mu[(D + 63) & ~63], the column mean of x
  words + 3 NP16 + that        aux = {S, 1 / S, max_p |x_p - mu|^2}, S the power of two that puts the largest |x_p - mu| into [2^13, 2^14)"""
import functools

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
N_STD = R.KM_N_STD       # 2817 = 256 t + 1 = 128 * 22 + 1: a last work-group of one point for the screens and for the exact kernel


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


@pytest.fixture()
def KM(H):
    """u2seg_amd.cluster.kmeans with nothing cached before and after a test: no shadow, no workspace (whose screening state would
    otherwise come from another case)."""
    from u2seg_amd.cluster import kmeans as km

    def drop():
        km.release_shadow()
        km._ws_cache.pop("assign:" + str(torch.device(DEV)), None)

    drop()
    try:
        yield km
    finally:
        drop()


def fresh(H, KM, n, d, k):
    """Before each case: the cached workspace and shadow go, and a ZEROED workspace takes their place - the caching allocator may
    hand a popped workspace's block out again, screening state (first pass switched off) included."""
    KM.release_shadow()
    key = "assign:" + str(torch.device(DEV))
    KM._ws_cache.pop(key, None)
    need = H.call_nostream("u2_kmeans_assign_workspace_floats", n, d, k)
    KM._ws_cache[key] = (torch.zeros(need, dtype=torch.float32, device=DEV), k, None)


@functools.lru_cache(maxsize=None)
def ladder(k, d, n, offset):
    """One ladder and one float64 reference per shape, shared by every path's test and never written to."""
    x, c, ref, is_lad = R.kmeans_gap_ladder(k, d, n, offset, device=DEV)
    if n >= 2048 and k >= 2:
        R.kmeans_check_ladder(ref, n, d)                          # the conditions on the reference alone, before any kernel runs
    return x, c, ref


def check(path, x, c, labels, ref):
    assert labels.dtype == torch.int64 and labels.shape == (x.shape[0],)
    msg = R.kmeans_rule_report(path, x, c, labels, ref)
    assert msg is None, msg


def ids(cases):
    return ["K%d-D%d-N%d-off%d" % (k, d, n, off) for k, d, n, off in cases]


# ----------------------------------------------------------------------------------------------------------------------------
# the exact kernel alone
# ----------------------------------------------------------------------------------------------------------------------------
EXACT = R.KM_EXACT_CASES      # the case lists are in float64_refs.py, where the CPU twin checks every one's inputs


@pytest.mark.parametrize("k,d,n,off", EXACT, ids=ids(EXACT))
def test_exact_kernel(H, KM, k, d, n, off):
    """exact=True: kmeans_assign_kernel over every point.  One centroid tile (K = 40), ten (300: the branch-free pass), two full
    passes and a tile of one centroid (641); N = 255, 1, 127, 129: below the screens, a lone point, one short and one past a
    work-group; D = 48, 16: no multiple of 32, which the default call sends here as well (asserted); K = 1."""
    x, c, ref = ladder(k, d, n, off)
    fresh(H, KM, n, d, k)
    check("exact", x, c, KM.assign(x, c, exact=True), ref)
    assert KM.last_recheck_count(x.device) is None
    if n < 256 or d % 32 or k < 2:
        check("default call, unscreened", x, c, KM.assign(x, c), ref)
        assert KM.last_recheck_count(x.device) is None          # it did not screen


# ----------------------------------------------------------------------------------------------------------------------------
# the two-level screen without a shadow
# ----------------------------------------------------------------------------------------------------------------------------
TWO_LEVEL = R.KM_TWO_LEVEL_CASES


@pytest.mark.parametrize("k,d,n,off", TWO_LEVEL, ids=ids(TWO_LEVEL))
def test_two_level_screen(H, KM, k, d, n, off):
    """N below SHADOW_MIN_POINTS: leading-piece pass, three-product pass, exact kernel over the list - twice.  The first call runs
    the first pass (a fresh workspace); where it left more than N / 4 undecided the second call runs without it and reads 0,
    otherwise the second call repeats the first.  K = 17, D = 768 at offset 25 is a case of the first kind (every pair of centroids
    is closer than the first pass's margin there); N = 6145 at K = 40 one of the second kind with the pass at work; at K = 300,
    D = 256 more than 128 points are on the exact kernel's list: two work-groups of it."""
    assert n < KM.SHADOW_MIN_POINTS
    x, c, ref = ladder(k, d, n, off)
    fresh(H, KM, n, d, k)
    first = KM.assign(x, c)
    und1, re1 = KM.last_coarse_undecided(x.device), KM.last_recheck_count(x.device)
    assert KM._shadow(x) is None and re1 is not None and 0 <= re1 <= und1 <= n, (und1, re1)
    second = KM.assign(x, c)
    und2, re2 = KM.last_coarse_undecided(x.device), KM.last_recheck_count(x.device)
    print("two-level K=%d D=%d N=%d off=%d: first pass left %d then %d, exact list %d then %d" % (k, d, n, off, und1, und2, re1, re2))
    check("two-level, first call (first pass on, left %d, exact list %d)" % (und1, re1), x, c, first, ref)
    check("two-level, second call (first pass %s, exact list %d)" % ("off" if und1 > n // 4 else "on", re2), x, c, second, ref)
    if und1 > n // 4:
        assert und2 == 0, (und1, und2)                           # switched off
    else:
        assert und2 == und1, (und1, und2)                        # ran again, on the same inputs
    if (k, d, off) == (17, 768, 25.0):
        assert und1 > n // 4, und1
    if (k, d, n) == (300, 256, N_STD):
        assert re1 >= 129 and re2 >= 129, (re1, re2)
    if n == 24 * 256 + 1:
        assert 0 < und1 <= n // 4, und1


# ----------------------------------------------------------------------------------------------------------------------------
# the first pass over the shadow
# ----------------------------------------------------------------------------------------------------------------------------
SHADOW = R.KM_SHADOW_CASES


@pytest.mark.parametrize("k,d,n,off", SHADOW, ids=ids(SHADOW))
def test_shadow_screen(H, KM, monkeypatch, k, d, n, off):
    """K <= 320 over the fp16 shadow of x - mu (kmeans_coarse_kernel), twice; N = 66 003: 258 tiles for the persistent grid."""
    monkeypatch.setattr(KM, "SHADOW_MIN_POINTS", 256)
    x, c, ref = ladder(k, d, n, off)
    fresh(H, KM, n, d, k)
    first = KM.assign(x, c)
    und1, re1 = KM.last_coarse_undecided(x.device), KM.last_recheck_count(x.device)
    assert KM._shadow_cache and KM._shadow(x) is not None and re1 is not None and 0 <= re1 <= und1 <= n, (und1, re1)
    second = KM.assign(x, c)
    und2, re2 = KM.last_coarse_undecided(x.device), KM.last_recheck_count(x.device)
    print("shadow K=%d D=%d N=%d off=%d: first pass left %d then %d, exact list %d then %d" % (k, d, n, off, und1, und2, re1, re2))
    check("shadow, first call (first pass left %d, exact list %d)" % (und1, re1), x, c, first, ref)
    check("shadow, second call (first pass left %d, exact list %d)" % (und2, re2), x, c, second, ref)
    assert und2 == (0 if und1 > n * 55 // 100 else und1), (und1, und2)


BLOCKS = R.KM_BLOCKS_CASES


@pytest.mark.parametrize("k,d,n,off", BLOCKS, ids=ids(BLOCKS))
def test_blocks_path(H, KM, monkeypatch, k, d, n, off):
    """K > 320 over the shadow: the pairs (319, 320), (5, 325), (K - 2, K - 1) and, at K = 641, (7, 640) lie across the blocks whose
    candidates km_chunk_merge_kernel merges; some points but not all go on to the exact kernel."""
    monkeypatch.setattr(KM, "SHADOW_MIN_POINTS", 256)
    x, c, ref = ladder(k, d, n, off)
    fresh(H, KM, n, d, k)
    got = KM.assign(x, c)
    re1 = KM.last_recheck_count(x.device)
    assert KM._ws_cache["assign:" + str(x.device)][2] == "blocks" and KM._shadow(x) is not None
    print("blocks K=%d D=%d N=%d off=%d: exact list %d" % (k, d, n, off, re1))
    check("blocks (exact list %d)" % re1, x, c, got, ref)
    assert 0 < re1 < n, re1
    check("blocks, second call", x, c, KM.assign(x, c), ref)


# ----------------------------------------------------------------------------------------------------------------------------
# scale and NaN rows, on every path
# ----------------------------------------------------------------------------------------------------------------------------
def every_path(H, KM, monkeypatch, x, c):
    """name -> labels of the exact kernel, the two-level screen (both calls) and the first pass over the shadow (K <= 320: both calls;
    K > 320: the blocks path)."""
    n, d = x.shape
    k = c.shape[0]
    got = {}
    fresh(H, KM, n, d, k)
    got["exact"] = KM.assign(x, c, exact=True)
    if k <= 320:
        got["two-level"] = KM.assign(x, c)
        got["two-level again"] = KM.assign(x, c)
        assert KM._shadow(x) is None
    monkeypatch.setattr(KM, "SHADOW_MIN_POINTS", 256)
    fresh(H, KM, n, d, k)
    got["shadow"] = KM.assign(x, c)
    assert KM._shadow(x) is not None and KM.last_recheck_count(x.device) is not None
    got["shadow again"] = KM.assign(x, c)
    return got


@pytest.mark.parametrize("power", [-40, 40])
def test_scale(H, KM, monkeypatch, power):
    """x and c times 2^-40 and 2^40: the rule holds on every path (every quantity of it scales by 2^(2 power) exactly), and the exact
    kernel, all of whose fp32 operations scale exactly, returns the labels of the unscaled case."""
    x, c, _ = ladder(40, 64, N_STD, 0.0)
    xs, cs = x * 2.0 ** power, c * 2.0 ** power
    assert torch.equal(xs * 2.0 ** -power, x) and torch.equal(cs * 2.0 ** -power, c)
    ref = R.kmeans_decision_ref(xs, cs)
    for path, lab in every_path(H, KM, monkeypatch, xs, cs).items():
        check("%s, inputs x 2^%d" % (path, power), xs, cs, lab, ref)
        if path == "exact":
            fresh(H, KM, x.shape[0], 64, 40)
            assert torch.equal(lab, KM.assign(x, c, exact=True)), "the exact kernel's labels change with a power-of-two scale"


@pytest.mark.parametrize("k,d", [(40, 64), (641, 64)])
def test_nan_rows_of_x(H, KM, monkeypatch, k, d):
    """Rows 0, 300 and N - 1 of x hold a NaN (one element, the whole row, the last element): label 0 on every path, the rule at every
    other row, and - the exact kernel - the very labels of the run without them there."""
    x0, c, _ = ladder(k, d, N_STD, 0.0)
    x = x0.clone()
    x[0, 3] = float("nan")
    x[300] = float("nan")
    x[N_STD - 1, d - 1] = float("nan")
    ref = R.kmeans_decision_ref(x, c)
    assert ref["nan"].nonzero()[:, 0].tolist() == [0, 300, N_STD - 1]
    for path, lab in every_path(H, KM, monkeypatch, x, c).items():
        assert lab[[0, 300, N_STD - 1]].tolist() == [0, 0, 0], (path, lab[[0, 300, N_STD - 1]].tolist())
        check(path + ", three NaN rows", x, c, lab, ref)
        if path == "exact":
            fresh(H, KM, N_STD, d, k)
            same = KM.assign(x0, c, exact=True) == lab
            assert bool(same[~ref["nan"]].all()), "NaN rows changed the labels of other rows"


# ----------------------------------------------------------------------------------------------------------------------------
# u2_kmeans_prepare
# ----------------------------------------------------------------------------------------------------------------------------
PREPARE = [(n, d, off) for n in (256, 257, 1000) for d in (32, 64, 768) for off in (0.0, 25.0)]


@pytest.mark.parametrize("n,d,off", PREPARE, ids=["N%d-D%d-off%d" % p for p in PREPARE])
def test_prepare_writes_what_the_first_pass_reads(H, n, d, off):
    """u2_kmeans_prepare through the C ABI on rows whose norms (about the offset) spread over six decades, one zero row among them:
      mu      |mu - mean| <= gamma_N mean|x| + 2^-24 |mean| per column (a sum of N terms in some order, one division);
      S       a power of two, S max_p |fl32(x_p - mu)| in [2^13, 2^14), aux[1] S == 1;
      shadow  decoded through the lane order of the module docstring == fp16(S fl32(x - mu)) bit for bit, formed in fp32 from the mu
              and S read back (the scaling by a power of two is exact); rows >= N are zero;
      norms   |x - mu|, |(x - mu) - shadow / S| and |x| within gamma_(D+4) relative of the float64 norms of the same fp32 vectors
              (D rounded squares, their sum, a square root; the dropped part v - h / S is an fp32 number, its subtraction exact) -
              the dropped part's in particular not below (1 - gamma_(D+4)) of it: the first pass's margin has only the factor
              4.04 / 4 over Cauchy-Schwarz; padding rows are zero;
    and nothing is written behind u2_kmeans_shadow_floats(N, D)."""
    g = torch.Generator().manual_seed(n * 1000 + d + int(off))
    x = torch.randn((n, d), generator=g, dtype=F64) * 10.0 ** (6 * torch.rand((n, 1), generator=g, dtype=F64) - 3)
    x[n // 3] = 0
    x = (x + off).float().to(DEV)
    floats = H.call_nostream("u2_kmeans_shadow_floats", n, d)
    tiles = -(-n // 256)
    words, np16, dpad = (d // 32) * tiles * 4096, 256 * tiles, (d + 63) & ~63
    assert floats == words + 3 * np16 + dpad + 64
    canary = 1024
    buf = torch.full((floats + canary,), -7.0, device=DEV)
    H.call("u2_kmeans_prepare", x, buf, n, d)
    assert bool((buf[floats:] == -7.0).all()), "u2_kmeans_prepare wrote beyond u2_kmeans_shadow_floats"
    xn = buf[words: words + 3 * np16].view(3, np16)
    mu = buf[words + 3 * np16: words + 3 * np16 + d]
    aux = buf[words + 3 * np16 + dpad: words + 3 * np16 + dpad + 3]
    x64 = x.to(F64)
    # mu
    mean, mean_abs = x64.mean(0), x64.abs().mean(0)
    err = (mu.to(F64) - mean).abs()
    bound = float(R.gamma32(n)) * mean_abs + R.U24 * mean.abs()
    assert bool((err <= bound).all()), "mu: column %d off by %.3e, bound %.3e" % (int((err - bound).argmax()), float(err.max()), float(bound.max()))
    # S
    s, s_inv = float(aux[0]), float(aux[1])
    y = x - mu[None, :]                                           # fl32(x - mu), as the kernels form it
    ynorm = y.to(F64).norm(dim=1)
    assert s > 0 and torch.frexp(torch.tensor(s))[0].item() == 0.5 and s * s_inv == 1.0, (s, s_inv)
    assert 2.0 ** 13 <= s * float(ynorm.max()) < 2.0 ** 14, (s, float(ynorm.max()))
    assert abs(float(aux[2]) - float(ynorm.max()) ** 2) <= float(R.gamma32(d + 4)) * float(ynorm.max()) ** 2
    # the shadow
    sh = buf[:words].view(torch.float16).view(d // 32, 16 * tiles, 4, 16, 2, 4)     # [step][group][fg][fr][half][e]
    sh = sh.permute(1, 3, 0, 4, 2, 5).reshape(np16, d)                               # point g * 16 + fr, dim step * 32 + half * 16 + fg * 4 + e
    want = (y * s).to(torch.float16)
    bad = sh[:n].contiguous().view(torch.int16) != want.view(torch.int16)
    assert not bool(bad.any()), "shadow: %d of %d elements differ; first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), sh[:n][bad][0].item(), want[bad][0].item())
    assert not bool(sh[n:].contiguous().view(torch.int16).any()), "shadow rows >= N are not zero"
    # the norms
    dropped = y.to(F64) - sh[:n].to(F64) / s
    assert torch.equal(dropped.float().to(F64), dropped)          # an fp32 number: the kernel's subtraction is exact
    rel = float(R.gamma32(d + 4))
    for name, got, ref in (("|x - mu|", xn[0], ynorm), ("|(x - mu) - shadow / S|", xn[1], dropped.norm(dim=1)), ("|x|", xn[2], x64.norm(dim=1))):
        e = (got[:n].to(F64) - ref).abs()
        assert bool((e <= rel * ref).all()), "%s: row %d: got %.9e, float64 %.9e, bound %.3e relative" % (
            name, int((e - rel * ref).argmax()), float(got[int((e - rel * ref).argmax())]), float(ref[int((e - rel * ref).argmax())]), rel)
        assert not bool(got[n:].any()), name + ": padding rows are not zero"
    low = xn[1, :n].to(F64) - (1 - rel) * dropped.norm(dim=1)
    assert bool((low >= 0).all()), "the dropped part's norm is too small at row %d by %.3e" % (int(low.argmin()), float(-low.min()))
