"""u2_usl_regularizer (u2seg_amd/csrc/usl.hip: the long-list instantiation knn_select_kernel<68, 8> of knn_select.h + usl_refine_kernel)
against float64 on every row, through the C ABI: a workspace of exactly u2_usl_reg_workspace_ints words with every byte 0xFF, reg_out
and zero_count followed by canary words that must survive.

The reference, the per-row bound and the rows it holds for are float64_refs.usl_reg_ref (its docstring derives them: the
difference-form bound gamma_(D+2) on each distance, one rounding per reciprocal, square root or product, gamma_H for the sum, three
roundings for the blend; a row is checked when the H + 4 candidates provably contain the true top H - knn_decidable with H for K -
and, with the same-cluster mask, when fp32 cannot move the masked position across the H-th place).  Two kinds of input per case:
  random   clustered rows; NO row may be unchecked, asserted on the reference before reg_out is read;
  lattice  integer coordinates in [-8, 8] with exactly zero column sums (float64_refs.lattice_rows): keys and distances are exact,
           the kernel's lists are the stable float64 lists, every row is checked, and only the reciprocal, the sum and the blend
           round (the bound with g = 0).
The grid: H at 1, 63 and the capacity 64 (68 candidates: the second slot of the refine kernel's lanes); S at H (fewer selected rows
than candidate slots), either side of the 256-row pass and two passes + 1; N around the 128 rows of a work-group; D at the
pipeline's prologue only (16), its first steady-state iteration (48) and 768; both masks; alpha 0.5, 1, 2."""
import ctypes

import pytest
import torch

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
CANARY = -12345.0
CANARY_I = -777
TAIL = 1024

US_H = [1, 63, 64]
US_S = ["H", 255, 256, 257, 513]
US_N = [1, 127, 129, 300]
US_D = [16, 48, 768]
US_ALPHA = [0.5, 1, 2]

# every (H, S) pair twice, the other parameters walking through their lists at different paces
CASES = [(h, s, US_N[(5 * hi + si + 2 * p) % 4], US_D[(hi + si + p) % 3], bool((hi + si + p) % 2), US_ALPHA[(2 * hi + si + 2 * p) % 3])
         for p in range(2) for hi, h in enumerate(US_H) for si, s in enumerate(US_S)]


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def test_the_grid_covers_what_it_claims():
    assert len(set(CASES)) == len(CASES) == 30
    for i, values in enumerate((US_H, US_S, US_N, US_D, [False, True], US_ALPHA)):
        assert {c[i] for c in CASES} == set(values)
    assert {(c[0], c[1]) for c in CASES} == {(h, s) for h in US_H for s in US_S}
    for h in US_H:
        mine = [c for c in CASES if c[0] == h]
        assert {c[3] for c in mine} == set(US_D) and {c[4] for c in mine} == {False, True} and {c[5] for c in mine} == set(US_ALPHA)
    for d in US_D:
        assert {c[5] for c in CASES if c[3] == d} == set(US_ALPHA) and {c[4] for c in CASES if c[3] == d} == {False, True}


def call_usl(H, x, y, labels, reg_in, h, alpha, m, omm, exclude, ws="exact", n=None, s=None, d=None):
    """u2_usl_regularizer through the C ABI -> (status, reg_out [N], zero_count); the canaries behind both must survive."""
    n = x.shape[0] if n is None else n
    s = y.shape[0] if s is None else s
    d = x.shape[1] if d is None else d
    if isinstance(ws, str):
        words = ctypes.c_longlong(-1)
        assert H.call_nostream("u2_usl_reg_workspace_ints", n, s, d, h, ctypes.addressof(words)) == 0
        ws = torch.full((words.value,), -1, dtype=torch.int32, device=DEV)                 # every byte 0xFF
    out = torch.full((max(n, 0) + TAIL,), CANARY, dtype=torch.float32, device=DEV)
    zc = torch.full((1 + TAIL,), CANARY_I, dtype=torch.int32, device=DEV)
    zc[0] = 0
    rc = H.call_nostream("u2_usl_regularizer", x, y, labels, reg_in, out, zc, ws, n, s, d, h, float(alpha), m, omm,
                         1 if exclude else 0, H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out[max(n, 0):] == CANARY).all()) and bool((zc[1:] == CANARY_I).all()), "u2_usl_regularizer wrote beyond its outputs"
    return rc, out[: max(n, 0)], int(zc[0])


def make_case(kind, n, s, d, exclude, seed):
    """(x [N, D], selected rows [S, D], labels [N], reg_in [N]) on the device.  Row 1 of x (where there is one) is a copy of selected
    row 0 with label 0: its zero distance is masked in either mode.  The other labels are drawn from [0, S + 3): some are no
    position at all.  No other zero distance exists (a lattice's zero rows, the last of an odd N and of an odd S, meet under the
    label S - 1)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "lattice":
        x, y = R.lattice_rows(n, d, g), R.lattice_rows(s, d, g)
    else:
        centers = torch.randn((7, d), generator=g)
        pool = centers[torch.randint(0, 7, (n + s,), generator=g)] + 0.6 * torch.randn((n + s, d), generator=g)
        x, y = pool[:n].contiguous(), pool[n:].contiguous()
    labels = torch.randint(0, s + 3, (n,), generator=g)
    if kind == "lattice":
        if n % 2 and s % 2:
            labels[n - 1] = s - 1
        if n > 2:
            x[0], x[1], labels[0], labels[1] = -y[0], y[0], 1 if s > 1 else 0, 0     # in place of a +- pair: the column sums stay 0
        R.assert_lattice(y, x)
        R.assert_lattice(x, y)
    elif n > 1:
        x[1], labels[1] = y[0], 0
    reg_in = torch.rand(n, generator=g) * 3
    return x.to(DEV), y.to(DEV), labels.to(DEV), reg_in.to(DEV)


@pytest.mark.parametrize("kind", ["random", "lattice"])
@pytest.mark.parametrize("h,s_spec,n,d,exclude,alpha", CASES, ids=["H%d-S%s-N%d-D%d-x%d-a%s" % c for c in CASES])
def test_regularizer_against_float64(H, h, s_spec, n, d, exclude, alpha, kind):
    s = h if s_spec == "H" else s_spec
    i = CASES.index((h, s_spec, n, d, exclude, alpha))
    x, y, labels, reg_in = make_case(kind, n, s, d, exclude, 100 + i)
    m = R.fp32_value(0.3) if i % 3 else 0.0
    omm = R.fp32_value(1 - m)
    if not m:
        reg_in = torch.zeros_like(reg_in)
    ref = R.usl_reg_ref(x, y, labels, reg_in, h, alpha, m, omm, exclude, exact=kind == "lattice")
    want, bound, checked, alt = ref
    assert int((~checked).sum()) == 0 and not bool(alt[2].any()), "%d of %d rows are unchecked: the case does not test what it is there for" % (int((~checked).sum()), n)
    rc, got, zeros = call_usl(H, x, y, labels, reg_in, h, alpha, m, omm, exclude)
    assert rc == 0 and zeros == 0
    over = ~R.usl_reg_within(got, ref)
    assert not bool(over.any()), "%d of %d rows beyond their bound; first %d: got %r, want %r, bound %.3g" % (
        int(over.sum()), n, int(over.nonzero()[0]), got[over][0].item(), want[over][0].item(), float(bound[over][0]))


def test_unmasked_zero_distances_are_counted_and_refusals_write_nothing(H):
    """exclude_same_cluster with copies of selected rows under other labels: zero_count is the number of such rows (the reference's
    AssertionError).  H outside [1, 64], D that is no multiple of 16, S < H, no workspace: the status, and neither
    output is written; N = 0 answers 0."""
    x, y, labels, reg_in = make_case("random", 300, 257, 48, True, 7)
    for r in (5, 127, 128, 299):
        x[r] = y[r % 7 + 1]
        labels[r] = r % 7 + 2
    rc, _, zeros = call_usl(H, x, y, labels, reg_in, 20, 1, 0.0, 1.0, True)
    assert rc == 0 and zeros == 4
    ws = torch.full((1 << 17,), -1, dtype=torch.int32, device=DEV)

    def status(n, s, d, h, w=ws):
        rc, out, zeros = call_usl(H, x, y, labels, reg_in, h, 1, 0.0, 1.0, False, ws=w, n=n, s=s, d=d)
        assert bool((out == CANARY).all()) and zeros == 0 and (w is None or bool((w == -1).all()))
        return rc

    assert status(300, 257, 48, 0) == -1 and status(300, 257, 48, 65) == -1
    assert status(300, 257, 8, 20) == -1 and status(300, 257, 24, 20) == -1
    assert status(300, 19, 48, 20) == -2 and status(300, 63, 16, 64) == -2
    assert status(300, 257, 48, 20, None) == -1
    assert status(0, 257, 48, 20) == 0
    n = ctypes.c_longlong(-1)
    for h in (0, 65):
        assert H.call_nostream("u2_usl_reg_workspace_ints", 300, 257, 48, h, ctypes.addressof(n)) == -1 and n.value == -1
