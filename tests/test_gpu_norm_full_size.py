"""Normalisation kernels (u2seg_amd/csrc/norm.hip, the stem tail of pool_resize.hip) at the training shapes (batch 16,
800 x 1344 canvas) against a float64 reference computed on the GPU with plain torch ops.

At these sizes the kernels take paths the small parity tests never reach: non-temporal accesses (tensors > NT_BYTES = 160 MB),
the grid-stride loops of the apply passes (fast_grid caps them at 4096 work-groups), row blocks of thousands of rows in the
column reductions, the finalize folded into the apply passes with hundreds of work-groups, and every backward mask mode.

Inputs come from a seeded device generator, rounded to bf16; both sides see the same bf16 values.  The reference rounds where
the reference model rounds under autocast (the norm output is a bf16 tensor before the residual add, the sum is bf16 before
the ReLU, gradients arriving on several handles are summed into a bf16 tensor), and uses the closed-form float64 BN / GN
gradients.  The ReLU mask of the backward reference is the kernel's own forward output (`out > 0`): the forward check has
already bounded that output, and the reference model's ReLU backward reads its own output the same way.

Tolerances are derived from the kernels' fp32 arithmetic (u = 2^-24, fp contraction off), element by element:
    |got - bf16(ref)| <= e + step(|ref| + e)
where e bounds the fp32 error of the value before its last rounding and step(v) is one bf16 step at magnitude v (both
roundings, the kernel's and the reference's, are at most half a step each).  Every checked tensor must also meet the
max-normalised bound of the small tests (`rel_err` < 4e-3 activations, 5e-3 input gradients, 1e-4 parameter gradients).
Float64 work is done in pieces of CHUNK elements, so the module stays within a few GB of device memory.
"""
import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -24          # fp32 unit roundoff
CHUNK = 1 << 24         # elements per float64 piece (128 MB)
EPS = 1e-5
MOM = 0.1


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()  # fails loudly if libu2seg_hip.so is absent
    return functional


@pytest.fixture(scope="module")
def H():
    from u2seg_amd import _hip

    return _hip


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn_bf(shape, g):
    return torch.randn(shape, generator=g, device=DEV, dtype=BF16)


def step(v):
    """One bf16 step at magnitude v >= 0 (float64): 2^(e - 8) for v in [2^(e-1), 2^e); 0 at v = 0."""
    _, e = torch.frexp(v)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 8), torch.zeros_like(v))


def rnd(v):
    """float64 -> the bf16 value as float64 (the reference's rounding to a bf16 tensor)."""
    return v.to(BF16).to(F64)


def reduce_depth(slots, rows, c):
    """Longest chain of fp32 additions in u2_colstats / u2_norm_bwd_reduce (colreduce_kernel): a thread's running sum over
    its rows of the block, the LDS sum over the block's row lanes, then one atomicAdd per block - the launch geometry of the
    two launchers (per_slot clamped to 8 ... 512 blocks, at least 64 rows per block).  Recursive summation over a chain of
    length d errs by at most d u sum|terms| (Higham, gamma_d)."""
    per_slot = min(512, max(8, 2048 // slots))
    rpb = max(64, -(-rows // per_slot))
    blocks = -(-rows // rpb)
    rows_par = 256 // min(256, c // 8)
    return -(-rpb // rows_par) + rows_par + blocks


def stem_depth(b, h, w, c):
    """The same for u2_affine_relu_maxpool_bwd_reduce (stem_tail_bwd_grid: a thread walks 2 x 2 pixel blocks)."""
    hb, wb, cpr = (h + 1) // 2, (w + 1) // 2, c // 8
    gx = -(-wb * cpr // 256)
    gy = min(max(1, 4096 // gx), b * hb)
    per_thread = -(-b * hb // gy) * -(-wb * cpr // (gx * 256)) * 4
    return per_thread + 256 // cpr + gx * gy


class Check:
    """Accumulates one element-wise comparison over the pieces of a tensor and reports the worst element."""

    def __init__(self, name, old_bound):
        self.name, self.old_bound = name, old_bound
        self.bad, self.n, self.worst, self.max_err, self.max_ref, self.info = 0, 0, 0.0, 0.0, 0.0, ""

    def add(self, got, ref, e):
        """got: the kernel's bf16 values; ref: the float64 value before the last rounding; e: bound of the kernel's fp32 error
        before that rounding."""
        got = got.detach().to(F64)
        err = (got - rnd(ref)).abs()
        tol = e + step(ref.abs() + e)
        self._count(got, ref, (err > tol) | err.isnan(), err / (tol + 1e-300), tol)   # NaN: never within a bound

    def add_interval(self, got, lo, hi, ref):
        """got must lie in [lo, hi]: the reference chain (monotone in its input: roundings, sums with a fixed addend, ReLU)
        evaluated at the two ends of the interval the kernel's fp32 value is known to lie in.  This is the one-step bound made
        exact: it allows a second step only where the interval straddles a rounding midpoint of an intermediate bf16 tensor."""
        got = got.detach().to(F64)
        dist = torch.maximum(lo - got, got - hi).clamp_min(0)
        self._count(got, ref, (dist > 0) | got.isnan(), dist, hi - lo)

    def _count(self, got, ref, bad, ratio, tol):
        self.bad += int(bad.sum())
        self.n += got.numel()
        i = int(ratio.argmax())
        if float(ratio.reshape(-1)[i]) > self.worst:
            self.worst = float(ratio.reshape(-1)[i])
            self.info = "got %r ref %r tol %r" % (float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(tol.reshape(-1)[i]))
        self.max_err = max(self.max_err, float((got - ref).abs().max()))
        self.max_ref = max(self.max_ref, float(ref.abs().max()))

    def done(self):
        assert self.bad == 0, "%s: %d of %d elements beyond the derived bound (worst %.3g x the bound: %s)" % (
            self.name, self.bad, self.n, self.worst, self.info)
        # the small tests' max-normalised bound holds as well: the per-element bound is never the looser one
        if self.old_bound is not None:
            assert self.max_err <= self.old_bound * (self.max_ref + 1e-12), (self.name, self.max_err, self.max_ref)


def check_vec(name, got, ref, bound, old_bound=None):
    """fp32 per-channel results (statistics, parameter gradients) against float64 with a derived bound per entry."""
    got = got.detach().to(F64).reshape(-1)
    ref, bound = ref.reshape(-1), bound.reshape(-1)
    err = (got - ref).abs()
    i = int((err / (bound + 1e-300)).argmax())
    assert bool((err <= bound).all()), "%s[%d]: got %r ref %r bound %r" % (name, i, float(got[i]), float(ref[i]), float(bound[i]))
    if old_bound is not None:
        assert float(err.max()) <= old_bound * float(ref.abs().max()), (name, float(err.max()), float(ref.abs().max()))


def pieces(slots, rows, c):
    """(slot, row slice) pairs covering a [slots, rows, c] tensor in pieces of about CHUNK elements."""
    rc = max(1, CHUNK // c)
    for s in range(slots):
        for r0 in range(0, rows, rc):
            yield s, slice(r0, min(rows, r0 + rc))


# -------------------------------------------------------------------------------------------------
# the float64 reference of a normalisation over [S][R][C] (BN: S = 1; GN: S = images, groups of cg channels)
class NormRef:
    def __init__(self, x3, gamma, beta, cg, sum_gamma):
        """sum_gamma: relative error bound of the fp32 column sums the kernel's finalize starts from (BN: the sums are handed
        over as fp32 values, one rounding: u; GN: u2_colstats' chains plus the cg-channel group sum)."""
        S, R, C = x3.shape
        self.x3, self.S, self.R, self.C, self.cg = x3, S, R, C, cg
        s1, s2, sa = (torch.zeros((S, C), dtype=F64, device=DEV) for _ in range(3))
        for s, rs in pieces(S, R, C):
            xc = x3[s, rs].to(F64)
            s1[s] += xc.sum(0)
            s2[s] += (xc * xc).sum(0)
            sa[s] += xc.abs().sum(0)
        self.col_s1, self.col_s2, self.col_sa = s1, s2, sa
        G = C // cg
        grp = lambda t: t.view(S, G, cg).sum(2).repeat_interleave(cg, 1)  # noqa: E731
        n = float(R * cg)
        self.n = n
        mu, e2, a = grp(s1) / n, grp(s2) / n, grp(sa) / n
        self.mu = mu
        self.var = (e2 - mu * mu).clamp_min(0)
        self.is_ = 1.0 / torch.sqrt(self.var + EPS)
        # fp32 finalize (bn_fwd_coeffs / gn_finalize_fwd_kernel): mu = s1 / n, var = s2 / n - mu^2, is = rsqrtf(var + eps)
        #   mu:   the sum's error sum_gamma * sum|x| / n, the division u|mu| (+ u for the rounding of the sum): e_mu
        #   var:  s2 / n errs by (sum_gamma + u) E[x^2] + u E[x^2]; mu^2 by 2|mu| e_mu + u mu^2 (twice for the product's
        #         inputs); the subtraction by u var: e_var.  This is where E[x^2] - mu^2 cancels: e_var / var ~ mu^2 / var.
        #   is:   half the relative error of var + eps, plus the rounding of the sum and rsqrtf's ulp (4 u): delta
        self.e_mu = sum_gamma * a + 2 * U * mu.abs()
        self.e_var = (sum_gamma + 2 * U) * e2 + 2 * mu.abs() * self.e_mu + 3 * U * mu * mu + U * self.var
        self.delta = self.e_var / (2 * (self.var + EPS)) + 4 * U
        # the kernel's invstd is at most that far off, and never above eps^-1/2 (var is clamped at 0)
        self.is_hi = torch.minimum(self.is_ * (1 + self.delta), torch.full_like(self.is_, EPS ** -0.5))
        self.g = gamma.detach().to(F64).view(1, C).expand(S, C)
        self.b = beta.detach().to(F64).view(1, C).expand(S, C)

    def y(self, s, rs):
        """normalised piece (float64) and the bound of the kernel's fp32 error on it.
        kernel: f = x * sc + sh, sc = g * is_k, sh = b - mu_k * g * is_k, i.e. f = (x - mu_k) g is_k + b + roundings:
            f - y = g [(x - mu)(is_k - is) + (mu - mu_k) is_k]  ->  |g| (|xhat| delta + e_mu is_hi)
            roundings: at most three on each of x sc, mu g is, b, and the sum  ->  3 u (|x| + |mu|) |g| is_hi + 3 u |b|
        x 2 for the second-order terms the first-order bound leaves out."""
        xc = self.x3[s, rs].to(F64)
        xh = (xc - self.mu[s]) * self.is_[s]
        g, b, ih = self.g[s], self.b[s], self.is_hi[s]
        y = xh * g + b
        e = g.abs() * (xh.abs() * self.delta[s] + self.e_mu[s] * ih) + 3 * U * ((xc.abs() + self.mu[s].abs()) * g.abs() * ih + b.abs())
        return xc, xh, y, 2 * e


def bn_inputs(shape, seed, const_value=0.3):
    """x [B, H, W, C] bf16 with channel families: mean 0 / 4 sigma / 16 sigma (the E[x^2] - mu^2 finalize cancels), all-zero
    channels (dead ReLU, padding) and one constant non-zero channel (var = 0: the result rests on eps and on the fp32 sums);
    gamma with negative entries, beta, running statistics that do not start at 0 / 1.
    The constant channel characterises a bound inherent to the sums-based interface: the fp32 finalize's
    E[x^2] - mu^2 errs by ~10 u c^2 against eps, so invstd, and with it the channel's input gradient, is good to e_var / 2 eps
    (c = 0.3: ~3e-3) - NormRef.delta carries that term; nothing else is loosened for it."""
    b, h, w, c = shape
    g = gen(seed)
    x = randn_bf(shape, g)
    sig = 0.5 + 1.5 * torch.rand(c, generator=g, device=DEV)
    fam = torch.arange(c, device=DEV) % 8
    off = torch.where(fam >= 5, 16.0, torch.where(fam >= 3, 4.0, 0.0)) * sig * torch.where(fam % 2 == 0, 1.0, -1.0)
    x.mul_(sig.to(BF16)).add_(off.to(BF16))
    x[..., fam == 6] = 0
    x[..., 7] = const_value
    gamma = 1 + 0.2 * torch.randn(c, generator=g, device=DEV)
    gamma[::5] *= -1
    beta = 0.1 * torch.randn(c, generator=g, device=DEV)
    rm0 = torch.randn(c, generator=g, device=DEV)
    rv0 = 0.5 + torch.rand(c, generator=g, device=DEV)
    return x, gamma, beta, rm0, rv0


def param(v, slot=False, seed=0):
    p = torch.nn.Parameter(v.clone())
    if slot:  # an arena gradient slot as FlatSGD registers it (solver/build.py), already holding a gradient
        p._u2_grad = torch.randn(v.shape, generator=gen(seed), device=DEV)
        p._u2_prior = p._u2_grad.clone()
    return p


def combine(douts, rs=None, s=None):
    """dout (+ dout2 (+ dout3)) as autograd forms it: bf16 sums, one handle after the other."""
    sel = (lambda d: d[s, rs]) if rs is not None else (lambda d: d)
    d = sel(douts[0]).to(F64)
    for e in douts[1:]:
        d = rnd(d + sel(e).to(F64))
    return d


def out_chain(res, relu):
    """The forward reference after the normalisation, as a function of the normalised value v (float64): under autocast the
    norm output is a bf16 tensor, `+ shortcut` a bf16 sum, then the ReLU, stored as bf16.  rounded=False leaves off the last
    rounding (the value the max-normalised comparison is made against).
    Residual outputs carry no max-normalised bound: where v lies within the kernel's fp32 error of a rounding midpoint, the
    two intermediate bf16 values are one step of |v| apart, and |v| can exceed the largest output (at res4 that is 0.047 at an
    output range of 9.25, 5.1e-3); the interval check bounds these elements exactly instead."""
    def chain(v, rounded=True):
        if res is not None:
            v = rnd(v) + res.to(F64)
        if relu:
            v = v.clamp_min(0)
        return rnd(v) if rounded else v
    return chain


def check_backward(ref, name, douts3, out3, relu, dx3, gamma, beta, depth_b, dres3=None, extra_group_sum=0):
    """dx (and the materialised dz) of the float64 closed form; dgamma / dbeta (arena slices or .grad).
    dx = is (g dz - a - xhat bq), a = sum_{c in group} g_c sum dz_c / n, bq = sum g_c sum dz_c xhat_c / n (BN: cg = 1).
    kernel: colreduce sums S1 = sum dz, S2 = sum dz (x - mu_k) is_k in fp32 (chains of depth_b: gam = depth_b u), then
    dx = k1 dz + k2 x + k3 with k1 = g is_k, k2 = -is_k^2 bq_k, k3 = -is_k a_k + is_k^2 bq_k mu_k."""
    S, R, C, cg = ref.S, ref.R, ref.C, ref.cg
    G = C // cg
    gam = depth_b * U
    m1, m2, a1, a2 = (torch.zeros((S, C), dtype=F64, device=DEV) for _ in range(4))

    def dz_piece(s, rs):
        d = combine(douts3, rs, s)
        if relu:
            d = d * (out3[s, rs] > 0)
        return d

    for s, rs in pieces(S, R, C):
        d = dz_piece(s, rs)
        xh = (ref.x3[s, rs].to(F64) - ref.mu[s]) * ref.is_[s]
        m1[s] += d.sum(0)
        m2[s] += (d * xh).sum(0)
        a1[s] += d.abs().sum(0)
        a2[s] += (d * xh).abs().sum(0)
    grp = lambda t: t.view(S, G, cg).sum(2).repeat_interleave(cg, 1) / ref.n  # noqa: E731
    g = ref.g
    a, bq, A1, A2 = grp(g * m1), grp(g * m2), grp(g.abs() * a1), grp(g.abs() * a2)
    chk = Check(name + ": dx", 5e-3)
    chz = Check(name + ": dz", 4e-3) if dres3 is not None else None
    for s, rs in pieces(S, R, C):
        d = dz_piece(s, rs)
        xc = ref.x3[s, rs].to(F64)
        xh = (xc - ref.mu[s]) * ref.is_[s]
        is_, ih, dl, em = ref.is_[s], ref.is_hi[s], ref.delta[s], ref.e_mu[s]
        dx = is_ * (g[s] * d - a[s] - xh * bq[s])
        # is_k: relative delta on each factor of is (twice on the xhat bq term); S1, S2: gam sum|.|; xhat_k - xhat:
        # |xhat| delta + e_mu is_k; the coefficients and the final expression: at most six roundings each on k1 dz, k2 x, k3
        e = ih * (dl * ((g[s] * d).abs() + a[s].abs() + 2 * (xh * bq[s]).abs()) + gam * A1[s] + em * ih * bq[s].abs()
                  + xh.abs() * ((gam + dl) * A2[s] + em * ih * A1[s])) \
            + 6 * U * ih * ((g[s] * d).abs() + ih * bq[s].abs() * (xc.abs() + ref.mu[s].abs()) + a[s].abs())
        chk.add(dx3[s, rs], dx, 2 * e)
        if chz is not None:
            chz.add(dres3[s, rs], d, torch.zeros_like(d))  # the kernel's dz is the same bf16 sum and the same mask: exact
    chk.done()
    if chz is not None:
        chz.done()
    # parameter gradients: dbeta = sum S1 (gam sum|dz|, plus the fp32 sum over images for GN), dgamma = sum S2
    # ((gam + delta) sum|dz xhat| + e_mu is_k sum|dz|); an arena slice adds one rounding of prior + result
    nb = extra_group_sum * U
    db_ref, dg_ref = m1.sum(0), m2.sum(0)
    db_bnd = ((gam + nb) * a1).sum(0)
    dg_bnd = ((gam + nb + ref.delta) * a2 + ref.e_mu * ref.is_hi * a1).sum(0)
    for p, r, bnd, nm in ((beta, db_ref, db_bnd, "dbeta"), (gamma, dg_ref, dg_bnd, "dgamma")):
        slot = getattr(p, "_u2_grad", None)
        if slot is not None:
            assert p.grad is None, nm + ": the arena slot was bypassed"
            prior = p._u2_prior.to(F64)
            got = slot.to(F64) - prior
            bnd = bnd + U * (prior.abs() + r.abs())
        else:
            got = p.grad
        check_vec(name + ": " + nm, got, r, 2 * bnd, 1e-4)


def check_stats(ref, name, mean, invstd, rm, rv, rm0, rv0):
    """mean / invstd of the finalize and the running statistics (momentum 0.1, unbiased factor n / (n - 1))."""
    n = ref.n
    mu, var, e_mu, e_var = ref.mu[0], ref.var[0], ref.e_mu[0], ref.e_var[0]
    check_vec(name + ": mean", mean, mu, 2 * e_mu)
    check_vec(name + ": invstd", invstd, ref.is_[0], 2 * ref.delta[0] * ref.is_[0])
    rm0, rv0 = rm0.to(F64), rv0.to(F64)
    unb = var * n / (n - 1)
    # (1 - m) r + m v: the update's four roundings on each term, plus m times the error of v
    check_vec(name + ": running_mean", rm, (1 - MOM) * rm0 + MOM * mu, 2 * (MOM * e_mu + 4 * U * ((1 - MOM) * rm0.abs() + MOM * mu.abs())))
    check_vec(name + ": running_var", rv, (1 - MOM) * rv0 + MOM * unb,
              2 * (MOM * e_var * n / (n - 1) + 4 * U * ((1 - MOM) * rv0 + MOM * unb)))


# -------------------------------------------------------------------------------------------------
# 1 + 2: BatchNorm through batch_norm_act at the benchmark's shapes, every wrapper combination
BN_SHAPES = {
    "res2_c64": (16, 200, 336, 64),      # 138 MB: just under NT_BYTES
    "res2_c256": (16, 200, 336, 256),    # 550 MB: non-temporal accesses
    "res4_c1024": (16, 50, 84, 1024),    # 138 MB
    "res5_c2048": (16, 25, 42, 2048),    # cpr = 256: the widest fast case, one row per work-group lane set
}
# (name, residual, relu, handles, arena slots)
BN_MODES = [
    ("plain", False, False, 1, False),           # MASK 0
    ("relu", False, True, 1, False),             # MASK 2: x * scale + shift > 0 recomputed
    ("relu_twin", False, True, 2, False),        # MASK 2 on the bf16 sum autograd forms of two handles
    ("res_relu", True, True, 1, True),           # MASK 3: relu bits, dz materialised; dgamma / dbeta into arena slices
    ("res_relu_twin", True, True, 2, False),     # MASK 3 + dout2 summed in the reduce kernel
    ("res_relu_twin3", True, True, 3, False),    # MASK 3 + dout2 + dout3
]


@pytest.mark.parametrize("shape_name", list(BN_SHAPES))
def test_batch_norm_act_full_shape(F, shape_name):
    shape = BN_SHAPES[shape_name]
    b, h, w, c = shape
    m = b * h * w
    x, gamma0, beta0, rm0, rv0 = bn_inputs(shape, seed=sum(shape))
    ref = NormRef(x.view(1, m, c), gamma0, beta0, 1, U)
    stats = torch.stack([ref.col_s1[0], ref.col_s2[0]]).float()
    g = gen(c + 1)
    res = randn_bf(shape, g)
    douts = [randn_bf(shape, g)]
    depth_b = reduce_depth(1, m, c)
    for k, (mode, has_res, relu, handles, slots) in enumerate(BN_MODES):
        while len(douts) < handles:
            douts.append(randn_bf(shape, g))
        name = "%s/%s" % (shape_name, mode)
        gamma, beta = param(gamma0, slots, 2 * k), param(beta0, slots, 2 * k + 1)
        rm, rv = rm0.clone(), rv0.clone()
        xd = x.detach().requires_grad_(True)     # leaves on the same memory: no copy of the full-size tensors
        rd = res.detach().requires_grad_(True) if has_res else None
        out = F.batch_norm_act(xd, stats, gamma, beta, rm, rv, rd, relu, MOM, EPS, twin=(handles if handles > 1 else False))
        saved = out.grad_fn.saved_tensors   # (y, out | bits | None, gamma, mean, invstd, scale | None, shift | None)
        check_stats(ref, name, saved[3], saved[4], rm, rv, rm0, rv0)
        chk = Check(name + ": out", None if has_res else 4e-3)
        for s, rs in pieces(1, m, c):
            _, _, y, e = ref.y(s, rs)
            chain = out_chain(res.view(m, c)[rs] if has_res else None, relu)
            chk.add_interval(out.view(m, c)[rs], chain(y - e), chain(y + e), chain(y, rounded=False))
        chk.done()
        hs = [out, getattr(out, "_u2_twin", None), getattr(out, "_u2_third", None)][:handles]
        torch.autograd.backward(hs, douts[:handles])
        o3 = out.detach().view(1, m, c)
        d3 = [d.view(1, m, c) for d in douts[:handles]]
        check_backward(ref, name, d3, o3, relu, xd.grad.view(1, m, c), gamma, beta, depth_b,
                       rd.grad.view(1, m, c) if has_res else None)
        del out, hs, xd, rd, saved, o3
    del douts, res


def test_batch_norm_act_fpn_upsample_add_full_shape(F):
    """FPN top-down step at p2 (res_up=True: u2_bn_finalize_fwd + u2_affine_upadd forward, u2_bn_bwd_apply_fused +
    u2_fpn_upsample_add_bwd backward): out = bf16(bf16(norm(y)) + nearest_x2(top)), 550 MB (non-temporal), no ReLU."""
    shape = (16, 200, 336, 256)
    b, h, w, c = shape
    m = b * h * w
    x, gamma0, beta0, rm0, rv0 = bn_inputs(shape, seed=77)
    ref = NormRef(x.view(1, m, c), gamma0, beta0, 1, U)
    stats = torch.stack([ref.col_s1[0], ref.col_s2[0]]).float()
    g = gen(78)
    top = randn_bf((b, h // 2, w // 2, c), g).requires_grad_(True)
    dout = randn_bf(shape, g)
    gamma, beta = param(gamma0, True, 5), param(beta0, True, 6)
    rm, rv = rm0.clone(), rv0.clone()
    xd = x.detach().requires_grad_(True)
    out = F.batch_norm_act(xd, stats, gamma, beta, rm, rv, top, False, MOM, EPS, res_up=True)
    saved = out.grad_fn.saved_tensors
    check_stats(ref, "fpn", saved[3], saved[4], rm, rv, rm0, rv0)
    idx = torch.arange(m, device=DEV)
    top2 = top.detach().view(-1, c)
    chk = Check("fpn: out", None)
    for s, rs in pieces(1, m, c):
        _, _, y, e = ref.y(s, rs)
        r = idx[rs]
        bi, rem = r // (h * w), r % (h * w)
        trow = (bi * (h // 2) + (rem // w) // 2) * (w // 2) + (rem % w) // 2
        chain = out_chain(top2[trow], False)
        chk.add_interval(out.view(m, c)[rs], chain(y - e), chain(y + e), chain(y, rounded=False))
    chk.done()
    out.backward(dout)
    check_backward(ref, "fpn", [dout.view(1, m, c)], None, False, xd.grad.view(1, m, c), gamma, beta, reduce_depth(1, m, c))
    # the coarser level's gradient: the fp32 sum of each 2 x 2 block of dout, rounded once (four bf16 terms: 3 u sum|.|)
    d6 = dout.view(b, h // 2, 2, w // 2, 2, c)
    chk = Check("fpn: dtop", 4e-3)
    for i in range(b):
        di = d6[i].to(F64)
        chk.add(top.grad[i], di.sum((1, 3)), 3 * U * di.abs().sum((1, 3)))
    chk.done()


# -------------------------------------------------------------------------------------------------
# 3: C-ABI modes the wrapper does not reach
@pytest.mark.parametrize("c", [128, 96, 160])
def test_batch_norm_direct_abi_modes(H, c):
    """u2_bn_act_fused / u2_norm_bwd_reduce / u2_bn_bwd_apply_fused called directly.  C = 128: MASK 1 (the activation is
    read) in the reduce with and without dz, and in the one-launch apply.  C = 96 / 160 (C / 8 does not divide 256): the
    launchers fall back to finalize + affine_act_kernel / norm_bwd_apply_kernel (grid-stride: 10.8 M elements over at most 4096
    work-groups), with a residual forward and both mask sources backward."""
    shape = (16, 50, 84, c)
    b, h, w, _ = shape
    m = b * h * w
    x, gamma, beta, rm0, rv0 = bn_inputs(shape, seed=c)
    ref = NormRef(x.view(1, m, c), gamma, beta, 1, U)
    sums = torch.stack([ref.col_s1[0], ref.col_s2[0]]).float().contiguous()
    g = gen(c + 3)
    res, dout, dout2 = randn_bf(shape, g), randn_bf(shape, g), randn_bf(shape, g)
    f32 = lambda: torch.empty(c, dtype=torch.float32, device=DEV)  # noqa: E731
    mean, invstd, scale, shift = f32(), f32(), f32(), f32()
    rm, rv = rm0.clone(), rv0.clone()
    out = torch.empty_like(x)
    H.call("u2_bn_act_fused", x, sums, float(m), None, gamma, beta, rm, rv, MOM, EPS, mean, invstd, scale, shift, res, out, m, c, c, 1,
           None)
    check_stats(ref, "abi%d" % c, mean, invstd, rm, rv, rm0, rv0)
    chk = Check("abi%d: out" % c, None)
    for s, rs in pieces(1, m, c):
        _, _, y, e = ref.y(s, rs)
        chain = out_chain(res.view(m, c)[rs], True)
        chk.add_interval(out.view(m, c)[rs], chain(y - e), chain(y + e), chain(y, rounded=False))
    chk.done()
    depth_b = reduce_depth(1, m, c)
    o3 = out.view(1, m, c)
    # (mask source, twin gradient): MASK 1 reading `out`, with dz materialised and dout2 summed in the kernel; MASK 2 from
    # scale / shift (this forward had a residual, so its sign is not `out`'s: the reference mask is x * scale + shift > 0)
    for k, (mode, with_dz) in enumerate((("mask1", False), ("mask1_dz", True), ("mask2", False))):
        name = "abi%d/%s" % (c, mode)
        gp, bp = param(gamma, True, 10 + k), param(beta, True, 20 + k)
        sums_b = torch.zeros((2, c), dtype=torch.float32, device=DEV)
        dz = torch.empty_like(x) if with_dz else None
        msc, msh = (scale, shift) if mode == "mask2" else (None, None)
        mask = None if mode == "mask2" else out
        H.call("u2_norm_bwd_reduce", dout, mask, x, mean, invstd, sums_b, 1, m, c, c, 1, msc, msh, dout2 if with_dz else None, dz,
               None, 0)
        coef = torch.empty((3, c), dtype=torch.float32, device=DEV)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x)
        if with_dz:   # the apply pass reads dz and x only (relu = 0), as the residual tail does
            H.call("u2_bn_bwd_apply_fused", sums_b, float(m), None, gp, mean, invstd, sums_b, gp._u2_grad, bp._u2_grad, coef, 1,
                   dz, None, x, dx, dres, m, c, c, 0, None, None)
        else:
            H.call("u2_bn_bwd_apply_fused", sums_b, float(m), None, gp, mean, invstd, sums_b, gp._u2_grad, bp._u2_grad, coef, 1,
                   dout, mask, x, dx, dres, m, c, c, 1, msc, msh)
        if mode == "mask2":   # the forward's own expression in fp32 (two roundings, no contraction, as the kernel evaluates it)
            msk3 = (x.float() * scale + shift).view(1, m, c)
        else:
            msk3 = o3
        douts = [dout.view(1, m, c)] + ([dout2.view(1, m, c)] if with_dz else [])
        check_backward(ref, name, douts, msk3, True, dx.view(1, m, c), gp, bp, depth_b, dres.view(1, m, c))
        if with_dz:
            assert torch.equal(dz, dres)   # relu = 0: dres is dz as given


@pytest.mark.parametrize("slots,rows,c,ld", [(1, 1075201, 64, 64), (3, 100003, 96, 104), (16, 67200, 128, 128), (1, 9973, 2048, 2048)])
def test_colstats_sums_vs_float64(H, slots, rows, c, ld):
    """u2_colstats: per-slot column sums and sums of squares against float64 sums of the same bf16 values.  Row counts that are
    not a multiple of any block size (a prime, 64 * 512 * k + 1), a row pitch wider than C (the extra columns are not summed),
    > 32 768 rows per slot.  Bound: reduce_depth(...) u sum|term| (recursive summation; the squares are exact in fp32)."""
    g = gen(rows + c)
    x = randn_bf((slots, rows, ld), g)
    x.add_((torch.arange(ld, device=DEV) % 3).to(BF16))  # non-zero means: the sums do not cancel
    out = torch.zeros((slots, 2, c), dtype=torch.float32, device=DEV)
    H.call("u2_colstats", x, out, slots, rows, c, ld)
    gam = reduce_depth(slots, rows, c) * U
    for s in range(slots):
        xs = x[s, :, :c].to(F64)
        check_vec("colstats sum", out[s, 0], xs.sum(0), gam * xs.abs().sum(0))
        check_vec("colstats sumsq", out[s, 1], (xs * xs).sum(0), gam * (xs * xs).sum(0))


# -------------------------------------------------------------------------------------------------
# 4: GroupNorm through group_norm_act (the semantic head: 128 channels, 32 groups, ReLU)
@pytest.mark.parametrize("shape,slots", [((16, 200, 336, 128), False), ((16, 200, 336, 128), True), ((2, 20, 24, 64), False)],
                         ids=["head", "head_arena", "small_constant_group"])
def test_group_norm_act_full_shape(F, shape, slots):
    b, h, w, c = shape
    hw = h * w
    groups = 32
    cg = c // groups
    g = gen(hw + c + int(slots))
    x = randn_bf(shape, g)
    sig = 0.5 + 1.5 * torch.rand((b, 1, 1, c), generator=g, device=DEV)
    off = torch.where(torch.arange(c, device=DEV) // cg % 3 == 1, 8.0, 0.0) * sig   # group means at 0 and ~8 sigma
    x.mul_(sig.to(BF16)).add_(off.to(BF16))
    x[:, :, :, cg * 5: cg * 6] = 0           # an all-zero group
    if b <= 2:
        # a constant non-zero group: var = 0, the result rests on eps (a power of two: the fp32 sums are exact, mu = 0.25)
        x[0, :, :, 0:cg] = 0.25
    gamma0 = 1 + 0.2 * torch.randn(c, generator=g, device=DEV)
    gamma0[::5] *= -1
    beta0 = 0.1 * torch.randn(c, generator=g, device=DEV)
    gamma, beta = param(gamma0, slots, 31), param(beta0, slots, 32)
    xd = x.detach().requires_grad_(True)
    out = F.group_norm_act(xd, gamma, beta, groups, True, EPS)
    x3 = x.view(b, hw, c)
    ref = NormRef(x3, gamma0, beta0, cg, (reduce_depth(b, hw, c) + cg) * U)
    name = "gn%s" % ("_arena" if slots else "")
    saved = out.grad_fn.saved_tensors   # (y, gamma, mean [B][C], invstd [B][C], scale, shift)
    check_vec(name + ": mean", saved[2], ref.mu, 2 * ref.e_mu)
    check_vec(name + ": invstd", saved[3], ref.is_, 2 * ref.delta * ref.is_)
    chk = Check(name + ": out", 4e-3)
    o3 = out.detach().view(b, hw, c)
    chain = out_chain(None, True)
    for s, rs in pieces(b, hw, c):
        _, _, y, e = ref.y(s, rs)
        chk.add_interval(o3[s, rs], chain(y - e), chain(y + e), chain(y, rounded=False))
    chk.done()
    dout = randn_bf(shape, g)
    out.backward(dout)
    check_backward(ref, name, [dout.view(b, hw, c)], o3, True, xd.grad.view(b, hw, c), gamma, beta,
                   reduce_depth(b, hw, c) + cg, extra_group_sum=b)


# -------------------------------------------------------------------------------------------------
# 5: the stem tail, norm -> bf16 -> ReLU -> max_pool2d(3, 2, 1) as one pass each way
def test_stem_tail_full_shape(F):
    """batch_norm_relu_max_pool at 16 x 400 x 672 x 64 (550 MB) against the float64 chain.  Forward: pooled values per element
    (max is 1-Lipschitz: the window's largest activation bound); the winner slots the pass records (its backward routes by
    them) against the first-max rule: the winner's activation is the window's maximum within the bounds, and no earlier slot
    ties with it exactly - same input value (same activation in the kernel), or both certainly negative before the ReLU (both
    0 after it: after the ReLU many windows tie at 0).  Backward: the float64 closed form on dz = bf16(sum of dy over the
    windows a pixel wins), masked where the pixel's activation is 0, routed by the recorded winners."""
    shape = (16, 400, 672, 64)
    b, h, w, c = shape
    m = b * h * w
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x, gamma0, beta0, rm0, rv0 = bn_inputs(shape, seed=11)
    ref = NormRef(x.view(1, m, c), gamma0, beta0, 1, U)
    stats = torch.stack([ref.col_s1[0], ref.col_s2[0]]).float()
    gamma, beta = param(gamma0), param(beta0)
    rm, rv = rm0.clone(), rv0.clone()
    xd = x.detach().requires_grad_(True)
    out = F.batch_norm_relu_max_pool(xd, stats, gamma, beta, rm, rv, MOM, EPS)
    saved = out.grad_fn.saved_tensors   # (y, idx, gamma, mean, invstd, scale, shift)
    idx = saved[1]
    check_stats(ref, "stem", saved[3], saved[4], rm, rv, rm0, rv0)
    hw = h * w
    pad = lambda t, v: TF.pad(t.permute(2, 0, 1), (1, 2, 1, 2), value=v).permute(1, 2, 0)  # noqa: E731
    tap = lambda t, k: t[k // 3: k // 3 + 2 * ho: 2, k % 3: k % 3 + 2 * wo: 2]  # noqa: E731
    max_err = max_ref = 0.0
    for i in range(b):
        rs = slice(i * hw, (i + 1) * hw)
        xc, _, y, e = ref.y(0, rs)
        # the kernel's activation bf16(relu(f)) with |f - y| <= e lies in [lo, hi] (rounding and ReLU are monotone)
        lo = rnd((y - e).clamp_min(0)).view(h, w, c)
        hi = rnd((y + e).clamp_min(0)).view(h, w, c)
        act = rnd(y.clamp_min(0)).view(h, w, c)          # the activation of the reference model
        lo_p, hi_p, act_p, x_p = pad(lo, -1.0), pad(hi, -1.0), pad(act, -1.0), pad(xc.view(h, w, c), float("nan"))
        del xc, y, e, lo, hi, act
        got = out[i].detach().to(F64)
        sl = idx[i].long()
        pool_lo, pool_hi, pool_ref = (torch.full((ho, wo, c), -1.0, dtype=F64, device=DEV) for _ in range(3))
        lo_w, hi_w, x_w = torch.full_like(got, -1.0), torch.full_like(got, -1.0), torch.zeros_like(got)
        for k in range(9):   # window slots in max_pool2d's scan order
            pool_lo, pool_hi = torch.maximum(pool_lo, tap(lo_p, k)), torch.maximum(pool_hi, tap(hi_p, k))
            pool_ref = torch.maximum(pool_ref, tap(act_p, k))
            on = sl == k
            lo_w, hi_w, x_w = torch.where(on, tap(lo_p, k), lo_w), torch.where(on, tap(hi_p, k), hi_w), torch.where(on, tap(x_p, k), x_w)
        # pooled value: the window's largest kernel activation lies between the largest lo and the largest hi
        assert bool(((got >= pool_lo) & (got <= pool_hi)).all()), "stem: pooled value outside the derived interval (image %d)" % i
        max_err, max_ref = max(max_err, float((got - pool_ref).abs().max())), max(max_ref, float(pool_ref.abs().max()))
        # the recorded winner: inside the map, and the pooled value is its activation
        assert bool((lo_w >= 0).all()), "stem: a winner slot outside the map (image %d)" % i
        assert bool(((got >= lo_w) & (got <= hi_w)).all()), "stem: pooled value is not the winner's activation (image %d)" % i
        for k in range(9):
            lk = tap(lo_p, k)
            # no slot's activation can exceed the winner's; an EARLIER slot must not even equal it (first max wins): certain
            # when its lowest possible activation reaches the pooled value (both 0 after the ReLU included) or when it holds
            # the winner's very input value
            assert not bool((lk > got).any()), "stem: slot %d beats the recorded winner (image %d)" % (k, i)
            earlier = sl > k
            tie = (lk >= got) | (tap(x_p, k) == x_w)
            assert not bool((earlier & tie).any()), "stem: slot %d ties with a later winner: not the first max (image %d)" % (k, i)
        del lo_p, hi_p, act_p, x_p, pool_lo, pool_hi, pool_ref, lo_w, hi_w, x_w
    assert max_err <= 4e-3 * max_ref, (max_err, max_ref)
    dy = randn_bf(out.shape, gen(12))
    out.backward(dy)
    # dz of every input pixel from the recorded winners: dy of the windows it wins, where the window's value is > 0
    dz = torch.empty(shape, dtype=BF16, device=DEV)
    for i in range(b):
        canvas = torch.zeros((h + 3, w + 3, c), dtype=F64, device=DEV)
        dyi = dy[i].to(F64) * (out[i] > 0)
        for k in range(9):
            canvas[k // 3: k // 3 + 2 * ho: 2, k % 3: k % 3 + 2 * wo: 2] += dyi * (idx[i] == k)
        dz[i] = canvas[1: h + 1, 1: w + 1].to(BF16)   # the fp32 sum of at most four bf16 terms, rounded once
        del canvas
    check_backward(ref, "stem", [dz.view(1, m, c)], None, False, xd.grad.view(1, m, c), gamma, beta, stem_depth(b, h, w, c))
