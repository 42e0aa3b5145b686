"""u2_sgd_step_opts (u2seg_amd/csrc/optim.hip) - clipping by value, by L2 / L1 / inf norm, Nesterov momentum, two learning rates -
against a float64 restatement (tests/solver_option_refs.py), at its decision edges, against u2_sgd_clip_step, and through
FlatSGD against the reference's own optimizer (tests/golden/solver_options_golden.npz).

The arena (solver_option_refs.SIZES): tensors of 1, 7, 65 536, 75 000 and 5 elements - a tensor that is all head, one full chunk,
a two-chunk tensor, a tail shorter than 4 - with per-tensor weight decay of 0 and > 0 and mixed learning-rate classes.  Every test
runs at least two consecutive steps, so that the momentum read in the second is the first's."""
import json
import os

import numpy as np
import pytest
import torch

from tests import float64_refs as R
from tests import solver_option_refs as S
from tests.test_gpu_norm_full_size import U, check_vec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
F32 = torch.float32
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024   # elements in front of and behind the arena: its base stays 16-byte aligned, as the kernels assume
SIZES = S.SIZES
TOTAL = sum(SIZES)
WD = [0.0, 1e-4, 5e-2, 0.0, 1e-4]
LR_CLASS = [0, 1, 0, 0, 1]
CLIP_OF = {S.NONE: 0.0, S.VALUE: 0.02, S.L2: 1.0, S.L1: 1.0, S.INF: 1.0}
# per-tensor gradient magnitudes (times randn, divided by grad_scale).  With the clips above: by value, tensors 0, 1, 4 have most
# elements clamped, tensor 2 about 5 %, tensor 3 none; L2 norms 0.3, 0.05, 2.6, 0.27, 18; L1 norms 0.2, 0.1, 520, 60, 32; inf norms
# 0.3, 0.04, 0.045, 0.0045, 12 (about): each norm mode clips some tensors and leaves others alone.
GRAD_MAG = [0.3, 0.02, 0.01, 0.001, 8.0]


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()  # fails loudly if libu2seg_hip.so is absent
    return _hip


@pytest.fixture(scope="module")
def tables():
    ct, cb, cl, fc = R.chunk_tables(SIZES)
    assert len(ct) == 6 and cl == [1, 7, R.CHUNK, R.CHUNK, 75000 - R.CHUNK, 5] and cb == [0, 1, 8, 65544, 131080, 140544]
    return {"chunk_tensor": torch.tensor(ct, dtype=torch.int32, device=DEV),
            "chunk_begin": torch.tensor(cb, dtype=torch.int64, device=DEV),
            "chunk_len": torch.tensor(cl, dtype=torch.int32, device=DEV),
            "first_chunk": torch.tensor(fc, dtype=torch.int32, device=DEV),
            "n": len(ct)}


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def bits(t):
    return t.view(torch.int32)


def dev_f32(values):
    return torch.tensor(values, dtype=F32, device=DEV)


def step_opts(H, T, p, g, m, partial, wd, lr_class, lr, lr_bias, mom, nesterov, mode, clip, scale):
    H.call("u2_sgd_step_opts", p, g, m, T["chunk_tensor"], T["chunk_begin"], T["chunk_len"], T["n"], partial, T["first_chunk"], wd,
           lr_class, lr, lr_bias, mom, int(nesterov), mode, clip, scale)


def seeded_grads(g0, scale):
    return torch.cat([(torch.randn(n, generator=g0, device=DEV, dtype=F64) * (a / scale)).float() for n, a in zip(SIZES, GRAD_MAG)])


# =================================================================================================
# 1. float64, per element
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("mode", [S.NONE, S.VALUE, S.L2, S.L1, S.INF])
def test_step_opts_abi_vs_float64(H, tables, mode, nesterov, scale):
    """u2_sgd_step_opts through the C ABI, the arena a slice [GUARD, GUARD + total) of larger buffers whose guard bands must stay
    bit-unchanged; two steps, the reference of the second starting from the kernel's own p, m after the first, so the one-step
    bound applies to each.  `partial` is NaN before every step: modes 0 and 1 must not touch it, the norm modes must have written
    every entry they read.

    Reference (float64, on the fp32 values of lr / lr_bias / mom / clip / scale / wd as the kernel receives them):
        coef = min(clip / (norm(g) scale + 1e-6f), 1) scale for the norm modes, scale otherwise;   g' = g coef, clamped to
        [-clip, clip] in mode 1;   d = g' + wd p;   m' = mom m + d;   u = d + mom m' (Nesterov) or m';   p' = p - lr_t u
    Bound, per element, fp32 roundings u = 2^-24 to first order (the library is built without contraction and without fast-math:
    every product, sum, division and square root rounds once, correctly; a fused multiply-add would only remove roundings):
        err(d)  <= eps_c |g'| + 4 u (|g'| + |wd p|)
        err(m') <= err(d) + 4 u |mom m|
        err(u)  =  err(m') without Nesterov;   err(d) + mom err(m') + 2 u |mom m'| + u |d| with it
        err(p') <= lr_t err(u) + 2 u (|p| + lr_t |u|)
      eps_c, the relative error of the coefficient before `* grad_scale`:
        L2   (d2 / 2 + 4) u, d2 = float64_refs.sumsq_depth(chunks): the bound of u2_sgd_clip_step, whose norm pass this is.
        L1   (d2 - 1 + 3) u: the same chain of additions of non-negative terms without the rounding of the square (|g| is exact)
             and without the square root, which halved the sum's error and rounded once; `* grad_scale`, `+ 1e-6f` and the division
             round once each.
        inf  3 u: a maximum is exact; `* grad_scale`, `+ 1e-6f` and the division round.
        0, 1 zero: the factor is the scalar handed in.
      fminf(., 1) and the clamp of mode 1 are exact and do not increase an error (|clamp(a) - clamp(b)| <= |a - b|).
      4 u: g' passes `coef *= grad_scale`, its product, `+ wd p` and `+ mom m` (4 roundings, 3 of them in d: 4 bounds both); wd p
        its product and the two sums; mom m its product and the last sum.
      Nesterov adds one multiply-add: mom m' rounds (u |mom m'|) and the sum rounds (u |u| <= u (|d| + |mom m'|)).
      p': lr_t u rounds once, the difference once (u |p'| <= u (|p| + lr_t |u|))."""
    T = tables
    wd_dev, cls_dev = dev_f32(WD), torch.tensor(LR_CLASS, dtype=torch.int32, device=DEV)
    wd = wd_dev.double().tolist()
    lr, lr_bias, mom, clip, scale = S.f32(0.1), S.f32(0.2), S.f32(0.9), S.f32(CLIP_OF[mode]), S.f32(scale)
    lr_t = [lr_bias if c else lr for c in LR_CLASS]
    g0 = gen(100 * mode + 10 * int(nesterov) + int(scale * 8))
    sentinel = torch.arange(TOTAL + 2 * GUARD, dtype=torch.int32, device=DEV) + 0x3F000000   # distinct floats near 0.5

    def buffer():
        b = torch.empty(TOTAL + 2 * GUARD, dtype=F32, device=DEV)
        bits(b).copy_(sentinel)
        return b

    bufs = [buffer() for _ in range(3)]
    P, Gd, M = (b[GUARD: GUARD + TOTAL] for b in bufs)
    assert all(v.data_ptr() % 16 == 0 for v in (P, Gd, M))
    P.copy_(torch.randn(TOTAL, generator=g0, device=DEV))
    M.copy_(0.1 * torch.randn(TOTAL, generator=g0, device=DEV))
    partial = torch.empty(T["n"], dtype=F32, device=DEV)
    for k in range(2):
        g = seeded_grads(g0, scale)
        Gd.copy_(g)
        p0, m0 = P.clone(), M.clone()
        partial.fill_(NAN)
        step_opts(H, T, P, Gd, M, partial, wd_dev, cls_dev, lr, lr_bias, mom, nesterov, mode, clip, scale)
        for b, nm in zip(bufs, "pgm"):
            assert torch.equal(bits(b)[:GUARD], sentinel[:GUARD]), "step %d wrote in front of the %s arena" % (k, nm)
            assert torch.equal(bits(b)[GUARD + TOTAL:], sentinel[GUARD + TOTAL:]), "step %d wrote behind the %s arena" % (k, nm)
        assert torch.equal(Gd, g), "the gradients were modified"
        assert bool(partial.isnan().all()) == (mode in (S.NONE, S.VALUE)), "the norm pass ran / did not run"
        if mode == S.VALUE:   # the case is about clamping: some elements are clamped, some are not
            inside = (g.double() * scale).abs() < clip
            assert int(inside.sum()) > 1000 and int((~inside).sum()) > 1000
        if mode >= S.L2:
            coef = S.opts_coef(g, SIZES, mode, clip, scale) / scale
            assert bool((coef < 0.9).any()) and bool((coef == 1.0).any()), coef
        rp, rm, _, _ = S.sgd_opts_ref(p0, g, m0, SIZES, wd, lr_t, mom, nesterov, mode, clip, scale)
        ep, em = S.sgd_opts_bounds(p0, g, m0, SIZES, wd, lr_t, mom, nesterov, mode, clip, scale, U)
        off = 0
        for t, n in enumerate(SIZES):
            s = slice(off, off + n)
            check_vec("step %d: m of tensor %d (%d elements at %d)" % (k, t, n, off), M[s], rm[s], em[s])
            check_vec("step %d: p of tensor %d (%d elements at %d)" % (k, t, n, off), P[s], rp[s], ep[s])
            off += n


# =================================================================================================
# 2. decision edges
def plain_state(g0):
    """Parameters, zero momentum, zero weight decay: with momentum 0 the step leaves m' = g', the gradient as clipped."""
    p = torch.randn(TOTAL, generator=g0, device=DEV)
    m = torch.zeros(TOTAL, device=DEV)
    wd = torch.zeros(len(SIZES), device=DEV)
    cls = torch.tensor(LR_CLASS, dtype=torch.int32, device=DEV)
    partial = torch.full((6,), NAN, device=DEV)
    return p, m, wd, cls, partial


def test_value_clip_at_the_threshold(H, tables):
    """Mode 1 with grad_scale 0.125 (a power of two: g scale is exact): every arena position - heads, float4 bodies, tails, both
    chunks of the long tensor - holds in turn g scale = +-clip, one ulp inside, one ulp outside, and values far inside and far
    outside.  With momentum 0 and no weight decay m' is the clamped gradient: it must equal the float32 clamp bit for bit
    (clip_grad_value_'s clamp_(min=-clip, max=clip) on the averaged gradient), in two consecutive steps with the pattern shifted."""
    scale, clip = 0.125, S.f32(0.02)
    c = torch.tensor(clip, dtype=F32)
    edge = c / scale                                            # exact: scale is 2^-3
    inf_ = torch.tensor(float("inf"))
    vals = torch.stack([edge, -edge, torch.nextafter(edge, inf_), torch.nextafter(edge, -inf_), torch.nextafter(-edge, inf_),
                        torch.nextafter(-edge, -inf_), edge * 0.37, -edge * 0.37, edge * 11.0, -edge * 11.0, torch.tensor(0.0)])
    g0 = gen(5)
    p, m, wd, cls, partial = plain_state(g0)
    for k in range(2):
        g_cpu = vals[(torch.arange(TOTAL) + 3 * k) % len(vals)]
        want = torch.clamp(g_cpu * torch.tensor(scale, dtype=F32), -c, c)
        assert int((want == c).sum()) >= 3 * (TOTAL // len(vals)) - 3 and bool((want.abs() <= c).all())
        g = g_cpu.to(DEV)
        p0 = p.clone()
        step_opts(H, tables, p, g, m, partial, wd, cls, S.f32(0.1), S.f32(0.2), 0.0, False, S.VALUE, clip, scale)
        assert torch.equal(bits(m.cpu()), bits(want + 0.0)), "step %d: the clamped gradient differs from the float32 clamp" % k
        lr_el = S.per_tensor([S.f32(0.2) if c_ else S.f32(0.1) for c_ in LR_CLASS], SIZES, p0.cpu()).float()
        assert torch.equal(p.cpu(), p0.cpu() - lr_el * want), "step %d: p' != p - lr_t g'" % k
    assert bool(partial.isnan().all())


@pytest.mark.parametrize("where,pos", [("head", 1), ("tail", 140548), ("end of the first chunk", 131079), ("second chunk", 131180)])
def test_inf_norm_finds_a_negative_maximum(H, tables, where, pos):
    """Mode 4: the element of largest magnitude is negative (-3 among |g| <= 0.5) and sits at `pos`: a head element of tensor 1, the
    tail element of tensor 4, the last element of the long tensor's first chunk, an element of its second chunk.  With momentum 0
    and no weight decay m' = g (coef scale): for the tensor that holds it, it must equal the float32 expression
    g * (min(clip / (3 scale + 1e-6f), 1) * scale) bit for bit, and the other tensors' coefficient is exactly 1 (max 0.5 scale <
    clip).  Two steps: the second with the sign of every gradient flipped."""
    scale, clip = S.f32(0.5), S.f32(1.0)
    g0 = gen(pos)
    p, m, wd, cls, partial = plain_state(g0)
    starts = [sum(SIZES[:t]) for t in range(len(SIZES))]
    t_hit = max(t for t, s in enumerate(starts) if s <= pos)
    assert t_hit == {"head": 1, "tail": 4}.get(where, 3)
    g = torch.rand(TOTAL, generator=g0, device=DEV) - 0.5
    g[pos] = -3.0
    one, s32, c32 = torch.tensor(1.0), torch.tensor(scale, dtype=F32), torch.tensor(clip, dtype=F32)
    total = torch.tensor(3.0) * s32
    coef = torch.minimum(c32 / (total + torch.tensor(1e-6, dtype=F32)), one) * s32
    assert float(coef) < 0.7 * scale
    for k in range(2):
        gk = g if k == 0 else -g       # the maximum of |g| is where it was; the largest VALUE is now elsewhere in step 0, here in step 1
        step_opts(H, tables, p, gk, m, partial, wd, cls, S.f32(0.1), S.f32(0.2), 0.0, False, S.INF, clip, scale)
        got, gc = m.cpu(), gk.cpu()
        for t, (s, n) in enumerate(zip(starts, SIZES)):
            want = gc[s: s + n] * (coef if t == t_hit else one * s32)
            assert torch.equal(bits(got[s: s + n]), bits(want + 0.0)), "step %d, tensor %d" % (k, t)
    assert not bool(partial.isnan().any()) and float(partial.max()) == 3.0


@pytest.mark.parametrize("mode", [S.L2, S.L1, S.INF])
def test_norm_below_the_threshold_leaves_the_gradient_alone(H, tables, mode):
    """Every tensor's norm is below clip: min(clip / (total + 1e-6f), 1) is exactly 1, and with grad_scale 1, momentum 0 and no weight
    decay m' is the gradient bit for bit.  (L1 of the long tensor: 75 000 x 1e-6 x 0.8 = 0.06 < 1.)"""
    g0 = gen(40 + mode)
    p, m, wd, cls, partial = plain_state(g0)
    for k in range(2):
        g = torch.randn(TOTAL, generator=g0, device=DEV) * 1e-6
        step_opts(H, tables, p, g, m, partial, wd, cls, S.f32(0.1), S.f32(0.2), 0.0, False, mode, 1.0, 1.0)
        assert torch.equal(bits(m), bits(g + 0.0)), "step %d" % k
    assert float(partial.max()) < 1.0


# =================================================================================================
# 3. equality with the existing kernel
@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_l2_without_options_is_the_existing_step_bit_for_bit(H, tables, scale):
    """Mode 2, no Nesterov, lr_bias == lr: parameters and momentum after two steps are bit-identical to u2_sgd_clip_step on the
    same inputs (the norm pass is the same kernel, the step the same expressions in the same order)."""
    T = tables
    g0 = gen(77)
    wd_dev, cls_dev = dev_f32(WD), torch.tensor(LR_CLASS, dtype=torch.int32, device=DEV)
    lr, mom, clip, scale = S.f32(0.1), S.f32(0.9), S.f32(1.0), S.f32(scale)
    p_a = torch.randn(TOTAL, generator=g0, device=DEV)
    m_a = 0.1 * torch.randn(TOTAL, generator=g0, device=DEV)
    p_b, m_b = p_a.clone(), m_a.clone()
    part_a, part_b = torch.full((6,), NAN, device=DEV), torch.full((6,), NAN, device=DEV)
    for k in range(2):
        g = seeded_grads(g0, scale)
        coef = S.opts_coef(g, SIZES, S.L2, clip, scale) / scale
        assert bool((coef < 0.9).any()) and bool((coef == 1.0).any())
        H.call("u2_sgd_clip_step", p_a, g, m_a, T["chunk_tensor"], T["chunk_begin"], T["chunk_len"], T["n"], part_a, T["first_chunk"],
               wd_dev, lr, mom, clip, scale)
        step_opts(H, T, p_b, g, m_b, part_b, wd_dev, cls_dev, lr, lr, mom, False, S.L2, clip, scale)
        assert torch.equal(bits(part_a), bits(part_b)), "step %d: partial sums" % k
        assert torch.equal(bits(m_a), bits(m_b)), "step %d: momentum" % k
        assert torch.equal(bits(p_a), bits(p_b)), "step %d: parameters" % k


def test_bad_arguments_are_refused(H, tables):
    """clip_mode outside 0..4 and a clip <= 0 with a clipping mode answer -1 and launch nothing."""
    g0 = gen(3)
    p, m, wd, cls, partial = plain_state(g0)
    p0 = p.clone()
    g = torch.randn(TOTAL, generator=g0, device=DEV)
    for mode, clip in ((5, 1.0), (-1, 1.0), (S.VALUE, 0.0), (S.L1, -1.0)):
        with pytest.raises(RuntimeError, match="u2_sgd_step_opts failed with status -1"):
            step_opts(H, tables, p, g, m, partial, wd, cls, 0.1, 0.2, 0.9, False, mode, clip, 1.0)
    assert torch.equal(p, p0) and float(m.abs().sum()) == 0.0


# =================================================================================================
# 4. FlatSGD against the reference's optimizer
def build(case, **solver):
    from tests.test_solver_options_host import net_cfg
    from u2seg_amd.layers.modules import GroupNorm
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer

    cfg = net_cfg(case)
    for k, v in solver.pop("CLIP_GRADIENTS", {}).items():
        cfg.SOLVER.CLIP_GRADIENTS[k] = v
    for k, v in solver.items():
        cfg.SOLVER[k] = v
    net = S.build_net(GroupNorm).to(DEV)
    opt = build_optimizer(cfg, net)
    return cfg, net, opt, build_lr_scheduler(cfg, opt)


@pytest.mark.parametrize("case", sorted(S.NET_CASES))
def test_flat_sgd_options_vs_the_reference_optimizer(H, case):
    """FlatSGD.step + the cosine schedule on the small module of solver_option_refs (conv with bias, normalisation layer, linear
    layer, 75 000-element weight) with BIAS_LR_FACTOR 2, WEIGHT_DECAY_BIAS, Nesterov and clipping by value / L1 norm / inf norm:
    three steps on the fixture's gradients.
      * Each step is checked per element against sgd_opts_ref from the arena's state before it, with the bound of
        test_step_opts_abi_vs_float64 (the rates are the fp32 values the kernel received).
      * After the three steps parameters and momentum are compared with what the REFERENCE's build_optimizer (clip-wrapped
        torch.optim.SGD, foreach) + WarmupCosineLR left (solver_options_golden.npz).  The bound E3 is that one-step bound
        accumulated along a float64 run of the three steps from the common start (solver_option_refs.propagate carries the
        error of a step's inputs to its outputs, to first order), and the tolerance is 2 E3: the fixture is an fp32 computation
        of the same step - the same products and sums per element, a norm by torch's blocked summation, whose error is below
        the chain bound eps_c - so it lies within E3 of the float64 run as the kernel does.  (E3 also absorbs the rates: the
        kernel gets them rounded to fp32, relative 2^-24, torch multiplies by the double.)"""
    golden = np.load(os.path.join(ROOT, "tests", "golden", "solver_options_golden.npz"))
    cfg, net, opt, sched = build(case)
    params = list(net.parameters())
    sizes = [p.numel() for p in params]
    names = [k for k, _ in net.named_parameters()]
    assert names == [k for k, _ in S.NET_PARAMS] and (opt.chunk_tensor.tolist(), opt.chunk_begin.tolist(), opt.chunk_len.tolist(),
                                                        opt.first_chunk.tolist()) == R.chunk_tables(sizes)
    assert opt.lr_class.tolist() == [0, 1, 0, 1, 0, 1, 0] and opt.has_bias_lr
    wd = opt.wd.double().tolist()
    assert wd == [S.f32(v) for v in (1e-4, 1e-3, 0.0, 1e-3, 1e-4, 1e-3, 1e-4)]
    mode = {"value": S.VALUE, "l1": S.L1, "inf": S.INF}[case]
    mom, clip = S.f32(cfg.SOLVER.MOMENTUM), S.f32(cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE)
    calls = []
    real_call = H.call
    run_p, run_m = opt.flat_param.double(), opt.flat_mom.double()       # the float64 run from the common start
    acc_p, acc_m = torch.zeros_like(run_p), torch.zeros_like(run_p)
    try:
        H.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        for k in range(S.NET_STEPS):
            g = torch.cat([v.reshape(-1) for v in S.net_grads(k)]).to(DEV)
            for p, v in zip(params, S.net_grads(k)):
                p.grad.copy_(v)
            assert torch.equal(opt.flat_grad, g)
            lr_t = [S.f32(opt.lr_bias if c else opt.lr) for c in opt.lr_class.tolist()]
            assert [opt.lr, opt.lr_bias] == pytest.approx([golden[case + "/lrs"][k][0], golden[case + "/lrs"][k][1]], rel=1e-15)
            p0, m0 = opt.flat_param.clone(), opt.flat_mom.clone()
            opt.step(1.0)
            sched.step()
            rp, rm, _, _ = S.sgd_opts_ref(p0, g, m0, sizes, wd, lr_t, mom, True, mode, clip, 1.0)
            ep, em = S.sgd_opts_bounds(p0, g, m0, sizes, wd, lr_t, mom, True, mode, clip, 1.0, U)
            check_vec("%s step %d: m" % (case, k), opt.flat_mom, rm, em)
            check_vec("%s step %d: p" % (case, k), opt.flat_param, rp, ep)
            lr_el, wd_el = S.per_tensor(lr_t, sizes, run_p), S.per_tensor(wd, sizes, run_p)
            acc_p, acc_m = S.propagate(acc_p, acc_m, wd_el, lr_el, mom, True)
            e1p, e1m = S.sgd_opts_bounds(run_p, g, run_m, sizes, wd, lr_t, mom, True, mode, clip, 1.0, U)
            run_p, run_m, _, upd = S.sgd_opts_ref(run_p, g, run_m, sizes, wd, lr_t, mom, True, mode, clip, 1.0)
            acc_p, acc_m = acc_p + e1p + U * lr_el * upd.abs(), acc_m + e1m
    finally:
        H.call = real_call
    assert [c for c in calls if c.startswith("u2_sgd")] == ["u2_sgd_step_opts"] * S.NET_STEPS
    off = 0
    for name, n in zip(names, sizes):
        s = slice(off, off + n)
        want_p = torch.from_numpy(golden["%s/param/%s" % (case, name)]).to(DEV).double()
        want_m = torch.from_numpy(golden["%s/momentum/%s" % (case, name)]).to(DEV).double()
        check_vec("%s: %s vs the reference optimizer" % (case, name), S.kept(opt.flat_param[s]), want_p, 2 * S.kept(acc_p[s]))
        check_vec("%s: momentum of %s vs the reference optimizer" % (case, name), S.kept(opt.flat_mom[s]), want_m, 2 * S.kept(acc_m[s]))
        off += n
    assert json.loads(str(golden[case + "/numbering"])) == [names[i] for m in opt.group_members for i in m]


def test_flat_sgd_defaults_still_issue_the_existing_step(H):
    """Every option at its default (L2 clipping, no Nesterov, BIAS_LR_FACTOR 1, multi-step schedule): step() issues
    u2_sgd_clip_step, never u2_sgd_step_opts - with clipping and without."""
    from u2seg_amd.solver import WarmupMultiStepLR

    for clip_on in (True, False):
        cfg, net, opt, sched = build("l1", NESTEROV=False, BIAS_LR_FACTOR=1.0, LR_SCHEDULER_NAME="WarmupMultiStepLR", WARMUP_ITERS=2,
                                     STEPS=(5,), CLIP_GRADIENTS={"ENABLED": clip_on, "CLIP_TYPE": "norm", "CLIP_VALUE": 1.0,
                                                                 "NORM_TYPE": 2.0})
        assert type(sched) is WarmupMultiStepLR and not opt.has_bias_lr
        calls = []
        real_call = H.call
        try:
            H.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
            for k in range(2):
                for p, v in zip(net.parameters(), S.net_grads(k)):
                    p.grad.copy_(v)
                before = opt.flat_param.clone()
                opt.step(1.0)
                sched.step()
                assert not torch.equal(before, opt.flat_param)
        finally:
            H.call = real_call
        assert [c for c in calls if c.startswith("u2_sgd")] == ["u2_sgd_clip_step"] * 2
