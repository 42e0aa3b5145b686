"""Float64 restatement of u2_sgd_step_opts (u2seg_amd/csrc/optim.hip) with its derived error bound, and the small module, values
and gradients that tests/golden/make_solver_options_fixture.py, tests/test_solver_options_host.py and
tests/test_gpu_solver_options.py share.  Plain torch only; nothing here touches the HIP library."""
import math

import torch

from tests import float64_refs as R

F64 = torch.float64
NONE, VALUE, L2, L1, INF = range(5)                          # clip_mode of u2_sgd_step_opts
EPS32 = float(torch.tensor(1e-6, dtype=torch.float32))       # the kernel's 1e-6f

# The arena of the direct tests, in order (CHUNK = 65 536).  Offsets: 1 @ 0;  7 @ 1 (head 3, one float4);  65 536 @ 8 (exactly one
# full chunk);  75 000 @ 65 544 (two chunks: 65 536 and 9 464);  5 @ 140 544 (one float4 and a tail of 1).
SIZES = [1, 7, R.CHUNK, 75000, 5]


def f32(v):
    """The value a `float` argument of the C ABI carries."""
    return float(torch.tensor(v, dtype=torch.float32))


def per_tensor(values, sizes, like):
    return R._per_tensor(values, sizes, like)


def opts_coef(g, sizes, mode, clip, scale):
    """Per-tensor factor on the gradient, float64 [n_tensors]: min(clip / (norm(g) scale + 1e-6f), 1) scale for the norm modes -
    clip_grad_norm_(p, clip, 2 | 1 | inf) on gradients pre-scaled by `scale` - and `scale` for modes 0 and 1."""
    g = g.to(F64)
    if mode in (NONE, VALUE):
        return torch.full((len(sizes),), float(scale), dtype=F64, device=g.device)
    p = {L2: 2.0, L1: 1.0, INF: math.inf}[mode]
    norms = torch.stack([torch.linalg.vector_norm(piece, p) for piece in torch.split(g, list(sizes))])
    return torch.clamp(clip / (norms * scale + EPS32), max=1.0) * scale


def sgd_opts_ref(p, g, m, sizes, wd, lr_t, mom, nesterov, mode, clip, scale):
    """One step in float64.  wd, lr_t: one value per tensor.  Returns (p', m', d, u):
    g' = g coef (clamped to [-clip, clip] in mode 1),  d = g' + wd p,  m' = mom m + d,  u = d + mom m' (Nesterov) or m',
    p' = p - lr_t u."""
    p, g, m = p.to(F64), g.to(F64), m.to(F64)
    gs = g * per_tensor(opts_coef(g, sizes, mode, clip, scale), sizes, p)
    if mode == VALUE:
        gs = gs.clamp(-clip, clip)
    d = gs + per_tensor(wd, sizes, p) * p
    m1 = mom * m + d
    u = d + mom * m1 if nesterov else m1
    return p - per_tensor(lr_t, sizes, p) * u, m1, d, u


def norm_eps(n, mode, u):
    """Relative error bound of a tensor's coefficient before `* grad_scale` (the derivation: test_step_opts_abi_vs_float64)."""
    chunks = -(-n // R.CHUNK)
    if mode == L2:
        return (R.sumsq_depth(chunks) / 2 + 4) * u
    if mode == L1:
        return (R.sumsq_depth(chunks) - 1 + 3) * u
    if mode == INF:
        return 3 * u
    return 0.0


def sgd_opts_bounds(p, g, m, sizes, wd, lr_t, mom, nesterov, mode, clip, scale, u):
    """Per-element bounds (e_p, e_m) of the fp32 kernel's error on (p', m') of sgd_opts_ref; derivation in the docstring of
    tests/test_gpu_solver_options.py::test_step_opts_abi_vs_float64."""
    p, g, m = p.to(F64), g.to(F64), m.to(F64)
    p1, m1, d, upd = sgd_opts_ref(p, g, m, sizes, wd, lr_t, mom, nesterov, mode, clip, scale)
    wp = (per_tensor(wd, sizes, p) * p).abs()
    gc = (d - per_tensor(wd, sizes, p) * p).abs()          # |g'|
    eps_c = per_tensor([norm_eps(n, mode, u) for n in sizes], sizes, p)
    e_d = eps_c * gc + 4 * u * (gc + wp)
    e_m = e_d + 4 * u * (mom * m).abs()
    e_u = e_m
    if nesterov:
        e_u = e_d + mom * e_m + 2 * u * (mom * m1).abs() + u * d.abs()
    lr = per_tensor(lr_t, sizes, p)
    e_p = lr * e_u + 2 * u * (p.abs() + lr * upd.abs())
    return e_p, e_m


def propagate(e_p, e_m, wd_el, lr_el, mom, nesterov):
    """First-order error of (p', m') that errors (e_p, e_m) of the step's inputs cause (the gradient factor does not depend on
    p or m): d moves by wd e_p, m' by mom e_m + wd e_p, u as the step forms it, p' by e_p + lr err(u)."""
    e_d = wd_el * e_p
    e_m1 = mom * e_m + e_d
    e_u = e_d + mom * e_m1 if nesterov else e_m1
    return e_p + lr_el * e_u, e_m1


# ---- the small module of the FlatSGD tests and of tests/golden/solver_options_golden.npz ----------------------------------
# (name, shape) in parameter order: a conv with bias, a normalisation layer, a linear layer, a 75 000-element weight (two chunks)
NET_PARAMS = [("conv.weight", (8, 3, 3, 3)), ("conv.bias", (8,)), ("gn.weight", (8,)), ("gn.bias", (8,)),
              ("fc.weight", (5, 16)), ("fc.bias", (5,)), ("big.weight", (250, 300))]
NET_STEPS = 3
NET_MAX_ITER = 10
# SOLVER keys common to the option sets; the schedule is the half-cosine without warm-up, so that both rates move every step
NET_SOLVER = {"BASE_LR": 0.1, "MOMENTUM": 0.9, "WEIGHT_DECAY": 1e-4, "WEIGHT_DECAY_NORM": 0.0, "WEIGHT_DECAY_BIAS": 1e-3,
              "BIAS_LR_FACTOR": 2.0, "NESTEROV": True, "MAX_ITER": NET_MAX_ITER, "WARMUP_ITERS": 0,
              "LR_SCHEDULER_NAME": "WarmupCosineLR", "BASE_LR_END": 0.0}
NET_CASES = {"value": {"CLIP_TYPE": "value", "CLIP_VALUE": 0.02, "NORM_TYPE": 2.0},
             "l1": {"CLIP_TYPE": "norm", "CLIP_VALUE": 1.0, "NORM_TYPE": 1.0},
             "inf": {"CLIP_TYPE": "norm", "CLIP_VALUE": 0.05, "NORM_TYPE": float("inf")}}


COSINE_RUNS = [(1000, 100), (777, 50)]     # (MAX_ITER, WARMUP_ITERS) of the fixture's plain WarmupCosineLR runs
COSINE_BASE_LR = 0.01


def build_net(norm_cls, conv_cls=torch.nn.Conv2d, linear_cls=torch.nn.Linear):
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = conv_cls(3, 8, 3)
            self.gn = norm_cls(2, 8)
            self.fc = linear_cls(16, 5)
            self.big = linear_cls(300, 250, bias=False)

    net = Net()
    assert [(k, tuple(v.shape)) for k, v in net.named_parameters()] == NET_PARAMS
    with torch.no_grad():
        for (_, p), v in zip(net.named_parameters(), net_values(0)):   # norm weights of 1 and biases of 0 would hide a wrong decay
            p.copy_(v)
    return net


def net_values(seed, scale=None):
    """One seeded fp32 tensor per parameter; `scale`: per-parameter factors."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = [torch.randn(shape, generator=g) for _, shape in NET_PARAMS]
    return out if scale is None else [v * s for v, s in zip(out, scale)]


def net_grads(step):
    """Gradients of step `step`: magnitudes chosen so that each option set clips some tensors (or elements) and not others."""
    return net_values(1 + step, scale=[0.01, 0.3, 0.02, 0.002, 0.05, 1.0, 0.001])


def big_index():
    """The elements of the 75 000-element weight that the fixture keeps: both ends, 64 on each side of the chunk boundary (tensor
    element CHUNK), and every 97th."""
    n = 75000
    idx = set(range(64)) | set(range(n - 64, n)) | set(range(R.CHUNK - 64, R.CHUNK + 64)) | set(range(0, n, 97))
    return torch.tensor(sorted(idx))


def kept(t):
    """A tensor as the fixture stores it: flat, the large one reduced to big_index()."""
    t = t.reshape(-1)
    return t[big_index().to(t.device)] if t.numel() == 75000 else t
