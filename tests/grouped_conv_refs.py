"""Float64 references of the grouped 3x3 convolution (u2_gconv3x3_fwd / _dgrad / _wgrad, include/u2seg_hip.h) with their
sum |term| companions, built per group from the dense references of tests/float64_refs.py on channel slices, the fold
W' = bf16(w * s) the kernels apply while they stage a filter, and the operand generator and case list of
tests/test_gpu_grouped_conv.py.  tests/test_grouped_conv_host.py checks the references against torch's conv2d(groups = G) and its
autograd in float64."""
import torch

from tests import float64_refs as R

F64 = torch.float64

# (C, groups): cg = 4, 8, 16, 32, 64, 32 (three super-groups: not a power of two), 8 at eight super-groups
CHANNELS = [(32, 8), (64, 8), (64, 4), (64, 2), (128, 2), (96, 3), (256, 32)]
SMALL_MAPS = [(2, 13, 19), (1, 1, 5)]   # ragged edges (stride 2: 7 x 10); a single row
LARGE_MAP = (2, 33, 47)                 # several pixel patches, several work-groups adding into one dw element
LARGE_CHANNELS = [(64, 8), (256, 32)]
CASES = [(c, g) + m for (c, g) in CHANNELS for m in SMALL_MAPS] + [(c, g) + LARGE_MAP for (c, g) in LARGE_CHANNELS]


def out_hw(h, w, stride):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def fold(w, s):
    """W'[n][c][t] = bf16_rne(fp32(w[n][c][t]) * fp32(s[n])): one fp32 multiply, one rounding (layers/frozen.py).  -> float64"""
    return (w.float() * s.float().view(-1, 1, 1, 1)).bfloat16().to(F64)


def _slices(c, groups):
    cg = c // groups
    return [slice(i * cg, (i + 1) * cg) for i in range(groups)]


def gconv_fwd_ref(x, w, groups, stride, bias=None):
    """x [B, C, H, W], w [C, C / groups, 3, 3] -> (y, A) [B, C, Ho, Wo]"""
    p = w.shape[2] // 2
    parts = [R.conv_fwd_ref(x[:, c], w[n], stride, p, p, None if bias is None else bias[n])
             for c, n in zip(_slices(x.shape[1], groups), _slices(w.shape[0], groups))]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)


def gconv_dgrad_ref(dy, w, groups, in_hw, stride):
    """dy [B, C, Ho, Wo] -> (dx, A) [B, C, H, W]"""
    p = w.shape[2] // 2
    parts = [R.conv_dgrad_ref(dy[:, n], w[n], in_hw, stride, p, p) for n in _slices(w.shape[0], groups)]
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)


def gconv_wgrad_ref(x, dy, groups, stride, k=3):
    """-> (dw, A) [N, C / groups, k, k]"""
    cs, ns = _slices(x.shape[1], groups), _slices(dy.shape[1], groups)
    parts = [R.conv_wgrad_ref(x[:, c], dy[:, n], k, k, stride, k // 2, k // 2) for c, n in zip(cs, ns)]
    return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)


def grouped_operands(case, stride, mode):
    """x [B, C, H, W], w [C, cg, 3, 3], bias [C], gy [B, C, Ho, Wo], scale [C], old [C, cg, 3, 3] as float64.
    "exact": small integers (amplitudes by float64_refs.exact_amp for sums of 9 cg terms), scale in {1, 2, -1, -2} (w * scale stays
    a small integer: the fold is exact), old integers.  "real": the generator of float64_refs.conv_operands (activation-like x,
    gy = N(0, 1) 2^-10), but w stays an fp32 value that is NOT a bf16 number, so that the kernels' own rounding is exercised;
    scale U(0.5, 2) fp32; old N(0, 1) fp32."""
    c, groups, b, h, wd = case
    cg = c // groups
    ho, wo = out_hw(h, wd, stride)
    g = torch.Generator().manual_seed((c * 7919 + groups * 104729 + b * 31 + h * 1009 + wd * 17 + stride) % (2 ** 31) + (mode == "real"))
    if mode == "exact":
        inside = float(R._cols(torch.ones((1, 1, h, wd), dtype=F64), 3, 3, stride, 1, 1).sum(1).mean())
        a_f = R.exact_amp(max(1, round(cg * inside)))
        x, w = R.ints((b, c, h, wd), a_f, g), R.ints((c, cg, 3, 3), a_f, g)
        bias = R.ints((c,), 16 * a_f, g)
        a_g = R.exact_amp(max(1, round(cg * inside * ho * wo / (h * wd))), a_f)
        gy = R.ints((b, c, ho, wo), a_g, g)
        scale = torch.tensor([1.0, 2.0, -1.0, -2.0], dtype=F64)[torch.randint(0, 4, (c,), generator=g)]
        old = R.ints((c, cg, 3, 3), 64, g)
        return x, w, bias, gy, scale, old
    assert mode == "real"
    k = 9 * cg
    mu = torch.tensor([0.0, 1.0, 4.0], dtype=F64)[torch.randint(0, 3, (c,), generator=g)]
    x = torch.relu(torch.randn((b, c, h, wd), generator=g, dtype=F64) + mu.view(1, c, 1, 1))
    x[:, 0] = 0
    flat = x[:, 1].reshape(-1).clone()
    flat[torch.randint(0, flat.numel(), (min(3, flat.numel()),), generator=g)] = 64.0
    x[:, 1] = flat.view(b, h, wd)
    w = torch.randn((c, cg, 3, 3), generator=g, dtype=F64) / k ** 0.5 + (torch.rand((c, 1, 1, 1), generator=g, dtype=F64) * 2 - 1) / k
    bias = torch.randn((c,), generator=g, dtype=F64) * 0.1
    gy = torch.randn((b, c, ho, wo), generator=g, dtype=F64) * 2.0 ** -10
    scale = torch.rand((c,), generator=g, dtype=F64) * 1.5 + 0.5
    old = torch.randn((c, cg, 3, 3), generator=g, dtype=F64)
    f32 = lambda t: t.float().to(F64)
    return R.bf16_round(x), f32(w), f32(bias), R.bf16_round(gy), f32(scale), f32(old)



# ---- the ResNeXt fixture blocks (tests/golden/resnext_block_golden.npz): a chain of layers with a running error bound ----
# The method of tests/frozen_bn_refs.py (a quantity is (value, e): the fp32 computation's value lies within e of the float64 value;
# a layer that sums L terms adds (L + 3) u A' to what it inherits), with grouped sums: L = 9 cg for the grouped layer.
U24 = R.U24
BLOCKS = {"proj": (32, 64, 32, 2), "ident": (64, 64, 32, 1)}   # name -> (in, out, bottleneck, stride); num_groups = 4
BLOCK_GROUPS = 4
BLOCK_CONVS = (("conv1", 1, False), ("conv2", BLOCK_GROUPS, True), ("conv3", 1, False), ("shortcut", 1, True))   # name, groups, strided


def chain_fwd(x, ex, wf, t, groups, stride):
    y, _ = gconv_fwd_ref(x, wf, groups, stride, bias=t)
    _, a = gconv_fwd_ref(x.abs() + ex, wf.abs(), groups, stride, bias=None if t is None else t.abs())
    inherit, _ = gconv_fwd_ref(ex, wf.abs(), groups, stride)
    return y, inherit + (wf[0].numel() + 3) * U24 * a


def chain_dgrad(dz, ez, wf, groups, in_hw, stride):
    dx, _ = gconv_dgrad_ref(dz, wf, groups, in_hw, stride)
    a, _ = gconv_dgrad_ref(dz.abs() + ez, wf.abs(), groups, in_hw, stride)
    inherit, _ = gconv_dgrad_ref(ez, wf.abs(), groups, in_hw, stride)
    return dx, inherit + (wf.shape[0] // groups * wf.shape[2] * wf.shape[3] + 3) * U24 * a


def chain_wgrad(x, ex, dz, ez, s, groups, stride, k):
    """dw = s * wgrad(x, dz) and its bound (s: float64 [N], or None for 1)."""
    dw, _ = gconv_wgrad_ref(x, dz, groups, stride, k)
    a, _ = gconv_wgrad_ref(x.abs() + ex, dz.abs() + ez, groups, stride, k)
    i1, _ = gconv_wgrad_ref(x.abs() + ex, ez, groups, stride, k)
    i2, _ = gconv_wgrad_ref(ex, dz.abs(), groups, stride, k)
    length = dz.shape[0] * dz.shape[2] * dz.shape[3]
    e = i1 + i2 + (length + 3) * U24 * a
    if s is None:
        return dw, e
    return s.view(-1, 1, 1, 1) * dw, s.abs().view(-1, 1, 1, 1) * e


def block_layers(fx, name, kind="frozen"):
    """The layers of fixture block `name` as float64: {conv: dict(w, groups, stride, s, t)}, s and t from the buffers in float64."""
    from tests import frozen_bn_refs as FR

    stride = BLOCKS[name][3]
    out = {}
    for cname, groups, strided in BLOCK_CONVS:
        key = "%s.%s.%s." % (kind, name, cname)
        if key + "weight" not in fx:
            continue
        n = {k: torch.from_numpy(fx[key + "norm." + k]).to(F64) for k in ("weight", "bias", "running_mean", "running_var")}
        s, t = FR.scale_shift64(n["weight"], n["bias"], n["running_mean"], n["running_var"], float(fx[key + "norm.eps"]))
        out[cname] = dict(w=torch.from_numpy(fx[key + "weight"]).to(F64), groups=groups, stride=stride if strided else 1, s=s, t=t)
    return out


def block_chain(layers, x, gy):
    """One ResNeXt BottleneckBlock (resnet.py:100-210, num_groups = 4) with FrozenBN in float64 with unrounded W' = w s:
    {name: (value, bound)} for y, dx and the convs' dw - frozen_bn_refs.block_chain with a grouped conv2.  Asserts that every ReLU decision is out of its bound's reach (the
    fixture's precondition: a mask that fp32 could decide the other way has no bounded gradient)."""
    z0 = torch.zeros_like(x)

    def fwd(k, v, e):
        lay = layers[k]
        return chain_fwd(v, e, lay["w"] * lay["s"].view(-1, 1, 1, 1), lay["t"], lay["groups"], lay["stride"])

    def bwd(k, g, eg, v, ev):
        """the conv's two gradients -> ((dw, e), (dx, e))"""
        lay = layers[k]
        wf = lay["w"] * lay["s"].view(-1, 1, 1, 1)
        return (chain_wgrad(v, ev, g, eg, lay["s"], lay["groups"], lay["stride"], wf.shape[2]),
                chain_dgrad(g, eg, wf, lay["groups"], v.shape[2:], lay["stride"]))

    a1, e1 = fwd("conv1", x, z0)
    h1 = a1.clamp(min=0)
    a2, e2 = fwd("conv2", h1, e1)
    h2 = a2.clamp(min=0)
    a3, e3 = fwd("conv3", h2, e2)
    sc, es = fwd("shortcut", x, z0) if "shortcut" in layers else (x, z0)
    z, ez = a3 + sc, e3 + es + U24 * (a3.abs() + sc.abs() + e3 + es)
    for pre, e in ((a1, e1), (a2, e2), (z, ez)):
        assert bool((pre.abs() > e).all()), "fixture precondition: a ReLU input lies within the fp32 error of zero"
    out = {"y": (z.clamp(min=0), ez)}
    dz = gy * (z > 0)
    zz = torch.zeros_like(dz)
    out["conv3.dweight"], (d2, g2) = bwd("conv3", dz, zz, h2, e2)
    d2, g2 = d2 * (a2 > 0), g2 * (a2 > 0)
    out["conv2.dweight"], (d1, g1) = bwd("conv2", d2, g2, h1, e1)
    d1, g1 = d1 * (a1 > 0), g1 * (a1 > 0)
    out["conv1.dweight"], (dx, gx) = bwd("conv1", d1, g1, x, z0)
    if "shortcut" in layers:
        out["shortcut.dweight"], (ds, gs) = bwd("shortcut", dz, zz, x, z0)
    else:
        ds, gs = dz, zz
    out["dx"] = (dx + ds, gx + gs + U24 * (dx.abs() + ds.abs() + gx + gs))
    return out


# ---- the same blocks with BatchNorm in training mode (tests/golden/resnext_block_bn_<name>_golden.npz) ----
# Carried through a whole block, a worst-case bound of the BatchNorm backward pass (a projection with cancellation) comes out larger
# than the gradients, so the fixture records the reference's intermediates and every layer is held on ITS recorded input and ITS
# recorded output gradient: the bound is one layer's.  Only the forward pass is also carried along the chain (block_forward_bn).
#
# y = conv(x) (within ey), per channel over the M = B H W values: mu = mean y, v = mean (y - mu)^2, r = (v + eps)^-1/2,
# xh = (y - mu) r, o = gamma xh + beta.  An fp32 evaluation - in any order of the sums, and in either form of the affine step
# (gamma xh + beta, or y (gamma r) + (beta - mu gamma r) as ATen's CPU kernel has it) - differs from the float64 value by the
# inherited error (each input's error times the magnitude of the partial derivative, taken at the perturbed point) plus the
# rounding of its own operations: a sum of M terms errs by at most (M + 2) u sum |term|, every other operation by u times the
# magnitude of its result; 6 u times the sum of the magnitudes of a step's intermediate terms covers its few operations.
def _mean(t):
    return t.mean((0, 2, 3), keepdim=True)


def bn_fwd(y, ey, gamma, beta, eps):
    """-> (o, eo, cache for bn_bwd)"""
    m = y.shape[0] * y.shape[2] * y.shape[3]
    ga, be = gamma.view(1, -1, 1, 1), beta.view(1, -1, 1, 1)
    mu = _mean(y)
    emu = _mean(ey) + (m + 2) * U24 * _mean(y.abs() + ey)
    d = y - mu
    ed = ey + emu + 2 * U24 * (y.abs() + mu.abs() + ey + emu)
    v = _mean(d * d)
    ev = _mean(2 * d.abs() * ed + ed * ed) + (m + 4) * U24 * _mean((d.abs() + ed) ** 2)
    assert bool((ev < 0.5 * (v + eps)).all()), "the variance is not resolved in fp32"
    r = (v + eps) ** -0.5
    er = r * ev / (2 * (v + eps - ev)) + 4 * U24 * r
    xh = d * r
    exh = ed * (r + er) + d.abs() * er + 2 * U24 * d.abs() * r
    o = ga * xh + be
    eo = ga.abs() * ((ey + emu) * (r + er) + d.abs() * er) \
        + 6 * U24 * (ga.abs() * (r + er) * (y.abs() + mu.abs() + ey + emu) + be.abs())
    return o, eo, (ga, r, er, xh, exh, m)


def bn_bwd(g, eg, cache):
    """dy = gamma r (g - mean g - xh mean(g xh)) and its bound."""
    ga, r, er, xh, exh, m = cache
    m1, m2 = _mean(g), _mean(g * xh)
    em1 = _mean(eg) + (m + 2) * U24 * _mean(g.abs() + eg)
    em2 = _mean(eg * (xh.abs() + exh) + g.abs() * exh) + (m + 3) * U24 * _mean((g.abs() + eg) * (xh.abs() + exh))
    t = g - m1 - xh * m2
    et = eg + em1 + exh * (m2.abs() + em2) + xh.abs() * em2
    mag = g.abs() + m1.abs() + (xh * m2).abs()
    dy = ga * r * t
    edy = ga.abs() * ((r + er) * et + er * t.abs()) + 6 * U24 * ga.abs() * (r + er) * (mag + et)
    return dy, edy


def bn_block_layers(fx, name):
    """{conv: dict(w, groups, stride, gamma, beta, eps)} of the BN fixture block `name`, float64."""
    stride = BLOCKS[name][3]
    out = {}
    for cname, groups, strided in BLOCK_CONVS:
        key = "bn.%s.%s." % (name, cname)
        if key + "weight" not in fx:
            continue
        out[cname] = dict(w=torch.from_numpy(fx[key + "weight"]).to(F64), groups=groups, stride=stride if strided else 1,
                          gamma=torch.from_numpy(fx[key + "norm.weight"]).to(F64), beta=torch.from_numpy(fx[key + "norm.bias"]).to(F64),
                          eps=float(fx[key + "norm.eps"]))
    return out


def bn_layer(lay, xin, ex):
    """conv + training-mode BatchNorm of one layer on xin (within ex) -> (o, eo, cache)"""
    y, ey = chain_fwd(xin, ex, lay["w"], None, lay["groups"], lay["stride"])
    return bn_fwd(y, ey, lay["gamma"], lay["beta"], lay["eps"])


def bn_layer_bwd(lay, cache, xin, g):
    """The layer's gradients for the gradient g of its norm's output (exact: a recorded value), xin exact too
    -> ((dw, e), (dx, e))"""
    dy, edy = bn_bwd(g, torch.zeros_like(g), cache)
    z = torch.zeros_like(xin)
    return (chain_wgrad(xin, z, dy, edy, None, lay["groups"], lay["stride"], lay["w"].shape[2]),
            chain_dgrad(dy, edy, lay["w"], lay["groups"], xin.shape[2:], lay["stride"]))


def block_forward_bn(layers, x):
    """The block's output carried along the chain from x -> (y, ey)"""
    z0 = torch.zeros_like(x)
    a1, e1, _ = bn_layer(layers["conv1"], x, z0)
    a2, e2, _ = bn_layer(layers["conv2"], a1.clamp(min=0), e1)
    a3, e3, _ = bn_layer(layers["conv3"], a2.clamp(min=0), e2)
    sc, es = bn_layer(layers["shortcut"], x, z0)[:2] if "shortcut" in layers else (x, z0)
    z = a3 + sc
    return z.clamp(min=0), e3 + es + U24 * (a3.abs() + sc.abs() + e3 + es)
