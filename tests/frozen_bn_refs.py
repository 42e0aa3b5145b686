"""float64 restatement of conv -> FrozenBatchNorm2d (-> + residual) (-> ReLU), shared by tests/test_freeze_host.py (against the
reference's fp32 known answers, tests/golden/freeze_block_golden.npz) and tests/test_gpu_frozen_bn.py (against the device).

The contract: s = weight * rsqrt(running_var + eps), t = bias - running_mean * s,
W' = bf16(fp32(w) * s[co]) (the product rounded once to fp32, once to bf16), out = bf16(relu?(sum x W' + t)) or, with a residual
r, bf16(relu?(bf16(sum x W' + t) + r)); dz = g [out > 0], dr = dz, dx = dgrad(dz, W'), dw[co] = s[co] * wgrad(x, dz)[co].

Every sum is formed by tests/float64_refs.py (unfold + matmul in float64 with its magnitude sum A = sum |term|); what differs
between the two users is only whether W' is rounded (the device) or not (the reference applies the affine map in fp32)."""
import torch

from tests import float64_refs as R

F64 = torch.float64
U24 = R.U24


def scale_shift64(weight, bias, mean, var, eps):
    s = weight.to(F64) * torch.rsqrt(var.to(F64) + float(eps))
    return s, bias.to(F64) - mean.to(F64) * s


def fold(w, s, rounded=True):
    """W' as float64.  rounded: the contract's two roundings from the fp32 operands (s as the device holds it); else w * s in
    float64 (conv followed by y * s is the same sum)."""
    if rounded:
        return (w.float() * s.float().view(-1, 1, 1, 1)).bfloat16().to(F64)
    return w.to(F64) * s.to(F64).view(-1, 1, 1, 1)


# ---- a chain of layers with a running error bound (the host test's comparison with fp32 known answers) ----
# A quantity is (value, e): the fp32 computation's value lies within e of the float64 value.  A layer that sums L terms adds
# (L + 3) u A' to what it inherits - (L - 1) additions of partial sums of magnitude <= A' plus the affine map's multiply and add, one
# spare for second-order terms - where A' = sum |term| with |input| + e in place of |input|; the inherited part is the same
# linear map applied to e with |W'|.
def chain_fwd(x, ex, wf, t, stride, pad):
    y, _ = R.conv_fwd_ref(x, wf, stride, pad, pad, bias=t)
    _, a = R.conv_fwd_ref(x.abs() + ex, wf.abs(), stride, pad, pad, bias=t.abs())
    inherit, _ = R.conv_fwd_ref(ex, wf.abs(), stride, pad, pad)
    length = wf[0].numel()
    return y, inherit + (length + 3) * U24 * a


def chain_dgrad(dz, ez, wf, in_hw, stride, pad):
    dx, _ = R.conv_dgrad_ref(dz, wf, in_hw, stride, pad, pad)
    a, _ = R.conv_dgrad_ref(dz.abs() + ez, wf.abs(), in_hw, stride, pad, pad)
    inherit, _ = R.conv_dgrad_ref(ez, wf.abs(), in_hw, stride, pad, pad)
    length = wf.shape[0] * wf.shape[2] * wf.shape[3]
    return dx, inherit + (length + 3) * U24 * a


def chain_wgrad(x, ex, dz, ez, s, kh, kw, stride, pad):
    """dw = s * wgrad(x, dz) and its bound."""
    dw, _ = R.conv_wgrad_ref(x, dz, kh, kw, stride, pad, pad)
    a, _ = R.conv_wgrad_ref(x.abs() + ex, dz.abs() + ez, kh, kw, stride, pad, pad)
    i1, _ = R.conv_wgrad_ref(x.abs() + ex, ez, kh, kw, stride, pad, pad)
    i2, _ = R.conv_wgrad_ref(ex, dz.abs(), kh, kw, stride, pad, pad)
    length = dz.shape[0] * dz.shape[2] * dz.shape[3]
    sa = s.abs().view(-1, 1, 1, 1)
    return s.view(-1, 1, 1, 1) * dw, sa * (i1 + i2 + (length + 3) * U24 * a)


def block_layers(fx, name):
    """The layers of one fixture block: {conv: (w, s, t, stride, pad)} as float64 (s, t from the buffers in float64)."""
    cin, cout, cb, stride = {"proj": (16, 32, 8, 2), "ident": (16, 16, 8, 1)}[name]
    out = {}
    for cname, st, pad in (("conv1", 1, 0), ("conv2", stride, 1), ("conv3", 1, 0), ("shortcut", stride, 0)):
        key = "%s.%s." % (name, cname)
        if key + "weight" not in fx:
            continue
        n = {k: torch.from_numpy(fx[key + "norm." + k]) for k in ("weight", "bias", "running_mean", "running_var")}
        s, t = scale_shift64(n["weight"], n["bias"], n["running_mean"], n["running_var"], float(fx[key + "norm.eps"]))
        out[cname] = (torch.from_numpy(fx[key + "weight"]).to(F64), s, t, st, pad)
    return out


def block_chain(layers, x, gy):
    """One BottleneckBlock (resnet.py:100-210) in float64 with unrounded W': {name: (value, bound)} for y, dx and the convs' dw.
    Asserts that every ReLU decision is out of its bound's reach (a precondition on the fixture: a mask that fp32 could decide
    the other way has no bounded gradient)."""
    z0 = torch.zeros_like(x)
    wf = {k: fold(v[0], v[1], rounded=False) for k, v in layers.items()}
    fwd = lambda k, v, e: chain_fwd(v, e, wf[k], layers[k][2], layers[k][3], layers[k][4])
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
    dgrad = lambda k, d, e, hw: chain_dgrad(d, e, wf[k], hw, layers[k][3], layers[k][4])
    wgrad = lambda k, v, ev, d, ed: chain_wgrad(v, ev, d, ed, layers[k][1], wf[k].shape[2], wf[k].shape[3], layers[k][3], layers[k][4])
    zz = torch.zeros_like(dz)
    out["conv3.dweight"] = wgrad("conv3", h2, e2, dz, zz)
    d2, g2 = dgrad("conv3", dz, zz, h2.shape[2:])
    d2, g2 = d2 * (a2 > 0), g2 * (a2 > 0)
    out["conv2.dweight"] = wgrad("conv2", h1, e1, d2, g2)
    d1, g1 = dgrad("conv2", d2, g2, h1.shape[2:])
    d1, g1 = d1 * (a1 > 0), g1 * (a1 > 0)
    out["conv1.dweight"] = wgrad("conv1", x, z0, d1, g1)
    dx, gx = dgrad("conv1", d1, g1, x.shape[2:])
    if "shortcut" in layers:
        out["shortcut.dweight"] = wgrad("shortcut", x, z0, dz, zz)
        ds, gs = dgrad("shortcut", dz, zz, x.shape[2:])
    else:
        ds, gs = dz, zz
    out["dx"] = (dx + ds, gx + gs + U24 * (dx.abs() + ds.abs() + gx + gs))
    return out
