"""FrozenBN on the training path and BACKBONE.FREEZE_AT on the device (u2seg_amd/layers/frozen.py, csrc/frozen.hip,
modeling/backbone.py ResNet.freeze; contract: DESIGN.md section 24, restated in float64 by tests/frozen_bn_refs.py).

Layer level, through Conv2d + FrozenBatchNorm2d, every element of every output, none masked, in the two modes of
tests/test_gpu_conv_float64.py:

A. exact: small-integer x, w, g, residual; s in +-2^k (negative ones included) and integer t, so W' = w s, every product and every
   partial sum are integers; sum |term| < 2^24 is asserted, so the fp32 sums are exact in any order.  out, dx, the residual's
   gradient and dw (through .grad and through a FlatSGD arena slot) must equal the exact values bit for bit, and the training
   output must equal the same module's torch.no_grad() output bit for bit.
B. real: activation-like inputs, random buffers; s, t are read from eval_scale_shift() on the device, W' is computed from the
   contract on the CPU.  The kernel's only error is that of adding L terms in fp32, E = (L + 2) 2^-24 sum |term|
   (float64_refs.fp32_sum_bound): bf16 outputs lie in [RNE_bf16(ref - E), RNE_bf16(ref + E)] with the second rounding and the
   ReLU applied to both ends; dw = s dW' lies within |s| E + 2^-24 |ref| (the scaling's one rounding).  No threshold comes from
   the code under test; the largest |err| / bound is printed as information.

Block and model level: the two fixture blocks against the same float64 layers, teacher-forced on the stored bf16 intermediates;
the fine-tune config and a SyncBN model with a frozen prefix as full models through two optimizer steps."""
import os

import numpy as np
import pytest
import torch

from tests import float64_refs as R
from tests import frozen_bn_refs as FR
from tests.test_gpu_conv_float64 import big_share, check_bf16, dev_act, host_act

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
MODES = ["exact", "real"]

# (geom, residual, relu): B = 2
LAYERS = [
    (R.g3(2, 12, 20, 64, 64, 3, 1), False, True),
    (R.g3(2, 12, 20, 64, 64, 3, 2), False, True),
    (R.g3(2, 13, 21, 64, 64, 3, 2), False, True),
    (R.g3(2, 12, 20, 64, 256, 1, 1), True, True),
    (R.g3(2, 12, 20, 256, 64, 1, 1), False, True),
    (R.g3(2, 12, 20, 128, 256, 1, 2), False, False),
    (R.g3(2, 12, 20, 64, 48, 3, 1), False, False),   # padded output channels: the pads must stay 0
]
IDS = ["%dx%d_%d-%d_s%d_%dx%d%s%s" % (g[5], g[6], g[3], g[4], g[7], g[1], g[2], "_res" if res else "", "_relu" if relu else "")
       for g, res, relu in LAYERS]


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()
    return functional


def report(name, what, value):
    print("FROZEN64 %s | %s | %.4g" % (name, what, value))


def make_layer(geom, mode, g):
    """Conv2d + FrozenBatchNorm2d on the device with the case's weights and buffers -> (module, s, t as the device computes them,
    float64 on the CPU)."""
    from u2seg_amd.layers.modules import Conv2d, FrozenBatchNorm2d

    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    if mode == "exact":
        norm = FrozenBatchNorm2d(cout, eps=0.0)
        scale = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.5, -0.5])[torch.randint(0, 6, (cout,), generator=g)]
        scale[0], scale[1] = -2.0, 0.5
        norm.weight.copy_(scale)
        norm.bias.copy_(torch.randint(-32, 33, (cout,), generator=g).float())
        norm.running_mean.zero_()
        norm.running_var.fill_(1.0)
    else:
        norm = FrozenBatchNorm2d(cout)
        norm.weight.copy_(0.5 + torch.rand(cout, generator=g))
        norm.weight[cout // 3] *= -1.0
        norm.bias.copy_(0.3 * torch.randn(cout, generator=g))
        norm.running_mean.copy_(0.2 * torch.randn(cout, generator=g))
        norm.running_var.copy_(0.5 + torch.rand(cout, generator=g))
    conv = Conv2d(cin, cout, kh, stride=stride, padding=ph, bias=False, norm=norm).to(DEV)
    conv.train()
    s, t = conv.norm.eval_scale_shift()
    assert s.dtype == torch.float32 and t.dtype == torch.float32
    s, t = s.to(F64).cpu(), t.to(F64).cpu()
    if mode == "exact":
        assert torch.equal(s, scale.to(F64)) and torch.equal(t, norm.bias.to(F64).cpu()) and bool((s < 0).any())
    return conv, s, t


def check_dw(name, got, ref_dwf, a_dwf, s, m, mode):
    """dw = s dW' (fp32) against float64: equal (exact), or within |s| E + 2^-24 |ref| (real)."""
    got = got.to(F64).cpu()
    sv = s.view(-1, 1, 1, 1)
    ref = sv * ref_dwf
    if mode == "exact":
        assert 2 * float(a_dwf.max()) < R.TWO24 and 2 * float((sv.abs() * a_dwf).max()) < R.TWO24, name
        bound = torch.zeros_like(ref)
    else:
        bound = sv.abs() * R.fp32_sum_bound(m, a_dwf) + R.U24 * ref.abs()
        err = (got - ref).abs()
        report(name, "max |err| / bound", float((err[bound > 0] / bound[bound > 0]).max()))
    bad = ((got - ref).abs() > bound) | ~torch.isfinite(got)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements beyond the bound; first at %s: got %r, ref %r, bound %r" % (
            name, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i]), float(bound[i])))


def layer_case(geom, residual, mode):
    """Operands of one case (float64 holding bf16 values; w holds fp32 values)."""
    x, w, _bias, gy, old = R.conv_operands(geom, mode)
    if mode == "real":
        # the master weights are fp32, not bf16 values: the fold rounds the product, not the factors
        g = torch.Generator().manual_seed(geom[3] * 131 + geom[4])
        w = (w * (1 + 2.0 ** -9 * torch.rand(w.shape, generator=g, dtype=F64))).float().to(F64)
    return x, w, gy, (old if residual else None)


def run_frozen_layer(F, geom, residual, relu, mode, arena):
    """One layer through Conv2d.forward under autograd; arena: the weight's gradient goes into a FlatSGD slot, else to .grad.
    Returns the measured (out, dx, dr, dw) on the CPU with the module and the references' ingredients."""
    from u2seg_amd.solver.build import FlatSGD

    b, h, w_, cin, cout, kh, kw, stride, ph, pw = geom
    g = torch.Generator().manual_seed(1234 + sum(geom))
    x, w, gy, old = layer_case(geom, residual, mode)
    conv, s, t = make_layer(geom, mode, g)
    with torch.no_grad():
        conv.weight.copy_(w.float())
    opt = FlatSGD(conv, lr=0.1) if arena else None
    if opt is not None:
        opt.zero_grad()
    xd = dev_act(x).requires_grad_(True)
    rd = dev_act(old).requires_grad_(True) if old is not None else None
    out = conv(xd, residual=rd, relu=relu)
    assert out.requires_grad and out.grad_fn is not None
    out.backward(dev_act(gy))
    F.join_all_streams()
    if arena:
        assert conv.weight._u2_grad.data_ptr() == conv.weight.grad.data_ptr()
    with torch.no_grad():
        # the same module without a graph: the folded inference path (the accumulating epilogue where a residual is owned)
        plain = conv(xd.detach(), residual=rd.detach().clone() if rd is not None else None, relu=relu,
                     residual_owned=rd is not None)
    assert torch.equal(out, plain), "training and no_grad outputs differ"
    return dict(conv=conv, opt=opt, s=s, t=t, x=x, w=w, gy=gy, old=old, out=out, xd=xd, rd=rd)


def check_frozen_layer(F, geom, residual, relu, mode, arena, name):
    b, h, w_, cin, cout, kh, kw, stride, ph, pw = geom
    ho, wo = R.conv_out_size(h, w_, kh, kw, stride, ph, pw)
    m, taps = b * ho * wo, kh * kw
    r = run_frozen_layer(F, geom, residual, relu, mode, arena)
    wf = FR.fold(r["w"], r["s"])                 # W' from the contract, on the CPU
    if mode == "exact":
        assert torch.equal(wf, r["w"] * r["s"].view(-1, 1, 1, 1))
    # exact mode: s = +-1/2 makes the terms multiples of 1/2 - one more bit, so the precondition sum |term| < 2^24 is asked of 2 A
    amul = 2.0 if mode == "exact" else 1.0
    y, a = R.conv_fwd_ref(r["x"], wf, stride, ph, pw, bias=r["t"])
    if mode == "exact" and taps * cin >= 32:
        assert big_share(y) > 0.25, (name, big_share(y))
    out, pad = host_act(r["out"], cout)
    assert pad == 0.0, name
    check_bf16(name + " fwd", out, y, a * amul, taps * cin, mode, relu=relu, old=r["old"])
    # the backward kernels read the STORED output's sign
    dz = r["gy"] * (out > 0) if relu else r["gy"]
    if residual:
        dr, pad = host_act(r["rd"].grad, cout)
        assert pad == 0.0 and torch.equal(dr, dz), name + " residual gradient"
    dx_ref, dx_a = R.conv_dgrad_ref(dz, wf, (h, w_), stride, ph, pw)
    dx, pad = host_act(r["xd"].grad, cin)
    assert pad == 0.0, name
    check_bf16(name + " dgrad", dx, dx_ref, dx_a * amul, taps * cout, mode)
    dwf, dwa = R.conv_wgrad_ref(r["x"], dz, kh, kw, stride, ph, pw)
    check_dw(name + " dw", r["conv"].weight.grad, dwf, dwa, r["s"], m, mode)
    for buf in ("weight", "bias", "running_mean", "running_var"):
        assert getattr(r["conv"].norm, buf).grad is None and not getattr(r["conv"].norm, buf).requires_grad
    return r, dz


@pytest.mark.parametrize("arena", [False, True], ids=["grad", "arena"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom,residual,relu", LAYERS, ids=IDS)
def test_frozen_layer(F, geom, residual, relu, mode, arena):
    check_frozen_layer(F, geom, residual, relu, mode, arena, "%s %s %s" % (geom, mode, "arena" if arena else "grad"))


@pytest.mark.parametrize("geom,residual,relu", [LAYERS[0], LAYERS[3]], ids=[IDS[0], IDS[3]])
def test_two_backward_calls_before_one_step(F, geom, residual, relu):
    """The slot holds the sum of both scaled gradients (exact mode: the integer sum, bit for bit)."""
    b, h, w_, cin, cout, kh, kw, stride, ph, pw = geom
    r, dz1 = check_frozen_layer(F, geom, residual, relu, "exact", True, "two backward calls, first")
    conv = r["conv"]
    first = conv.weight.grad.to(F64).cpu().clone()
    g = torch.Generator().manual_seed(99)
    gy2 = R.ints(r["gy"].shape, 3, g)
    xd = dev_act(r["x"]).requires_grad_(True)
    rd = dev_act(r["old"]) if residual else None
    out = conv(xd, residual=rd, relu=relu)
    out.backward(dev_act(gy2))
    F.join_all_streams()
    o, _ = host_act(out, cout)
    dz2 = gy2 * (o > 0) if relu else gy2
    dwf, dwa = R.conv_wgrad_ref(r["x"], dz2, kh, kw, stride, ph, pw)
    second = r["s"].view(-1, 1, 1, 1) * dwf
    assert 2 * float((first.abs() + r["s"].abs().view(-1, 1, 1, 1) * dwa).max()) < R.TWO24
    assert float(second.abs().max()) > 0
    assert torch.equal(conv.weight.grad.to(F64).cpu(), first + second)
    # after a step the layouts follow the new weights: the next forward equals the no_grad path again
    r["opt"].step()
    out2 = conv(xd.detach().requires_grad_(True), residual=rd, relu=relu)
    with torch.no_grad():
        plain = conv(xd.detach(), residual=rd.clone() if rd is not None else None, relu=relu, residual_owned=rd is not None)
    assert torch.equal(out2, plain) and not torch.equal(out2, out)


# ---- the fold kernel's two layouts, read back ----
@pytest.mark.parametrize("cin,cp,cout,k", [(64, 64, 48, 3), (16, 32, 40, 3), (24, 32, 8, 1), (256, 256, 64, 1), (70, 96, 130, 1)],
                         ids=["3x3_64-48", "3x3_16of32-40", "1x1_24of32-8", "1x1_256-64", "1x1_70of96-130"])
def test_fold_layouts_read_back(F, cin, cp, cout, k):
    """u2_frozen_fold's output itself against W' from the contract on the CPU, bit for bit: the forward layout [N][T][Cp] and the
    data-gradient layout [Cp][T][Npad] with the taps reversed, with every pad - input channels Cin..Cp-1 and output channels
    N..Npad-1 - zero.  Shapes: Npad > N, Cin < Cp, Cin * T no multiple of 64, an odd number of 64-column chunks, two 64-channel
    row blocks with a partial third."""
    geom = R.g3(1, 4, 5, cin, cout, k, 1)
    g = torch.Generator().manual_seed(7 * cin + cout)
    conv, s, _t = make_layer(geom, "real", g)
    w = (torch.randn((cout, cin, k, k), generator=g) / (cin * k * k) ** 0.5).float()
    with torch.no_grad():
        conv.weight.copy_(w)
    x = torch.zeros((1, 4, 5, cp), dtype=BF16, device=DEV)
    x[..., :cin] = torch.randn((1, 4, 5, cin), generator=g).to(DEV)
    for _ in range(2):   # the second pass rewrites nothing (fresh entry), the layouts must still stand
        out = conv(x)
    assert out.grad_fn is not None
    entry = conv.__dict__["_u2_frozen_fold"]
    npad, taps = (cout + 31) // 32 * 32, k * k
    wf = FR.fold(w, s).reshape(cout, cin, taps)                      # [n][c][t]
    fwd = torch.zeros((cout, taps, cp), dtype=F64)
    fwd[:, :, :cin] = wf.permute(0, 2, 1)
    dgrad = torch.zeros((cp, taps, npad), dtype=F64)
    dgrad[:cin, :, :cout] = wf.flip(2).permute(1, 2, 0)
    assert tuple(entry.fwd.shape) == tuple(fwd.shape) and tuple(entry.dgrad.shape) == tuple(dgrad.shape)
    assert torch.equal(entry.fwd.to(F64).cpu(), fwd)
    assert torch.equal(entry.dgrad.to(F64).cpu(), dgrad)
    assert float(wf.abs().min()) > 0   # no weight is zero by accident: the zero pads above are the kernel's


# ---- the trainable stem behind a FrozenBN ----
def _frozen_stem(g):
    from u2seg_amd.modeling.backbone import BasicStem

    stem = BasicStem(3, 64, norm="FrozenBN")
    n = stem.conv1.norm
    n.weight.copy_(0.5 + torch.rand(64, generator=g))
    n.weight[::5] *= -1.0
    n.bias.copy_(0.3 * torch.randn(64, generator=g))
    n.running_mean.copy_(0.2 * torch.randn(64, generator=g))
    n.running_var.copy_(0.5 + torch.rand(64, generator=g))
    with torch.no_grad():
        stem.conv1.weight.copy_(torch.randn((64, 3, 7, 7), generator=g) * 0.01)
    return stem.to(DEV).train()


def test_trainable_stem_behind_frozen_bn(F):
    """BasicStem with FrozenBN under autograd (NORM FrozenBN, FREEZE_AT 0).  Pixels are integers and mean 0 / std 1, so the canvas
    is exact in bf16.  The output equals the no_grad path's and affine_act + max_pool_3x3_s2 bit for bit.  With integer dy (a
    pixel lies in at most four windows: the routed sums are exact) the node's dx must equal bf16(fp32(s * routed dy)) under the
    stored activation's mask, bit for bit - the routing taken from the unfused max pool's backward.  The stem weight's gradient
    is the fp32 sum over B Ho Wo outputs of dx times canvas: within E = (L + 2) 2^-24 sum |term| of float64."""
    g = torch.Generator().manual_seed(11)
    stem = _frozen_stem(g)
    imgs = [torch.randint(0, 256, (3, 50, 70), generator=g, dtype=torch.uint8).to(DEV),
            torch.randint(0, 256, (3, 64, 61), generator=g, dtype=torch.uint8).to(DEV)]
    mean, std = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
    hw = (64, 96)
    out = stem(imgs, mean, std, hw)
    assert out.requires_grad and out.grad_fn is not None
    with torch.no_grad():
        plain = stem(imgs, mean, std, hw)
        y, _ = F.stem_conv(stem.conv1.weight, imgs, mean, std, *hw)
        s, t = (v.float().contiguous() for v in stem.conv1.norm.eval_scale_shift())
        act = F.affine_act(y, s, t, None, True)
    assert bool((s < 0).any()) and torch.equal(out, plain)
    leaf = act.clone().requires_grad_(True)
    pooled = F.max_pool_3x3_s2(leaf)
    assert torch.equal(out, pooled.detach())
    dy = torch.randint(-4, 5, tuple(out.shape), generator=g).to(BF16).to(DEV)
    pooled.backward(dy)
    routed = leaf.grad.float()                                  # integer sums of at most four integers: exact
    assert float(routed.abs().max()) <= 16
    expect = ((s.view(1, 1, 1, -1) * routed) * (act > 0)).to(BF16)   # one fp32 product, one rounding to bf16
    # the node alone, on y as a leaf
    yl = y.clone().requires_grad_(True)
    alone = F.affine_relu_max_pool_train(yl, s, t)
    assert torch.equal(alone, out)
    alone.backward(dy)
    assert torch.equal(yl.grad, expect)
    assert float((yl.grad != 0).double().mean()) > 0.02
    # through the module: the weight gradient of the stem conv under that dx
    out.backward(dy)
    F.join_all_streams()
    canvas, _ = R.stem_canvas([i.cpu() for i in imgs], mean.cpu(), std.cpu(), *hw)
    assert torch.equal(R.bf16_round(canvas), canvas)
    dx64, _ = host_act(expect, 64)
    ref, a = R.conv_wgrad_ref(canvas, dx64, 7, 7, 2, 3, 3)
    m = dx64.shape[0] * dx64.shape[2] * dx64.shape[3]
    bound = R.fp32_sum_bound(m, a)
    got = stem.conv1.weight.grad.to(F64).cpu()
    err = (got - ref).abs()
    report("stem", "max |err| / E of the weight gradient", float((err[bound > 0] / bound[bound > 0]).max()))
    assert bool((err <= bound).all()) and bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0
    for buf in stem.conv1.norm.buffers():
        assert buf.grad is None and not buf.requires_grad


def test_trainable_frozen_stem_without_the_fused_tail_is_an_error(F, monkeypatch):
    """No two-pass form of the FrozenBN stem tail under autograd exists: with the one-pass tail switched off the stem says so
    instead of running a pass without a graph."""
    g = torch.Generator().manual_seed(12)
    stem = _frozen_stem(g)
    imgs = [torch.randint(0, 256, (3, 32, 32), generator=g, dtype=torch.uint8).to(DEV)]
    monkeypatch.setattr(F, "STEM_TAIL_FUSE", False)
    with pytest.raises(NotImplementedError, match="one-pass stem tail"):
        stem(imgs, torch.zeros(3, device=DEV), torch.ones(3, device=DEV), (32, 32))
    with torch.no_grad():   # without a graph the two-pass form serves as before
        out = stem(imgs, torch.zeros(3, device=DEV), torch.ones(3, device=DEV), (32, 32))
    assert tuple(out.shape) == (1, 8, 8, 64)


# ---- block level: the fixture blocks, teacher-forced ----
@pytest.mark.parametrize("name", ["proj", "ident"])
def test_fixture_block_against_the_float64_layers(F, name):
    """This project's BottleneckBlock with the fixture's weights and buffers (tests/golden/freeze_block_golden.npz).  Every layer
    is compared with the float64 layer of tests/frozen_bn_refs.py evaluated on the STORED bf16 input of that layer (forward)
    and the stored bf16 gradient of its output (backward): the bound is one layer's, no error is carried along the chain."""
    from u2seg_amd.modeling.backbone import BottleneckBlock

    fx = np.load(os.path.join(ROOT, "tests", "golden", "freeze_block_golden.npz"))
    cin, cout, cb, stride = {"proj": (16, 32, 8, 2), "ident": (16, 16, 8, 1)}[name]
    blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, norm="FrozenBN")
    convs = {k: getattr(blk, k) for k in ("conv1", "conv2", "conv3", "shortcut") if getattr(blk, k) is not None}
    for k, conv in convs.items():
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(fx["%s.%s.weight" % (name, k)]))
        for buf in ("weight", "bias", "running_mean", "running_var"):
            getattr(conv.norm, buf).copy_(torch.from_numpy(fx["%s.%s.norm.%s" % (name, k, buf)]))
        conv.norm.eps = float(fx["%s.%s.norm.eps" % (name, k)])
    blk.to(DEV).train()
    seen = {}
    for k, conv in convs.items():
        def hook(mod, args, kwargs, output, k=k):
            output.retain_grad()
            seen[k] = (args[0], kwargs.get("residual"), output)
        conv.register_forward_hook(hook, with_kwargs=True)
    x = R.bf16_round(torch.from_numpy(fx[name + ".x"]).to(F64))
    gy = R.bf16_round(torch.from_numpy(fx[name + ".gy"]).to(F64))
    xd = dev_act(x).requires_grad_(True)
    y = blk(xd)
    y.backward(dev_act(gy))
    F.join_all_streams()
    cins = {"conv1": cin, "conv2": cb, "conv3": cb, "shortcut": cin}
    couts = {"conv1": cb, "conv2": cb, "conv3": cout, "shortcut": cout}
    dx_parts = {}
    for k, conv in convs.items():
        xin, res, out = seen[k]
        st, pad = conv.stride, conv.padding
        kk = conv.kernel_size[0]
        s, t = (v.to(F64).cpu() for v in conv.norm.eval_scale_shift())
        wf = FR.fold(conv.weight.detach().cpu(), s)
        xi, p0 = host_act(xin.detach(), cins[k])
        assert p0 == 0.0
        old = host_act(res.detach(), couts[k])[0] if res is not None else None
        relu = k in ("conv1", "conv2", "conv3")
        ref, a = R.conv_fwd_ref(xi, wf, st, pad, pad, bias=t)
        got, p1 = host_act(out.detach(), couts[k])
        assert p1 == 0.0
        check_bf16("%s %s fwd" % (name, k), got, ref, a, kk * kk * cins[k], "real", relu=relu, old=old)
        gout, _ = host_act(out.grad, couts[k])
        dz = gout * (got > 0) if relu else gout
        dwf, dwa = R.conv_wgrad_ref(xi, dz, kk, kk, st, pad, pad)
        m = dz.shape[0] * dz.shape[2] * dz.shape[3]
        check_dw("%s %s dw" % (name, k), conv.weight.grad, dwf, dwa, s, m, "real")
        dref, da = R.conv_dgrad_ref(dz, wf, xi.shape[2:], st, pad, pad)
        e = R.fp32_sum_bound(kk * kk * couts[k], da)
        if k in ("conv2", "conv3"):   # their input has one reader: its stored gradient is this layer's data gradient
            dgot, _ = host_act(xin.grad if xin.grad is not None else seen["conv1" if k == "conv2" else "conv2"][2].grad, cins[k])
            check_bf16("%s %s dgrad" % (name, k), dgot, dref, da, kk * kk * couts[k], "real")
        else:
            dx_parts[k] = (R.rne_bf16(dref - e), R.rne_bf16(dref + e), dz)
    # the block input is read by conv1 and by the shortcut (a conv, or the identity: its gradient is the tail's dz): autograd adds
    # the two bf16 gradients and rounds once more - monotone in both
    lo1, hi1, _ = dx_parts["conv1"]
    if "shortcut" in dx_parts:
        lo2, hi2, _ = dx_parts["shortcut"]
    else:
        dz3 = seen["conv3"][2]
        g3, _ = host_act(dz3.grad, cout)
        o3, _ = host_act(dz3.detach(), cout)
        lo2 = hi2 = g3 * (o3 > 0)
    lo, hi = R.rne_bf16(lo1 + lo2), R.rne_bf16(hi1 + hi2)
    dx, p = host_act(xd.grad, cin)
    assert p == 0.0
    bad = (dx < lo) | (dx > hi) | ~torch.isfinite(dx)
    assert not bool(bad.any()), "%s block input gradient: %d of %d elements outside the interval" % (name, int(bad.sum()), bad.numel())
    # against the reference's fp32 answer only as information (bf16 storage between the layers: no derived bound applies)
    yy, _ = host_act(y.detach(), cout)
    report(name, "max |y - reference fp32 y|", float((yy - torch.from_numpy(fx[name + ".y"]).to(F64)).abs().max()))


# ---- model level ----
def _build(config, opts):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_optimizer

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", config))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "MODEL.ROI_HEADS.NUM_CLASSES", 8] + list(opts))
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    return cfg, model, build_optimizer(cfg, model)


def _two_steps(F, config, opts, prefix=2):
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.layers.modules import BatchNorm2d, FrozenBatchNorm2d

    cfg, model, opt = _build(config, opts)
    batch = make_synthetic_batch(2, height=128, width=160, device=DEV, num_thing_classes=8)
    bu = model.backbone.bottom_up
    params = dict(model.named_parameters())
    trainable = {k for k, p in params.items() if p.requires_grad}
    frozen = set(params) - trainable
    assert trainable and bool(frozen) == (prefix > 0) and bu.frozen_prefix == prefix
    fbn = {"%s.%s" % (n, b): buf for n, m in model.named_modules() if isinstance(m, FrozenBatchNorm2d)
           for b, buf in m.named_buffers()}
    before = {k: v.detach().clone() for k, v in list(params.items()) + list(fbn.items())}
    res2 = {}

    def keep_first(mod, args, out):   # (returns None: a forward hook's return value would replace the module's output)
        res2.setdefault("out", out)

    bu.res2.register_forward_hook(keep_first)
    # step 1 by hand, to look at the gradients
    opt.zero_grad()
    losses = model(batch)
    assert len(losses) == 10 and all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(losses.values()).backward()
    F.join_all_streams()
    F.assert_no_deferred_gradients()
    if prefix >= 2:
        assert res2["out"].requires_grad is False and res2["out"].grad_fn is None
        assert not hasattr(res2["out"], "_u2_twin") and not hasattr(res2["out"], "_u2_tail")
    else:
        assert res2["out"].requires_grad
    for k in trainable:
        gr = params[k].grad
        assert gr is not None and bool(torch.isfinite(gr).all()), k
    for k in trainable:   # the tensors behind the frozen prefix really receive something
        if k.startswith("backbone.bottom_up."):
            assert bool((params[k].grad != 0).any()), k
    for k in frozen:
        assert params[k].grad is None and not hasattr(params[k], "_u2_grad"), k
    assert all(b.grad is None for b in fbn.values())
    opt.step()
    # step 2 through the trainer
    from u2seg_amd.engine import SimpleTrainer

    trainer = SimpleTrainer(model, opt)
    losses = trainer.run_step(batch)
    torch.cuda.synchronize()
    trainer.check_finite()
    assert len(losses) == 10
    F.assert_no_deferred_gradients()
    for k in frozen:
        assert torch.equal(params[k].detach(), before[k]), k
    for k, buf in fbn.items():
        assert torch.equal(buf, before[k]), k
    unchanged = [k for k in trainable if torch.equal(params[k].detach(), before[k])]
    assert not unchanged, unchanged
    return model, [m for m in model.modules() if isinstance(m, BatchNorm2d)]


def test_finetune_config_trains(F):
    model, bns = _two_steps(F, "u2seg_R50_800_finetune.yaml", [])
    assert bns == [] and model.backbone.bottom_up.frozen_prefix == 2


def test_frozenbn_with_nothing_frozen_trains(F):
    """FREEZE_AT 0: the stem trains through the fused affine + ReLU + pool node, every FrozenBN layer through the folded path
    (the stem weight must receive a gradient and move: _two_steps asserts it for every bottom-up tensor)."""
    model, bns = _two_steps(F, "u2seg_R50_800_finetune.yaml", ["MODEL.BACKBONE.FREEZE_AT", 0], prefix=0)
    assert bns == [] and model.backbone.bottom_up.stem.conv1.weight.requires_grad


def test_syncbn_with_frozen_prefix_trains(F):
    model, bns = _two_steps(F, "u2seg_R50_800.yaml", ["MODEL.BACKBONE.FREEZE_AT", 2])
    assert bns and model.backbone.bottom_up.frozen_prefix == 2
    # the unfrozen BatchNorm layers still update their running statistics
    for bn in bns:
        assert bn._updates == 2
        assert not torch.equal(bn.running_mean, torch.zeros_like(bn.running_mean))
        assert not torch.equal(bn.running_var, torch.ones_like(bn.running_var))
    assert int(bns[0].state_dict()["num_batches_tracked"]) == 2
