"""RESNETS.NUM_GROUPS on the device: the grouped Conv2d layer under training BN, FrozenBN and on the folded eval path, the
ResNeXt fixture blocks (tests/golden/resnext_block_golden.npz) layer by layer, both against the float64 references of
tests/grouped_conv_refs.py, and the reduced ResNeXt u2seg model: it trains, its grouped weights receive gradients in the
optimizer's arena, it repeats its bits at inference, the fine-tune recipe trains; the default model never calls the new entries."""
import json
import os

import numpy as np
import pytest
import torch

from tests import float64_refs as R
from tests import grouped_conv_refs as G
from tests.test_gpu_conv_float64 import check_bf16, check_f32, check_stats, dev_act, host_act
from tests.test_gpu_frozen_bn import check_dw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
# the reduced ResNeXt model: the fixture's options (stage widths 32 / 64 / 128 / 256 in 4 groups) and small heads
with open(os.path.join(ROOT, "tests", "golden", "resnext_golden.json")) as _f:
    RESNEXT_OPTS = json.load(_f)["opts"]
SMALL_HEADS = ["MODEL.ROI_BOX_HEAD.FC_DIM", 64, "MODEL.ROI_MASK_HEAD.CONV_DIM", 256, "MODEL.ROI_HEADS.NUM_CLASSES", 8]
R50_REDUCED = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 32, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64, "MODEL.RESNETS.WIDTH_PER_GROUP", 32]
LAYER_CASES = [(64, 8, 2, 13, 19, 1), (64, 8, 2, 13, 19, 2), (128, 2, 2, 13, 19, 1), (96, 3, 2, 13, 19, 2)]   # C, groups, B, H, W, stride


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional

    _hip.load()
    return functional


def _operands(case):
    c, groups, b, h, w, stride = case
    x, wt, _bias, gy, _scale, _old = G.grouped_operands((c, groups, b, h, w), stride, "real")
    return x, wt, gy


def _frozen_norm(c, g):
    from u2seg_amd.layers.modules import FrozenBatchNorm2d

    norm = FrozenBatchNorm2d(c)
    norm.weight.copy_(0.5 + torch.rand(c, generator=g))
    norm.weight[c // 3] *= -1.0
    norm.bias.copy_(0.3 * torch.randn(c, generator=g))
    norm.running_mean.copy_(0.2 * torch.randn(c, generator=g))
    norm.running_var.copy_(0.5 + torch.rand(c, generator=g))
    return norm


# ---- layer level ----
@pytest.mark.parametrize("case", LAYER_CASES, ids=str)
def test_grouped_layer_under_frozen_bn_and_folded_eval(F, case):
    """Conv2d(groups) + FrozenBatchNorm2d + ReLU: the training path (layers/frozen.py -> _GroupedConv2dFn with scale = s, bias = t)
    and the folded eval path store the same bits, inside the interval of the float64 layer with W' = bf16(fp32(w) * s); the data
    gradient and dw = s dW' likewise, the latter in the optimizer-less form (returned to autograd)."""
    from u2seg_amd.layers.modules import Conv2d

    c, groups, b, h, w, stride = case
    cg = c // groups
    x, wt, gy = _operands(case)
    conv = Conv2d(c, c, 3, stride=stride, padding=1, bias=False, norm=_frozen_norm(c, torch.Generator().manual_seed(c)),
                  activation="relu", groups=groups).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wt.float())
    conv.train()
    s, t = (v.to(F64).cpu() for v in conv.norm.eval_scale_shift())
    wf = G.fold(wt, s)
    ref, a = G.gconv_fwd_ref(x, wf, groups, stride, bias=t)
    xd = dev_act(x).requires_grad_(True)
    out = conv(xd)
    out.backward(dev_act(gy))
    F.join_all_streams()
    name = "frozen grouped layer %s" % (case,)
    got, _ = host_act(out.detach(), c)
    check_bf16(name + " fwd", got, ref, a, 9 * cg, "real", relu=True)
    dz = gy * (got > 0)
    dref, da = G.gconv_dgrad_ref(dz, wf, groups, (h, w), stride)
    check_bf16(name + " dgrad", host_act(xd.grad, c)[0], dref, da, 9 * cg, "real")
    dwf, dwa = G.gconv_wgrad_ref(x, dz, groups, stride)
    check_dw(name + " dw", conv.weight.grad, dwf, dwa, s, dz.shape[0] * dz.shape[2] * dz.shape[3], "real")
    conv.eval()
    with torch.no_grad():
        out_eval = conv(dev_act(x))
    assert torch.equal(out_eval.view(torch.int16), out.detach().view(torch.int16)), "folded eval path and training path differ"
    assert "_u2_frozen_fold" not in conv.__dict__ and "_u2_layouts" not in conv.weight.__dict__ \
        and "_u2_eval_layouts" not in conv.weight.__dict__, "a grouped layer keeps no kernel layout"


@pytest.mark.parametrize("case", LAYER_CASES, ids=str)
def test_grouped_layer_under_training_bn(F, case, monkeypatch):
    """Conv2d(groups) + BatchNorm2d (training, deterministic statistics) + ReLU through the module: the conv output and its
    statistics against float64, and both conv gradients for the gradient the norm's backward handed to the conv output."""
    from u2seg_amd.layers import modules
    from u2seg_amd.layers.modules import BatchNorm2d, Conv2d

    c, groups, b, h, w, stride = case
    cg = c // groups
    x, wt, gy = _operands(case)
    conv = Conv2d(c, c, 3, stride=stride, padding=1, bias=False, norm=BatchNorm2d(c, sync=False), activation="relu", groups=groups).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(wt.float())
    conv.train()
    seen = {}
    real_conv2d = F.conv2d

    def conv2d(*args, **kwargs):
        y, stats = real_conv2d(*args, **kwargs)
        y.retain_grad()
        seen["y"], seen["stats"], seen["groups"] = y, stats.clone(), kwargs.get("groups")
        return y, stats

    monkeypatch.setattr(modules.F, "conv2d", conv2d)
    F.set_deterministic_stats(True)
    try:
        xd = dev_act(x).requires_grad_(True)
        out = conv(xd)
        out.backward(dev_act(gy * 1024))   # (the generator's gradients are 2^-10 small; the norm divides by the batch deviation)
        F.join_all_streams()
    finally:
        F.set_deterministic_stats(False)
    assert seen["groups"] == groups
    name = "bn grouped layer %s" % (case,)
    wp = G.fold(wt, torch.ones(c, dtype=F64))
    ref, a = G.gconv_fwd_ref(x, wp, groups, stride)
    yy, _ = host_act(seen["y"].detach(), c)
    check_bf16(name + " conv output", yy, ref, a, 9 * cg, "real")
    check_stats(name, seen["stats"], yy, "real")
    assert bool(torch.isfinite(out.detach().float()).all()) and float(out.detach().float().min()) == 0.0
    dz, _ = host_act(seen["y"].grad, c)
    assert float(dz.abs().max()) > 0
    dref, da = G.gconv_dgrad_ref(dz, wp, groups, (h, w), stride)
    check_bf16(name + " dgrad", host_act(xd.grad, c)[0], dref, da, 9 * cg, "real")
    dwf, dwa = G.gconv_wgrad_ref(x, dz, groups, stride)
    check_f32(name + " dw", conv.weight.grad, dwf, dwa, dz.shape[0] * dz.shape[2] * dz.shape[3], "real")


# ---- block level: the fixture blocks, teacher-forced ----
@pytest.mark.parametrize("name", ["proj", "ident"])
def test_fixture_block_against_the_float64_layers(F, name):
    """This project's BottleneckBlock(num_groups=4) with the fixture's weights and buffers.  Every layer is compared with the
    float64 layer evaluated on the STORED bf16 input of that layer (forward) and the stored bf16 gradient of its output
    (backward): the bound is one layer's, no error is carried along the chain (the method of tests/test_gpu_frozen_bn.py)."""
    from u2seg_amd.modeling.backbone import BottleneckBlock

    fx = np.load(os.path.join(ROOT, "tests", "golden", "resnext_block_golden.npz"))
    cin, cout, cb, stride = G.BLOCKS[name]
    blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, num_groups=G.BLOCK_GROUPS, norm="FrozenBN")
    convs = {k: getattr(blk, k) for k in ("conv1", "conv2", "conv3", "shortcut") if getattr(blk, k) is not None}
    pre = "frozen.%s" % name
    for k, conv in convs.items():
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(fx["%s.%s.weight" % (pre, k)]))
        for buf in ("weight", "bias", "running_mean", "running_var"):
            getattr(conv.norm, buf).copy_(torch.from_numpy(fx["%s.%s.norm.%s" % (pre, k, buf)]))
        conv.norm.eps = float(fx["%s.%s.norm.eps" % (pre, k)])
    assert blk.conv2.groups == G.BLOCK_GROUPS and tuple(blk.conv2.weight.shape) == (cb, cb // G.BLOCK_GROUPS, 3, 3)
    blk.to(DEV).train()
    seen = {}
    for k, conv in convs.items():
        def hook(mod, args, kwargs, output, k=k):
            output.retain_grad()
            seen[k] = (args[0], kwargs.get("residual"), output)
        conv.register_forward_hook(hook, with_kwargs=True)
    x = R.bf16_round(torch.from_numpy(fx[pre + ".x"]).to(F64))
    gy = R.bf16_round(torch.from_numpy(fx[pre + ".gy"]).to(F64))
    xd = dev_act(x).requires_grad_(True)
    y = blk(xd)
    y.backward(dev_act(gy))
    F.join_all_streams()
    cins = {"conv1": cin, "conv2": cb, "conv3": cb, "shortcut": cin}
    couts = {"conv1": cb, "conv2": cb, "conv3": cout, "shortcut": cout}
    dx_parts = {}
    for k, conv in convs.items():
        xin, res, out = seen[k]
        st, groups, kk = conv.stride, conv.groups, conv.kernel_size[0]
        length = kk * kk * cins[k] // groups
        s, t = (v.to(F64).cpu() for v in conv.norm.eval_scale_shift())
        wf = G.fold(conv.weight.detach().cpu(), s)
        xi, p0 = host_act(xin.detach(), cins[k])
        assert p0 == 0.0
        old = host_act(res.detach(), couts[k])[0] if res is not None else None
        relu = k in ("conv1", "conv2", "conv3")
        ref, a = G.gconv_fwd_ref(xi, wf, groups, st, bias=t)
        got, p1 = host_act(out.detach(), couts[k])
        assert p1 == 0.0
        check_bf16("%s %s fwd" % (name, k), got, ref, a, length, "real", relu=relu, old=old)
        gout, _ = host_act(out.grad, couts[k])
        dz = gout * (got > 0) if relu else gout
        dwf, dwa = G.gconv_wgrad_ref(xi, dz, groups, st, kk)
        m = dz.shape[0] * dz.shape[2] * dz.shape[3]
        check_dw("%s %s dw" % (name, k), conv.weight.grad, dwf, dwa, s, m, "real")
        dlen = kk * kk * couts[k] // groups
        dref, da = G.gconv_dgrad_ref(dz, wf, groups, xi.shape[2:], st)
        e = R.fp32_sum_bound(dlen, da)
        if k in ("conv2", "conv3"):   # their input has one reader: its stored gradient is this layer's data gradient
            dgot, _ = host_act(xin.grad if xin.grad is not None else seen["conv1" if k == "conv2" else "conv2"][2].grad, cins[k])
            check_bf16("%s %s dgrad" % (name, k), dgot, dref, da, dlen, "real")
        else:
            dx_parts[k] = (R.rne_bf16(dref - e), R.rne_bf16(dref + e))
    lo1, hi1 = dx_parts["conv1"]
    if "shortcut" in dx_parts:
        lo2, hi2 = dx_parts["shortcut"]
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
    yy, _ = host_act(y.detach(), cout)
    print("RESNEXT %s | max |y - reference fp32 y| (information: bf16 storage between the layers) | %.4g" % (
        name, float((yy - torch.from_numpy(fx[pre + ".y"]).to(F64)).abs().max())))


@pytest.mark.parametrize("name", ["proj", "ident"])
def test_bn_fixture_block_against_the_float64_layers(F, name, monkeypatch):
    """This project's BottleneckBlock(num_groups=4, norm="BN") in training mode with the weights and affine pairs of the
    reference's block (tests/golden/resnext_block_bn_<name>_golden.npz, which tests/test_grouped_conv_host.py ties to the float64
    layers).  Every convolution is compared with the float64 convolution of its STORED bf16 input, its statistics with the sums
    over its stored output, both conv gradients with the float64 ones for the stored gradient the norm handed back; the block's
    output against the reference's fp32 output is information (bf16 storage between the layers: no derived bound applies)."""
    from u2seg_amd.layers import modules
    from u2seg_amd.modeling.backbone import BottleneckBlock

    fx = np.load(os.path.join(ROOT, "tests", "golden", "resnext_block_bn_%s_golden.npz" % name))
    cin, cout, cb, stride = G.BLOCKS[name]
    pre = "bn.%s" % name
    blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, num_groups=G.BLOCK_GROUPS, norm="BN")
    convs = {k: getattr(blk, k) for k in ("conv1", "conv2", "conv3", "shortcut") if getattr(blk, k) is not None}
    with torch.no_grad():
        for k, conv in convs.items():
            conv.weight.copy_(torch.from_numpy(fx["%s.%s.weight" % (pre, k)]))
            conv.norm.weight.copy_(torch.from_numpy(fx["%s.%s.norm.weight" % (pre, k)]))
            conv.norm.bias.copy_(torch.from_numpy(fx["%s.%s.norm.bias" % (pre, k)]))
            conv.norm.eps = float(fx["%s.%s.norm.eps" % (pre, k)])
    blk.to(DEV).train()
    by_weight = {conv.weight.data_ptr(): k for k, conv in convs.items()}
    seen = {}
    real_conv2d = F.conv2d

    def conv2d(x_, w_, *args, **kwargs):
        y, stats = real_conv2d(x_, w_, *args, **kwargs)
        y.retain_grad()
        if x_.requires_grad and not x_.is_leaf:
            x_.retain_grad()
        seen[by_weight[w_.data_ptr()]] = (x_, y, stats.clone(), kwargs.get("groups", 1))
        return y, stats

    monkeypatch.setattr(modules.F, "conv2d", conv2d)
    x = R.bf16_round(torch.from_numpy(fx[pre + ".x"]).to(F64))
    gy = R.bf16_round(torch.from_numpy(fx[pre + ".gy"]).to(F64))
    F.set_deterministic_stats(True)
    try:
        xd = dev_act(x).requires_grad_(True)
        y = blk(xd)
        y.backward(dev_act(gy))
        F.join_all_streams()
    finally:
        F.set_deterministic_stats(False)
    assert sorted(seen) == sorted(convs) and seen["conv2"][3] == G.BLOCK_GROUPS
    cins = {"conv1": cin, "conv2": cb, "conv3": cb, "shortcut": cin}
    couts = {"conv1": cb, "conv2": cb, "conv3": cout, "shortcut": cout}
    for k, conv in convs.items():
        xin, yk, stats, groups = seen[k]
        st, kk = conv.stride, conv.kernel_size[0]
        wp = G.fold(conv.weight.detach().cpu(), torch.ones(couts[k], dtype=F64))
        xi, p0 = host_act(xin.detach(), cins[k])
        assert p0 == 0.0
        ref, a = G.gconv_fwd_ref(xi, wp, groups, st)
        got, p1 = host_act(yk.detach(), couts[k])
        assert p1 == 0.0
        label = "bn %s %s" % (name, k)
        check_bf16(label + " conv output", got, ref, a, kk * kk * cins[k] // groups, "real")
        check_stats(label, stats, got, "real")
        dz, _ = host_act(yk.grad, couts[k])
        assert float(dz.abs().max()) > 0
        dwf, dwa = G.gconv_wgrad_ref(xi, dz, groups, st, kk)
        check_f32(label + " dw", conv.weight.grad, dwf, dwa, dz.shape[0] * dz.shape[2] * dz.shape[3], "real")
        if k in ("conv2", "conv3"):   # their input has one reader: its stored gradient is this layer's data gradient
            dref, da = G.gconv_dgrad_ref(dz, wp, groups, xi.shape[2:], st)
            check_bf16(label + " dgrad", host_act(xin.grad, cins[k])[0], dref, da, kk * kk * couts[k] // groups, "real")
    yy, _ = host_act(y.detach(), cout)
    yref = torch.from_numpy(fx[pre + ".y"]).to(F64)
    print("RESNEXT bn %s | max |y - reference fp32 y|, mean |reference y| (information) | %.4g, %.4g" % (
        name, float((yy - yref).abs().max()), float(yref.abs().mean())))


# ---- model level ----
def _build(config, opts):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_optimizer

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", config))
    cfg.merge_from_list(["MODEL.DEVICE", DEV] + list(opts))
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    return cfg, model, build_optimizer(cfg, model)


def _grouped_convs(model):
    return {n: m for n, m in model.named_modules() if getattr(m, "groups", 1) > 1}


def _two_steps(F, config, opts):
    """Step 1 by hand (to look at the arena), step 2 through the trainer -> model"""
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.engine import SimpleTrainer

    cfg, model, opt = _build(config, opts)
    batch = make_synthetic_batch(2, height=128, width=160, device=DEV, num_thing_classes=8)
    grouped = _grouped_convs(model)
    assert len(grouped) == 16 and all(n.endswith(".conv2") for n in grouped)
    before = {n: m.weight.detach().clone() for n, m in grouped.items()}
    opt.zero_grad()
    losses = model(batch)
    assert len(losses) == 10 and all(bool(torch.isfinite(v)) for v in losses.values()), losses
    sum(losses.values()).backward()
    F.join_all_streams()
    F.assert_no_deferred_gradients()
    trained = 0
    for n, m in grouped.items():
        if not m.weight.requires_grad:
            assert not hasattr(m.weight, "_u2_grad"), n
            continue
        trained += 1
        slot = m.weight._u2_grad
        assert tuple(slot.shape) == tuple(m.weight.shape) and (m.weight.grad is None or m.weight.grad is slot), n
        assert bool(torch.isfinite(slot).all()) and bool((slot != 0).any()), "%s: no gradient in its arena slice" % n
        assert "_u2_layouts" not in m.weight.__dict__ and "_u2_frozen_fold" not in m.__dict__, n
    assert trained >= 13
    opt.step()
    trainer = SimpleTrainer(model, opt)
    losses = trainer.run_step(batch)
    torch.cuda.synchronize()
    trainer.check_finite()
    assert len(losses) == 10
    F.assert_no_deferred_gradients()
    for n, m in grouped.items():
        assert torch.equal(m.weight.detach(), before[n]) != m.weight.requires_grad, n
    return model, batch


def test_reduced_resnext_model_trains_and_repeats_its_bits_at_inference(F):
    model, batch = _two_steps(F, "u2seg_R50_800.yaml", RESNEXT_OPTS + SMALL_HEADS)
    model.eval()
    feats = []
    handle = model.backbone.register_forward_hook(lambda mod, args, out: feats.append({k: v.clone() for k, v in out.items()}))
    with torch.no_grad():
        a, b = model(batch), model(batch)
    handle.remove()
    assert len(feats) == 2 and sorted(feats[0]) == ["p2", "p3", "p4", "p5", "p6"]
    for k in feats[0]:
        assert bool(torch.isfinite(feats[0][k].float()).all()) and float(feats[0][k].float().abs().max()) > 0, k
        assert torch.equal(feats[0][k].view(torch.int16), feats[1][k].view(torch.int16)), "%s differs between two eval passes" % k
    assert _same(a, b), "two eval passes gave different results"


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if hasattr(a, "get_fields"):
        return _same(a.get_fields(), b.get_fields())
    if hasattr(a, "tensor"):
        return torch.equal(a.tensor, b.tensor)
    return a == b


def test_finetune_recipe_trains_on_resnext(F):
    model, _ = _two_steps(F, "u2seg_R50_800_finetune.yaml", RESNEXT_OPTS + SMALL_HEADS)
    assert model.backbone.bottom_up.frozen_prefix == 2
    assert not any(p.requires_grad for p in model.backbone.bottom_up.res2.parameters())


def test_the_default_model_never_calls_the_grouped_entries(F, monkeypatch):
    from u2seg_amd import _hip
    from u2seg_amd.data import make_synthetic_batch

    calls = []
    real_call, real_status = _hip.call, _hip.call_status
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(_hip, "call_status", lambda name, *a: (calls.append(name), real_status(name, *a))[1])
    cfg, model, opt = _build("u2seg_R50_800.yaml", R50_REDUCED + SMALL_HEADS)
    assert _grouped_convs(model) == {}
    batch = make_synthetic_batch(2, height=128, width=160, device=DEV, num_thing_classes=8)
    opt.zero_grad()
    sum(model(batch).values()).backward()
    F.join_all_streams()
    torch.cuda.synchronize()
    assert "u2_conv_igemm" in calls and len(calls) > 100
    assert [n for n in calls if n.startswith("u2_gconv3x3")] == []
