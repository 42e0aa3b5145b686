"""RESNETS.NUM_GROUPS on the host: the float64 references of the grouped convolution (tests/grouped_conv_refs.py) against torch's
conv2d(groups = G) and its autograd in float64, the float64 restatement of the ResNeXt fixture blocks against the reference's fp32
known answers (tests/golden/resnext_block_golden.npz and, under training-mode BatchNorm, resnext_block_bn_<block>_golden.npz, written
by tests/golden/make_resnext_fixture.py),
the module tree of the reduced ResNeXt model against the reference's (tests/golden/resnext_golden.json), what the builder refuses,
and the declarations of the three C entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import grouped_conv_refs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


# ---- the references ----
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c,groups", G.CHANNELS, ids=str)
def test_references_equal_torch_in_float64(c, groups, stride):
    g = torch.Generator().manual_seed(c + groups + stride)
    b, h, w = 2, 7, 10
    x = torch.randn((b, c, h, w), generator=g, dtype=F64, requires_grad=True)
    wt = torch.randn((c, c // groups, 3, 3), generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn((c,), generator=g, dtype=F64)
    y = TF.conv2d(x, wt, bias, stride, 1, 1, groups)
    assert tuple(y.shape[2:]) == G.out_hw(h, w, stride)
    gy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(gy)
    xd, wd = x.detach(), wt.detach()
    tol = 1e-12
    ref, a = G.gconv_fwd_ref(xd, wd, groups, stride, bias)
    assert float((ref - y.detach()).abs().max()) < tol * float(a.max())
    # the companion is the same sum over magnitudes
    assert torch.allclose(a, TF.conv2d(xd.abs(), wd.abs(), bias.abs(), stride, 1, 1, groups), rtol=1e-12, atol=0)
    dx, a = G.gconv_dgrad_ref(gy, wd, groups, (h, w), stride)
    assert float((dx - x.grad).abs().max()) < tol * float(a.max())
    dw, a = G.gconv_wgrad_ref(xd, gy, groups, stride)
    assert dw.shape == wt.shape and float((dw - wt.grad).abs().max()) < tol * float(a.max())


def test_fold_is_one_fp32_multiply_and_one_rounding():
    g = torch.Generator().manual_seed(3)
    w, s = torch.randn((8, 2, 3, 3), generator=g), torch.rand(8, generator=g) + 0.5
    got = G.fold(w.to(F64), s.to(F64))
    want = torch.stack([(w[n] * s[n]).bfloat16() for n in range(8)]).to(F64)
    assert torch.equal(got, want)


def test_operand_generator_preconditions():
    """Every case of tests/test_gpu_grouped_conv.py in exact mode: sum |term| stays below 2^24 for all three passes, scaled too."""
    from tests import float64_refs as R

    for case in G.CASES:
        for stride in (1, 2):
            c, groups, b, h, w = case
            x, wt, bias, gy, scale, old = G.grouped_operands(case, stride, "exact")
            ws = wt * scale.view(-1, 1, 1, 1)
            assert torch.equal(G.fold(wt, scale), ws)
            assert float(G.gconv_fwd_ref(x, ws, groups, stride, bias)[1].max()) < R.TWO24
            assert float(G.gconv_dgrad_ref(gy, ws, groups, (h, w), stride)[1].max()) < R.TWO24
            assert float((scale.abs().view(-1, 1, 1, 1) * G.gconv_wgrad_ref(x, gy, groups, stride)[1] + old.abs()).max()) < R.TWO24


# ---- the fixture blocks ----
@pytest.mark.parametrize("name", ["proj", "ident"])
def test_float64_restatement_reproduces_the_reference_block(name, kind="frozen"):
    """fp32 (the reference's BottleneckBlock(num_groups=4) on the CPU) against float64, every element, bound from the term counts
    carried through the chain (grouped_conv_refs.block_chain: the method of tests/frozen_bn_refs.py)."""
    fx = np.load(os.path.join(GOLDEN, "resnext_block_golden.npz"))
    layers = G.block_layers(fx, name)
    assert ("shortcut" in layers) == (name == "proj")
    cin, cout, cb, stride = G.BLOCKS[name]
    assert tuple(layers["conv2"]["w"].shape) == (cb, cb // G.BLOCK_GROUPS, 3, 3) and layers["conv2"]["stride"] == stride
    assert any(bool((v["s"] < 0).any()) for v in layers.values()), "a negative scale is part of the fixture"
    pre = "%s.%s" % (kind, name)
    x, gy = torch.from_numpy(fx[pre + ".x"]).to(F64), torch.from_numpy(fx[pre + ".gy"]).to(F64)
    assert tuple(x.shape) == (2, cin, 12, 20)
    ref = G.block_chain(layers, x, gy)
    assert sorted(ref) == sorted(["y", "dx"] + [k + ".dweight" for k in layers])
    for key, (val, bound) in ref.items():
        got = torch.from_numpy(fx["%s.%s" % (pre, key)]).to(F64)
        assert got.shape == val.shape, key
        err = (got - val).abs()
        print("RESNEXT64 %s %s | max |err| / E | %.4g" % (pre, key, float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all()), (key, float(err.max()), float(bound.max()))
        assert float(val.abs().max()) > 0
    y = ref["y"][0]
    assert 0.1 < float((y > 0).double().mean()) < 0.9, "both sides of the tail's ReLU are part of the fixture"


def _within(label, got, val, bound, shares):
    got = got.to(F64)
    assert got.shape == val.shape, label
    err = (got - val).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    share = float(bound.mean() / val.abs().mean().clamp(min=1e-300))
    print("RESNEXT64 %s | max |err| / E %.4g | mean E / mean |value| %.3g" % (label, ratio, share))
    assert bool((err <= bound).all()), (label, float(err.max()), float(bound.max()))
    assert float(val.abs().max()) > 0
    shares.append((label, share))


@pytest.mark.parametrize("name", ["proj", "ident"])
def test_float64_restatement_reproduces_the_reference_block_under_training_bn(name):
    """The reference's BottleneckBlock(num_groups=4, norm="BN") in training mode (fp32, CPU) against float64, every element.
    The block's output is held to the bound carried along the whole chain; every layer's norm output, dweight and input
    gradient to ONE layer's bound, on the layer's recorded fp32 input and the recorded gradient of its norm output
    (grouped_conv_refs.bn_layer / bn_layer_bwd).  The per-layer bounds must also say something: their mean stays below 5 % of
    the mean magnitude of what they bound (they come out at 0.005 - 0.2 %).  The chain's bound on y is a worst case through three
    normalisations and is about a tenth of the mean |y|: it catches a wrong block, not a wrong rounding; its ratio is printed."""
    fx = np.load(os.path.join(GOLDEN, "resnext_block_bn_%s_golden.npz" % name))
    pre = "bn.%s." % name
    rec = lambda key: torch.from_numpy(fx[pre + key]).to(F64)
    layers = G.bn_block_layers(fx, name)
    assert ("shortcut" in layers) == (name == "proj")
    cin, cout, cb, stride = G.BLOCKS[name]
    assert tuple(layers["conv2"]["w"].shape) == (cb, cb // G.BLOCK_GROUPS, 3, 3) and layers["conv2"]["stride"] == stride
    assert any(bool((v["gamma"] < 0).any()) for v in layers.values()), "a negative scale is part of the fixture"
    x, gy, y = rec("x"), rec("gy"), rec("y")
    assert tuple(x.shape) == (2, cin, 12, 20) and 0.2 < float((y > 0).double().mean()) < 0.8
    shares = []
    # the output along the chain
    _within(name + " y (chain)", y, *G.block_forward_bn(layers, x), [])
    # layer by layer
    dz = gy * (y > 0)
    inputs = {"conv1": x, "conv2": rec("conv1.o").clamp(min=0), "conv3": rec("conv2.o").clamp(min=0), "shortcut": x}
    grads = {"conv1": rec("conv1.g"), "conv2": rec("conv2.g"), "conv3": dz, "shortcut": dz}
    sc = rec("shortcut.o") if "shortcut" in layers else x
    dx_parts = []
    for k, lay in layers.items():
        xin = inputs[k]
        o, eo, cache = G.bn_layer(lay, xin, torch.zeros_like(xin))
        if k == "conv3":   # its norm's output goes into the tail: y = relu(o + shortcut), one more fp32 addition
            _within(name + " y (conv3 on its recorded input)", y, (o + sc).clamp(min=0), eo + G.U24 * (o.abs() + sc.abs() + eo), shares)
        else:
            _within("%s %s.o" % (name, k), rec(k + ".o"), o, eo, shares)
        (dw, edw), (dxin, edx) = G.bn_layer_bwd(lay, cache, xin, grads[k])
        _within("%s %s.dweight" % (name, k), rec(k + ".dweight"), dw, edw, shares)
        if k in ("conv2", "conv3"):
            _within("%s %s.dxin" % (name, k), rec(k + ".dxin"), dxin, edx, shares)
        else:
            dx_parts.append((dxin, edx))
    if len(dx_parts) == 1:
        dx_parts.append((dz, torch.zeros_like(dz)))   # the identity shortcut hands the tail's gradient on
    (d1, e1), (d2, e2) = dx_parts
    _within(name + " dx", rec("dx"), d1 + d2, e1 + e2 + G.U24 * (d1.abs() + d2.abs() + e1 + e2), shares)
    loose = [(label, share) for label, share in shares if not share < 0.05]
    assert not loose, loose


# ---- the model ----
def _cfg(opts=(), name="u2seg_R50_800.yaml"):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CFG_DIR, name))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _fixture():
    with open(os.path.join(GOLDEN, "resnext_golden.json")) as f:
        return json.load(f)


def test_reduced_resnext_model_has_the_references_keys_shapes_and_count():
    from u2seg_amd.modeling import build_model

    fx = _fixture()
    model = build_model(_cfg(fx["opts"]))
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == fx["state_dict"]
    assert sum(p.numel() for p in model.parameters()) == fx["num_params"]
    bu = model.backbone.bottom_up
    widths = [(st[0].conv2.groups, tuple(st[0].conv2.weight.shape)) for st in bu.stages]
    assert widths == [(4, (32, 8, 3, 3)), (4, (64, 16, 3, 3)), (4, (128, 32, 3, 3)), (4, (256, 64, 3, 3))]
    assert all(blk.conv1.groups == 1 and blk.conv3.groups == 1 for st in bu.stages for blk in st)


def test_one_group_is_the_model_it_was():
    import zlib

    from u2seg_amd.modeling import build_model

    with open(os.path.join(GOLDEN, "model_small.json")) as f:
        fx = json.load(f)
    model = build_model(_cfg(["MODEL.RESNETS.NUM_GROUPS", 1]))
    sd = model.state_dict()
    assert len(sd) == fx["num_state_entries"] and zlib.crc32("\n".join(sd.keys()).encode()) == fx["state_dict_keys_crc32"]
    assert sum(p.numel() for p in model.parameters()) == fx["num_params"]
    assert all(m.groups == 1 for m in model.modules() if hasattr(m, "groups"))


def test_dilation_is_refused_by_name():
    from u2seg_amd.modeling import build_model

    with pytest.raises(ValueError, match="MODEL.RESNETS.RES5_DILATION"):
        build_model(_cfg(["MODEL.RESNETS.RES5_DILATION", 2]))


@pytest.mark.parametrize("opts", [["MODEL.RESNETS.NUM_GROUPS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 2],      # cg = 2 in res2
                                  ["MODEL.RESNETS.NUM_GROUPS", 3, "MODEL.RESNETS.WIDTH_PER_GROUP", 8],       # 24 channels
                                  ["MODEL.RESNETS.NUM_GROUPS", 2, "MODEL.RESNETS.WIDTH_PER_GROUP", 64]],     # cg = 128 in res3
                         ids=["cg2", "width24", "cg128"])
def test_a_width_the_kernels_do_not_serve_is_refused_at_construction(opts):
    from u2seg_amd.modeling import build_model

    with pytest.raises(ValueError, match="MODEL.RESNETS.NUM_GROUPS") as e:
        build_model(_cfg(opts))
    assert "WIDTH_PER_GROUP" in str(e.value)


def test_served_widths():
    from u2seg_amd.layers.conv_launch import GroupedGeom, grouped_served

    assert all(grouped_served(c, g) for c, g in G.CHANNELS)
    assert all(grouped_served(c, 32) for c in (128, 256, 512, 1024, 2048))        # 32x4d, 32x8d through res5
    assert all(grouped_served(c, 64) for c in (256, 512, 1024, 2048))             # 64x4d
    assert not any(grouped_served(c, g) for c, g in [(64, 1), (64, 32), (48, 4), (40, 5), (256, 2), (96, 32)])
    geom = GroupedGeom.of((2, 13, 19, 64), (64, 8, 3, 3), 8, 2, 1)
    assert geom == (2, 13, 19, 64, 8, 2, 7, 10) and geom.cg == 8 and geom.m_out == 140
    with pytest.raises(AssertionError):
        GroupedGeom.of((2, 13, 19, 64), (64, 8, 1, 1), 8, 1, 0)


def test_x101_yaml_loads():
    cfg = _cfg(name="u2seg_X101_32x8d_800.yaml")
    r = cfg.MODEL.RESNETS
    assert (r.DEPTH, r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1) == (101, 32, 8, False)
    assert cfg.MODEL.WEIGHTS == ""
    base = _cfg()
    assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == base.MODEL.ROI_HEADS.NUM_CLASSES and cfg.SOLVER.BASE_LR == base.SOLVER.BASE_LR


def test_grouped_layer_module():
    from u2seg_amd.layers import Conv2d

    conv = Conv2d(64, 64, 3, padding=1, bias=False, groups=8)
    assert tuple(conv.weight.shape) == (64, 8, 3, 3) and conv.groups == 8
    assert Conv2d(64, 64, 3, padding=1).groups == 1 and tuple(Conv2d(64, 32, 3).weight.shape) == (32, 64, 3, 3)
    with pytest.raises(AssertionError):
        Conv2d(64, 64, 3, groups=7)


# ---- the C ABI ----
def test_the_three_entries_are_declared():
    from u2seg_amd import _hip

    d = _hip.declared_symbols()
    p, i = ctypes.c_void_p, ctypes.c_int
    assert d["u2_gconv3x3_fwd"] == (i, [p] * 6 + [i] * 7 + [p])       # in, w, scale, bias, out, stats | B H W C groups stride relu
    assert d["u2_gconv3x3_dgrad"] == (i, [p] * 4 + [i] * 6 + [p])     # dz, w, scale, dx | B H W C groups stride
    assert d["u2_gconv3x3_wgrad"] == (i, [p] * 4 + [i] * 6 + [p])     # x, dz, scale, dw | B H W C groups stride
