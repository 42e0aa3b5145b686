"""layers/conv_launch.py: ConvGeom's arithmetic and the positional argument lists of the five conv launches, against literals
transcribed by hand from the call sites these helpers replaced (include/u2seg_hip.h: u2_conv_igemm, u2_conv_wgrad,
u2_conv_wgrad_into).  No GPU and no library: _hip.call is replaced by a recorder and only data_ptr() is taken from the tensors."""
import inspect

import pytest
import torch

from u2seg_amd import _hip
from u2seg_amd.layers import conv_launch, frozen
from u2seg_amd.layers import functional as F
from u2seg_amd.layers.conv_launch import ConvGeom

VARIANT = 77   # no other argument of any case has this value
T = [torch.empty(4) for _ in range(5)]   # five operands with five addresses
P = [t.data_ptr() for t in T]
assert len(set(P)) == 5 and 0 not in P

# name: (x shape, weight shape, stride, pad, the 13 fields b h w cp n cin kh kw ho wo npad stride pad)
CASES = {
    "3x3": ((2, 5, 7, 32), (32, 32, 3, 3), 1, 1, (2, 5, 7, 32, 32, 32, 3, 3, 5, 7, 32, 1, 1)),
    "3x3s2": ((2, 5, 7, 32), (32, 32, 3, 3), 2, 1, (2, 5, 7, 32, 32, 32, 3, 3, 3, 4, 32, 2, 1)),
    "1x1s2": ((2, 5, 7, 32), (32, 32, 1, 1), 2, 0, (2, 5, 7, 32, 32, 32, 1, 1, 3, 4, 32, 2, 0)),
    "7x7s2": ((2, 5, 7, 32), (64, 3, 7, 7), 2, 3, (2, 5, 7, 32, 64, 3, 7, 7, 3, 4, 64, 2, 3)),
    "n15": ((2, 5, 7, 32), (15, 32, 1, 1), 1, 0, (2, 5, 7, 32, 15, 32, 1, 1, 5, 7, 32, 1, 0)),
    "fc": ((3, 7, 7, 32), (1024, 32, 7, 7), 1, 0, (3, 7, 7, 32, 1024, 32, 7, 7, 1, 1, 1024, 1, 0)),
    "fc_pad1": ((3, 7, 7, 32), (1024, 32, 7, 7), 1, 1, (3, 7, 7, 32, 1024, 32, 7, 7, 3, 3, 1024, 1, 1)),
    "fc_8x7": ((3, 8, 7, 32), (1024, 32, 7, 7), 1, 0, (3, 8, 7, 32, 1024, 32, 7, 7, 2, 1, 1024, 1, 0)),
    "1x1_on_1x1": ((3, 1, 1, 32), (1024, 32, 1, 1), 1, 0, (3, 1, 1, 32, 1024, 32, 1, 1, 1, 1, 1024, 1, 0)),
    "1x1c24": ((2, 5, 7, 32), (40, 24, 1, 1), 1, 0, (2, 5, 7, 32, 40, 24, 1, 1, 5, 7, 64, 1, 0)),
}


def geom(name):
    x_shape, w_shape, stride, pad, _ = CASES[name]
    return ConvGeom.of(torch.Size(x_shape), torch.Size(w_shape), stride, pad)


@pytest.fixture
def calls(monkeypatch):
    log = []
    monkeypatch.setattr(_hip, "call", lambda name, *args: log.append((name, tuple(_hip._conv(a) for a in args))))
    return log


def check(calls, name, args):
    assert calls == [(name, args)]
    assert len(args) + 1 == len(_hip.declared_symbols()[name][1])   # + the stream
    del calls[:]


@pytest.mark.parametrize("name", sorted(CASES))
def test_geom_is_the_13_tuple_in_the_call_sites_order(name):
    g = geom(name)
    assert tuple(g) == CASES[name][4]
    assert ConvGeom._fields == ("b", "h", "w", "cp", "n", "cin", "kh", "kw", "ho", "wo", "npad", "stride", "pad")
    assert len(g) == 13 and g == ConvGeom(*CASES[name][4])


def test_derived_properties():
    g = geom("3x3s2")
    assert (g.m_in, g.m_out, g.taps) == (2 * 5 * 7, 2 * 3 * 4, 9)
    g = geom("7x7s2")
    assert (g.m_in, g.m_out, g.taps) == (70, 24, 49)
    unit = {name: geom(name).is_1x1_unit for name in CASES}
    assert unit == {name: name in ("n15", "1x1_on_1x1", "1x1c24") for name in CASES}   # 1x1s2: strided
    assert not ConvGeom.of((2, 5, 7, 32), (32, 32, 1, 1), 1, 1).is_1x1_unit            # padded
    fc = {name: geom(name).is_fc for name in CASES}
    assert fc == {name: name == "fc" for name in CASES}


def test_forward_args(calls):
    x, wk, out, bias, stats = T
    conv_launch.forward(geom("3x3"), x, wk, out, bias, stats, False, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], P[3], P[4], 2, 5, 7, 32, 32, 5, 7, 32, 32, 3, 3, 1, 1, 1, 1, 0, 0, VARIANT))
    conv_launch.forward(geom("3x3s2"), x, wk, out, None, stats, True, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], None, P[4], 2, 5, 7, 32, 32, 3, 4, 32, 32, 3, 3, 1, 1, 2, 1, 1, 0, VARIANT))
    conv_launch.forward(geom("1x1s2"), x, wk, out, bias, None, False, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], P[3], None, 2, 5, 7, 32, 32, 3, 4, 32, 32, 1, 1, 0, 0, 2, 1, 0, 0, VARIANT))
    conv_launch.forward(geom("7x7s2"), x, wk, out, None, None, False, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], None, None, 2, 5, 7, 32, 32, 3, 4, 64, 64, 7, 7, 3, 3, 2, 1, 0, 0, VARIANT))
    conv_launch.forward(geom("n15"), x, wk, out, bias, stats, False, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], P[3], P[4], 2, 5, 7, 32, 32, 5, 7, 15, 32, 1, 1, 0, 0, 1, 1, 0, 0, VARIANT))
    conv_launch.forward(geom("fc"), x, wk, out, bias, None, True, 0, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], P[3], None, 3, 7, 7, 32, 32, 1, 1, 1024, 1024, 7, 7, 0, 0, 1, 1, 1, 0, VARIANT))


def test_forward_args_accumulating_with_relu(calls):
    """conv2d_add_'s form: out = relu(conv + bias + out)."""
    x, wk, out, bias, _ = T
    conv_launch.forward(geom("3x3s2"), x, wk, out, bias, None, True, 1, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], P[3], None, 2, 5, 7, 32, 32, 3, 4, 32, 32, 3, 3, 1, 1, 2, 1, 1, 1, VARIANT))
    conv_launch.forward(geom("3x3s2"), x, wk, out, bias, None, True, 1, VARIANT)
    assert type(calls[0][1][-3]) is int   # the flag reaches the library as an int, as int(relu) did at the call sites


def test_dgrad_args(calls):
    dz, wd, dx = T[:3]
    head = (P[0], P[1], P[2], None, None)
    conv_launch.dgrad(geom("3x3"), dz, wd, dx, VARIANT)
    check(calls, "u2_conv_igemm", head + (2, 5, 7, 32, 32, 5, 7, 32, 32, 3, 3, 1, 1, 1, 1, 0, 0, VARIANT))
    conv_launch.dgrad(geom("3x3s2"), dz, wd, dx, VARIANT)   # mul 1, div 2, pads k - 1 - pad = 1
    check(calls, "u2_conv_igemm", head + (2, 3, 4, 32, 32, 5, 7, 32, 32, 3, 3, 1, 1, 1, 2, 0, 0, VARIANT))
    conv_launch.dgrad(geom("1x1s2"), dz, wd, dx, VARIANT)   # pads 0, 0
    check(calls, "u2_conv_igemm", head + (2, 3, 4, 32, 32, 5, 7, 32, 32, 1, 1, 0, 0, 1, 2, 0, 0, VARIANT))
    conv_launch.dgrad(geom("7x7s2"), dz, wd, dx, VARIANT)   # pads 7 - 1 - 3 = 3; the output has cp = 32 channels, not cin = 3
    check(calls, "u2_conv_igemm", head + (2, 3, 4, 64, 64, 5, 7, 32, 32, 7, 7, 3, 3, 1, 2, 0, 0, VARIANT))
    conv_launch.dgrad(geom("n15"), dz, wd, dx, VARIANT)     # dz has npad = 32 channels
    check(calls, "u2_conv_igemm", head + (2, 5, 7, 32, 32, 5, 7, 32, 32, 1, 1, 0, 0, 1, 1, 0, 0, VARIANT))
    conv_launch.dgrad(geom("fc_pad1"), dz, wd, dx, VARIANT)   # pads 7 - 1 - 1 = 5
    check(calls, "u2_conv_igemm", head + (3, 3, 3, 1024, 1024, 7, 7, 32, 32, 7, 7, 5, 5, 1, 1, 0, 0, VARIANT))


def test_fc_dgrad_args(calls):
    dz, wt, dx = T[:3]
    conv_launch.fc_dgrad(geom("fc"), dz, wt, dx, VARIANT)
    check(calls, "u2_conv_igemm", (P[0], P[1], P[2], None, None, 1, 3, 1, 1024, 1024, 3, 1, 49 * 32, 49 * 32, 1, 1, 0, 0, 1, 1, 0, 0,
                                   VARIANT))


def test_wgrad_args(calls):
    x, dz, dw = T[:3]
    head = (P[0], P[1], P[2])
    conv_launch.wgrad_scratch(geom("3x3"), x, dz, dw)
    check(calls, "u2_conv_wgrad", head + (2, 5, 7, 32, 32, 5, 7, 32, 32, 3, 3, 1, 1, 1, 0))
    conv_launch.wgrad_scratch(geom("3x3s2"), x, dz, dw)
    check(calls, "u2_conv_wgrad", head + (2, 5, 7, 32, 32, 3, 4, 32, 32, 3, 3, 1, 1, 2, 0))
    conv_launch.wgrad_scratch(geom("7x7s2"), x, dz, dw)
    check(calls, "u2_conv_wgrad", head + (2, 5, 7, 32, 32, 3, 4, 64, 64, 7, 7, 3, 3, 2, 0))
    conv_launch.wgrad_scratch(geom("fc"), x, dz, dw)
    check(calls, "u2_conv_wgrad", head + (3, 7, 7, 32, 32, 1, 1, 1024, 1024, 7, 7, 0, 0, 1, 0))
    conv_launch.wgrad_into(geom("1x1c24"), x, dz, dw)   # cin 24 in cp 32, n 40 in npad 64: the tail is n, cin, cin, 1, 1, 0
    check(calls, "u2_conv_wgrad_into", head + (2, 5, 7, 32, 32, 5, 7, 64, 64, 1, 1, 0, 0, 1, 40, 24, 24, 1, 1, 0))
    conv_launch.wgrad_into(geom("n15"), x, dz, dw)
    check(calls, "u2_conv_wgrad_into", head + (2, 5, 7, 32, 32, 5, 7, 32, 32, 1, 1, 0, 0, 1, 15, 32, 32, 1, 1, 0))


def test_alloc_out_zeroes_padded_channels_only(monkeypatch):
    made = []
    for fn in ("zeros", "empty"):
        monkeypatch.setattr(torch, fn, lambda *a, _fn=fn, _real=getattr(torch, fn), **k: made.append(_fn) or _real(*a, **k))
    out = conv_launch.alloc_out(geom("n15"), "cpu")
    assert made == ["zeros"] and tuple(out.shape) == (2, 5, 7, 32) and out.dtype == torch.bfloat16 and not out.any()
    del made[:]
    out = conv_launch.alloc_out(geom("3x3s2"), "cpu")
    assert made == ["empty"] and tuple(out.shape) == (2, 3, 4, 32) and out.dtype == torch.bfloat16


# the stem's im2col fallback is a GEMM over a prepared matrix whose output has n columns as they are: it stays a direct call
STEM_FALLBACK = (
    '_hip.call("u2_conv_igemm", col, wk, out, None, None if _DET_STATS else stats, 1, m, 1, kp, kp, m, 1, n, n, 1, 1, 0, 0, 1,',
    '_hip.call("u2_conv_wgrad", col, dout, dwk, 1, m, 1, kp, kp, m, 1, n, n, 1, 1, 0, 0, 1, 0)',
)


def test_the_layers_write_no_conv_argument_list_themselves():
    names = ('"u2_conv_igemm"', '"u2_conv_wgrad"', '"u2_conv_wgrad_into"')
    for module, allowed in ((F, STEM_FALLBACK), (frozen, ())):
        hits = [line.strip() for line in inspect.getsource(module).splitlines() if any(name in line for name in names)]
        assert [line for line in hits if line not in allowed] == [], module.__name__
    helpers = inspect.getsource(conv_launch)
    assert [helpers.count(name) for name in names] == [3, 1, 1]
