"""A convolution's shapes as one record (ConvGeom) and the launches of u2_conv_igemm, u2_conv_wgrad and u2_conv_wgrad_into built
from it: a layer's positional argument lists (include/u2seg_hip.h) are written here and nowhere else.  No switches, no caches."""
import collections

import torch

from .. import _hip
from .weights import BF16, ceil32


class ConvGeom(collections.namedtuple("ConvGeom", "b h w cp n cin kh kw ho wo npad stride pad")):
    """x [b, h, w, cp] with cin <= cp logical channels, weight [n, cin, kh, kw], output [b, ho, wo, npad]."""
    __slots__ = ()

    @classmethod
    def of(cls, x_shape, weight_shape, stride, pad):
        b, h, w, cp = x_shape
        n, cin, kh, kw = weight_shape
        return cls(b, h, w, cp, n, cin, kh, kw, (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1, ceil32(n),
                   stride, pad)

    m_in = property(lambda g: g.b * g.h * g.w)      # rows of x as a matrix
    m_out = property(lambda g: g.b * g.ho * g.wo)   # rows of the output
    taps = property(lambda g: g.kh * g.kw)
    is_1x1_unit = property(lambda g: g.kh == 1 and g.kw == 1 and g.stride == 1 and g.pad == 0)
    # "fully connected": the filter covers the whole input, so every input pixel meets exactly one tap (box head fc1)
    is_fc = property(lambda g: g.ho == 1 and g.wo == 1 and g.pad == 0 and g.h == g.kh and g.w == g.kw and g.kh * g.kw > 1)


def alloc_out(g, device):
    """The output tensor; zeroed when it has padded channels, which no kernel writes."""
    return (torch.zeros if g.npad != g.n else torch.empty)((g.b, g.ho, g.wo, g.npad), dtype=BF16, device=device)


def forward(g, x, wk, out, bias, stats, relu, accumulate, variant):
    _hip.call("u2_conv_igemm", x, wk, out, bias, stats, g.b, g.h, g.w, g.cp, g.cp, g.ho, g.wo, g.n, g.npad, g.kh, g.kw, g.pad, g.pad,
              g.stride, 1, int(relu), accumulate, variant)


def dgrad(g, dz, wd, dx, variant):
    """The data gradient as a convolution of dz: extents and channel counts swapped, pad -> k - 1 - pad, the stride as `div`."""
    _hip.call("u2_conv_igemm", dz, wd, dx, None, None, g.b, g.ho, g.wo, g.npad, g.npad, g.h, g.w, g.cp, g.cp, g.kh, g.kw,
              g.kh - 1 - g.pad, g.kw - 1 - g.pad, 1, g.stride, 0, 0, variant)


def fc_dgrad(g, dz, wt, dx, variant):
    """g.is_fc: the data gradient is the plain GEMM dx[b, (kh,kw,c)] = dz[b, :] . W[:, (kh,kw,c)]."""
    k = g.kh * g.kw * g.cp
    _hip.call("u2_conv_igemm", dz, wt, dx, None, None, 1, g.b, 1, g.npad, g.npad, g.b, 1, k, k, 1, 1, 0, 0, 1, 1, 0, 0, variant)


def wgrad_scratch(g, x, dz, dwk):
    """Into zeroed scratch in the kernel's layout [npad, taps, cp]."""
    _hip.call("u2_conv_wgrad", x, dz, dwk, g.b, g.h, g.w, g.cp, g.cp, g.ho, g.wo, g.npad, g.npad, g.kh, g.kw, g.pad, g.pad, g.stride, 0)


def wgrad_into(g, x, dz, dst):
    """A 1x1 layer's gradient added straight into its [n, cin] parameter gradient."""
    _hip.call("u2_conv_wgrad_into", x, dz, dst, g.b, g.h, g.w, g.cp, g.cp, g.ho, g.wo, g.npad, g.npad, g.kh, g.kw, g.pad, g.pad,
              g.stride, g.n, g.cin, g.cin, 1, 1, 0)


class GroupedGeom(collections.namedtuple("GroupedGeom", "b h w c groups stride ho wo")):
    """A grouped 3x3 / pad-1 convolution (u2_gconv3x3_*): x [b, h, w, c], weight [c, c // groups, 3, 3], output [b, ho, wo, c]."""
    __slots__ = ()

    @classmethod
    def of(cls, x_shape, weight_shape, groups, stride, pad):
        b, h, w, c = x_shape
        n, cg, kh, kw = weight_shape
        assert (kh, kw, pad) == (3, 3, 1) and stride in (1, 2), "a grouped convolution is 3x3, pad 1, stride 1 or 2"
        assert n == c and groups >= 2 and cg * groups == c, ("grouped conv: channels", c, n, cg, groups)
        return cls(b, h, w, c, groups, stride, (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1)

    m_out = property(lambda g: g.b * g.ho * g.wo)
    cg = property(lambda g: g.c // g.groups)


def grouped_served(channels, groups):
    """Whether the u2_gconv3x3_* kernels serve a layer of `channels` in `groups` (include/u2seg_hip.h)."""
    return groups >= 2 and channels % groups == 0 and channels % 32 == 0 and channels // groups in (4, 8, 16, 32, 64)


def grouped_forward(g, x, w, scale, bias, out, stats, relu):
    """`w`: the fp32 parameter [c, cg, 3, 3] itself; scale / bias / stats: fp32 [c] / [c] / [2, c] or None."""
    _hip.call("u2_gconv3x3_fwd", x, w, scale, bias, out, stats, g.b, g.h, g.w, g.c, g.groups, g.stride, int(relu))


def grouped_dgrad(g, dz, w, scale, dx):
    _hip.call("u2_gconv3x3_dgrad", dz, w, scale, dx, g.b, g.h, g.w, g.c, g.groups, g.stride)


def grouped_wgrad(g, x, dz, scale, dw):
    """Accumulates into dw, fp32 [c, cg, 3, 3]."""
    _hip.call("u2_gconv3x3_wgrad", x, dz, scale, dw, g.b, g.h, g.w, g.c, g.groups, g.stride)
