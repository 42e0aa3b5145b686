"""What the convolution tests share to force a kernel and to check which one ran: the names of the variant words' fields and of
the u2_conv_last_kernel codes (K: include/u2seg_hip.h as parsed by u2seg_amd._hip), the environment override, and the variant
tables that more than one test module walks."""
import contextlib
import os

from u2seg_amd._hip import K


@contextlib.contextmanager
def forced(conv=None, wgrad=None):
    old = {k: os.environ.get(k) for k in ("U2_CONV_VARIANT", "U2_WGRAD_VARIANT")}
    try:
        for k, v in (("U2_CONV_VARIANT", conv), ("U2_WGRAD_VARIANT", wgrad)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        # the kernel tests see the library's own dispatch: the product path's rule of where the stream-K form may run
        # (layers/streams.py:streamk_region - only the bottom-up backbone asks for it) is tested in test_streamk_region_rule
        from u2seg_amd.layers import functional as _fn
        with _fn.streamk_region():
            yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def last_kernel():
    from u2seg_amd import _hip

    return _hip.call_nostream("u2_conv_last_kernel")


def igemm_code(bk, tm, tn, nst, glds=1):
    return K.K_IGEMM + bk * 10000 + (tm // 64) * 1000 + (tn // 64) * 100 + nst * 10 + glds


def stream_code(cin, cout):
    return K.K_STREAM + (cin // 32) * 10 + (0 if cout > 128 else 1 if cout > 64 else 2)


def tile_cfg(cfg):
    return cfg * 2 ** K.CV_TILE_CFG_SHIFT


def ring(stages):
    """conv_igemm's LDS ring of 2, 3 or 4 stages."""
    return (stages - 1) * 2 ** K.CV_RING_SHIFT


NEVER_TILE = tile_cfg(K.CV_TILE_CFG_NEVER)
TINY = K.CV_TINY_GRID   # 8 work-groups only: many tiles per group
STREAM = K.CV_STREAM_FORCE   # conv_stream.hip wherever it applies
HALO = K.CV_HALO_FORCE
_BIG, _BK32, _REG = K.CV_TILE_256X128, K.CV_BK32, K.CV_REG_STAGING
_WIDE, _STAGGER, _PARITY = K.CV_WIDE_FORCE, K.CV_WIDE_STAGGER, K.CV_WIDE_STAGGER_PARITY
# (U2_CONV_VARIANT, expected u2_conv_last_kernel of the FORWARD launch) on a 3x3 64 -> 256 case (K = 576)
CONV_VARIANTS = [
    (NEVER_TILE, igemm_code(64, 128, 128, 2)),            # 128 x 128, BK 64, 2-stage LDS-DMA ring (the default of that family)
    (NEVER_TILE | _REG, igemm_code(64, 128, 128, 2, 0)),  # register-staged operands
    (NEVER_TILE | ring(3), igemm_code(64, 128, 128, 3)),
    (NEVER_TILE | ring(4), igemm_code(64, 128, 128, 4)),
    (NEVER_TILE | _BK32, igemm_code(32, 128, 128, 4)),    # BK 32 (default ring depth 4)
    (NEVER_TILE | _BK32 | ring(2), igemm_code(32, 128, 128, 2)),
    (NEVER_TILE | _BK32 | ring(3), igemm_code(32, 128, 128, 3)),
    (NEVER_TILE | _BK32 | _REG, igemm_code(32, 128, 128, 2, 0)),
    (NEVER_TILE | _BIG, igemm_code(64, 256, 128, 2)),     # 256 x 128 tile, 8 waves
    (NEVER_TILE | _BIG | _REG, igemm_code(64, 256, 128, 2, 0)),
    (NEVER_TILE | _BIG | ring(3), igemm_code(64, 256, 128, 3)),
    (NEVER_TILE | _BIG | _BK32, igemm_code(32, 256, 128, 4)),
    (NEVER_TILE | _BIG | _BK32 | ring(2), igemm_code(32, 256, 128, 2)),
    (NEVER_TILE | _BIG | _BK32 | ring(3), igemm_code(32, 256, 128, 3)),
    (NEVER_TILE | _BIG | _BK32 | _REG, igemm_code(32, 256, 128, 2, 0)),
    (NEVER_TILE | _WIDE, K.K_IGEMM256),                   # conv_igemm256_kernel<false>
    (NEVER_TILE | _WIDE | _STAGGER, K.K_IGEMM256 + K.K_IGEMM256_STAGGER),   # conv_igemm256_kernel<true> (staggered wave groups)
    (NEVER_TILE | _WIDE | _STAGGER | _PARITY, K.K_IGEMM256 + K.K_IGEMM256_STAGGER),
] + [(tile_cfg(cfg) | (TINY if tiny else 0), K.K_TILE + cfg) for cfg in range(1, 7) for tiny in (0, 1)] + [
    # stream-K form, 24 work-groups: shares begin and end inside tiles, partial tiles are handed over
    (tile_cfg(cfg) | TINY | K.CV_STREAMK_FORCE, K.K_STREAMK + cfg) for cfg in (1, 2, 3, 4)] + [
    (HALO, K.K_HALO), (HALO | TINY, K.K_HALO),            # conv_halo.hip (halo-staged 3x3), 12 tiles / 8 work-groups
]
# the same on a 1x1 512 -> 40 layer: the 256 x 64 tile family
NARROW_VARIANTS = [
    (NEVER_TILE, igemm_code(64, 256, 64, 2)), (NEVER_TILE | _REG, igemm_code(64, 256, 64, 2, 0)),
    (NEVER_TILE | ring(3), igemm_code(64, 256, 64, 3)), (NEVER_TILE | ring(4), igemm_code(64, 256, 64, 4)),
    (NEVER_TILE | _BK32, igemm_code(32, 256, 64, 4)), (NEVER_TILE | _BK32 | ring(2), igemm_code(32, 256, 64, 2)),
    (NEVER_TILE | _BK32 | ring(3), igemm_code(32, 256, 64, 3)), (NEVER_TILE | _BK32 | _REG, igemm_code(32, 256, 64, 2, 0))]

_W, _X = K.K_WGRAD, K.K_WGRAD_XCD
# (U2_WGRAD_VARIANT, expected code) of the per-tap kernels: conv_wgrad_kernel<GLDS, TR> is K_WGRAD + 2 GLDS + TR
WGRAD_TAP_VARIANTS = [
    (0, _W + 3), (K.WG_REG_STAGING, _W + 1), (K.WG_SCALAR_GATHER, _W + 2), (K.WG_REG_STAGING | K.WG_SCALAR_GATHER, _W),
    (K.WG_XCD_FORCE, _W + 3 + _X), (K.WG_XCD_FORBID, _W + 3), (K.WG_WIDE_FORCE, K.K_WGRAD256),
    (K.WG_WIDE_FORCE | K.WG_XCD_FORCE, K.K_WGRAD256 + _X),
    (1 * 2 ** K.WG_FEWER_SPLITS_SHIFT, _W + 3), (2 * 2 ** K.WG_FEWER_SPLITS_SHIFT, _W + 3),
    # partial tiles + wgrad_reduce_kernel wherever there are >= 2 pixel splits / atomics
    (K.WG_PARTIALS_FORCE, _W + 3), (K.WG_PARTIALS_FORCE | K.WG_WIDE_FORCE, K.K_WGRAD256),
    (K.WG_PARTIALS_FORCE | K.WG_XCD_FORCE, _W + 3 + _X), (K.WG_ATOMICS, _W + 3)]
_ROUNDS2 = 1 * 2 ** K.WG_HALO_ROUNDS_SHIFT   # two rounds of work-groups
# wgrad_halo.hip forced: the default epilogue, two rounds, partial blocks + reduction pass, both, atomics
WGRAD_HALO_VARIANTS = [K.WG_HALO_FORCE, K.WG_HALO_FORCE | _ROUNDS2, K.WG_HALO_FORCE | K.WG_PARTIALS_FORCE,
                       K.WG_HALO_FORCE | K.WG_PARTIALS_FORCE | _ROUNDS2, K.WG_HALO_FORCE | K.WG_ATOMICS]
WS_FORCE, WS_TINY = K.WG_STREAM_FORCE, K.WG_STREAM_TINY


def ws_variant(cfg, tiny):
    """wgrad_stream.hip forced on any size with block configuration cfg (0 = automatic)."""
    return WS_FORCE | (WS_TINY if tiny else 0) | cfg * 2 ** K.WG_STREAM_CFG_SHIFT
