"""CPU tests of precise BatchNorm (u2seg_amd/engine/precise_bn.py): the hook's schedule, which layers it updates and at which
stride, the float64 oracle of the estimator that the GPU tests use, and the two C-ABI entries."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation")


def r50_fpn_widths():
    """Output channels of the 61 BatchNorm layers of R50-FPN in model.modules() order: the FPN's lateral / output pairs, then the
    bottom-up network (stem, res2..res5 with the shortcut before conv1..conv3 of a block)."""
    widths = [256] * 8 + [64]
    for bottleneck, out, blocks in ((64, 256, 3), (128, 512, 4), (256, 1024, 6), (512, 2048, 3)):
        for i in range(blocks):
            widths += ([out] if i == 0 else []) + [bottleneck, bottleneck, out]
    return widths


# ---- float64 oracles of the estimator -----------------------------------------------------------------------------------------
def fvcore_incremental(batches):
    """Literal float64 transcription of fvcore 0.1.5's update_bn_stats for one layer: batches = [(b, mean[C], var[C]), ...], where
    mean / var are the running buffers after a momentum-1.0 forward (batch mean, unbiased batch variance)."""
    tot = 0
    pop_mean = pop_sq = None
    for b, mean, var in batches:
        mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
        if pop_mean is None:
            pop_mean, pop_sq = np.zeros_like(mean), np.zeros_like(mean)
        tot += b
        sq = mean * mean + var * (b - 1) / b
        pop_mean = pop_mean + (mean - pop_mean) * b / tot
        pop_sq = pop_sq + (sq - pop_sq) * b / tot
    return pop_mean, pop_sq - pop_mean * pop_mean


def closed_form(batches):
    """The sums the device kernels accumulate: A = sum b mean, Q = sum b mean^2 + (b - 1) var, T = sum b."""
    A = Q = None
    T = 0.0
    for b, mean, var in batches:
        mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
        if A is None:
            A, Q = np.zeros_like(mean), np.zeros_like(mean)
        b = float(b)
        A = A + b * mean
        Q = Q + (b * mean * mean + (b - 1.0) * var)
        T += b
    m = A / T
    return m, Q / T - m * m


def random_sequence(rng, iters, channels, canvases=((800, 1344), (640, 1088), (1024, 1344), (480, 736)), n=16, stride=4):
    """Per-iteration (b, batch mean, unbiased batch variance) with b from a multi-scale canvas and |mean| >> std on some channels."""
    base = rng.normal(size=channels) * np.where(rng.random(channels) < 0.3, 200.0, 1.0)
    scale = rng.uniform(0.1, 3.0, size=channels)
    out = []
    for _ in range(iters):
        h, w = canvases[rng.integers(len(canvases))]
        b = n * -(-h // stride) * -(-w // stride)
        mean = (base + 0.05 * rng.normal(size=channels) * scale).astype(np.float32)
        var = (scale ** 2 * rng.uniform(0.5, 1.5, size=channels)).astype(np.float32)
        out.append((b, mean, var))
    return out


def test_closed_form_matches_fvcore_incremental():
    rng = np.random.default_rng(0)
    for iters, channels in ((1, 7), (5, 64), (200, 256)):
        seq = random_sequence(rng, iters, channels)
        m0, v0 = fvcore_incremental(seq)
        m1, v1 = closed_form(seq)
        np.testing.assert_allclose(m1, m0, rtol=1e-12, atol=1e-12)
        # var = E[x^2] - mean^2 cancels by up to mean^2 / var (~1e5 here): both forms carry that many float64 roundings
        np.testing.assert_allclose(v1, v0, rtol=1e-9, atol=1e-9 * float(np.max(m0 * m0)))
    # one batch: the population variance of that batch, i.e. the unbiased variance times (b - 1) / b
    b, mean, var = seq[0]
    m, v = closed_form([(b, mean, var)])
    np.testing.assert_allclose(m, mean.astype(np.float64), rtol=1e-15)
    np.testing.assert_allclose(v, var.astype(np.float64) * (b - 1) / b, rtol=1e-7, atol=1e-9 * float(np.max(mean.astype(np.float64) ** 2)))


def test_closed_form_is_not_the_averaged_variant():
    """The older fvcore form averages the per-batch variances; with moving means the population variance is larger."""
    seq = [(10, np.array([0.0]), np.array([1.0])), (10, np.array([4.0]), np.array([1.0]))]
    m, v = closed_form(seq)
    assert m[0] == 2.0 and abs(v[0] - (0.9 + 4.0)) < 1e-12


def test_precise_bn_due_schedule():
    from u2seg_amd.engine import precise_bn_due

    assert [i for i in range(20) if precise_bn_due(i, 10, 0)] == [9]
    assert [i for i in range(20) if precise_bn_due(i, 10, 4)] == [3, 7, 9]
    assert [i for i in range(12, 30) if precise_bn_due(i, 10, 4)] == []
    assert [i for i in range(3) if precise_bn_due(i, 3, 2)] == [1, 2]


def _model(name="u2seg_base.yaml", opts=()):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CFG_DIR, name))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    model = build_model(cfg)
    model.train()
    return model


def test_get_bn_modules_counts_and_strides():
    from u2seg_amd.engine import get_bn_modules
    from u2seg_amd.engine.precise_bn import _backbone_strides

    model = _model()
    bn = get_bn_modules(model)
    assert len(bn) == 61 and sum(m.num_features for m in bn) == 28608
    assert [m.num_features for m in bn] == r50_fpn_widths()
    bottom_up = model.backbone.bottom_up
    assert sum(1 for m in bn if any(m is x for x in bottom_up.modules())) == 53
    # every layer has an output stride, and it is the one of the map it normalises
    strides = _backbone_strides(model.backbone)
    assert all(id(m) in strides for m in bn)
    assert strides[id(bottom_up.stem.conv1.norm)] == 2
    res3 = bottom_up.res3[0]
    assert strides[id(res3.shortcut.norm)] == 8 and strides[id(res3.conv3.norm)] == 8
    assert strides[id(bottom_up.res2[0].conv1.norm)] == 4 and strides[id(bottom_up.res5[2].conv3.norm)] == 32
    assert strides[id(model.backbone.fpn_lateral2.norm)] == 4 and strides[id(model.backbone.fpn_output5.norm)] == 32
    # strided 1x1 (STRIDE_IN_1X1 True, the MSRA layout) or strided 3x3: conv1 of a downsampling block sits at either stride
    s1 = strides[id(res3.conv1.norm)]
    assert s1 == (8 if res3.conv1.stride == 2 else 4) and strides[id(res3.conv2.norm)] == 8

    assert get_bn_modules(_model(opts=["MODEL.RESNETS.NORM", "FrozenBN", "MODEL.FPN.NORM", ""])) == []
    model.eval()
    assert get_bn_modules(model) == []


def test_update_bn_stats_rejects_bn_outside_backbone():
    """A training-mode BatchNorm the backbone pass does not reach is named, not silently left at its moving average."""
    from u2seg_amd.engine import update_bn_stats

    model = _model(opts=["MODEL.SEM_SEG_HEAD.NORM", "SyncBN"])
    with pytest.raises(NotImplementedError, match="sem_seg_head"):
        update_bn_stats(model, iter([]), 1)


def test_update_bn_stats_without_bn_is_a_no_op():
    from u2seg_amd.engine import update_bn_stats

    model = _model(opts=["MODEL.RESNETS.NORM", "FrozenBN", "MODEL.FPN.NORM", ""])
    update_bn_stats(model, iter([]), 5)  # nothing to update: no batch is drawn, nothing asserts


def test_abi_declares_precise_bn_entries():
    from u2seg_amd import _hip

    syms = _hip.declared_symbols()
    P, I = ctypes.c_void_p, ctypes.c_int
    assert syms["u2_bn_precise_update"] == (I, [P, I, P, P, I, I, I, I, P])
    assert syms["u2_bn_precise_finalize"] == (I, [P, I, P, P, I, P])
    # that the library exports every declared symbol is test_host_logic.py::test_cabi_library_exports_every_declared_symbol
