"""Boundary and plain confusion matrices on the GPU (u2seg_amd/csrc/semeval.hip through the C ABI binding) against the host
definition (evaluation/semseg_ops.boundary_confusion_host) run on the CPU, and the semantic evaluator fed device tensors
against the same evaluator on the host.  Integers throughout: every comparison is ==.  Every case keeps the contract (labels
below n, sizes as declared): nothing here reads or writes out of bounds on purpose."""
import numpy as np
import pytest
import torch

from tests import semseg_boundary_cases as cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = cases.N


@pytest.fixture(scope="module")
def O():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.evaluation import semseg_ops

    _hip.load()
    return semseg_ops


def status(name, *args):
    from u2seg_amd import _hip

    return _hip.call_nostream(name, *args, _hip.stream_ptr())


def offset_copy(a, offset):
    """The map on the device, its first byte `offset` bytes behind a 16-byte boundary."""
    flat = torch.zeros(a.size + 32, dtype=torch.uint8, device=DEV)
    start = (-flat.data_ptr()) % 16 + offset
    view = flat[start : start + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == offset % 16 and view.is_contiguous()
    return view


def device(O, pred, gt, lut, d, n=N, with_conf=True, offset=0, start=0):
    """Both matrices from one call through the binding, started at `start`."""
    from u2seg_amd import _hip

    h, w = pred.shape
    p, g = offset_copy(pred, offset), offset_copy(gt, offset)
    lut_d = None if lut is None else torch.from_numpy(lut).to(DEV)
    conf = torch.full((n, n), start, dtype=torch.int64, device=DEV)
    bconf = torch.full((n, n), start, dtype=torch.int64, device=DEV)
    need = int(_hip.call_nostream("u2_semseg_boundary_scratch_bytes", h, w, d))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV) if need else None
    _hip.call("u2_semseg_boundary_confusion", p, g, lut_d, h, w, d, n, conf if with_conf else None, bconf, scratch, need)
    torch.cuda.synchronize()
    return conf.cpu().numpy(), bconf.cpu().numpy()


def host(O, pred, gt, lut, d, n=N):
    c, b = O.boundary_confusion_host(torch.from_numpy(pred), torch.from_numpy(gt), None if lut is None else torch.from_numpy(lut),
                                     d, n)
    return c.numpy(), b.numpy()


def check(O, pred, gt, lut, d, **kw):
    want_c, want_b = host(O, pred, gt, lut, d)
    got_c, got_b = device(O, pred, gt, lut, d, **kw)
    assert np.array_equal(got_b, want_b), (pred.shape, d, int(np.abs(got_b - want_b).sum()))
    assert np.array_equal(got_c, want_c), (pred.shape, d, int(np.abs(got_c - want_c).sum()))


def test_library_exports_the_entry_points(O):
    from u2seg_amd import _hip

    declared, lib = _hip.declared_symbols(), _hip.load()
    for name in ("u2_semseg_boundary_confusion", "u2_semseg_boundary_fused_cap", "u2_semseg_boundary_scratch_bytes"):
        assert name in declared and getattr(lib, name) is not None
    assert O.fused_cap() >= 31


@pytest.mark.parametrize("h,w,d", cases.SHAPES)
def test_shapes_equal_the_host_definition(O, h, w, d):
    """1 x 1 up to several tiles; windows larger than the image; d = 40 on the general path."""
    for name, (pred, gt) in cases.label_maps(h, w, seed=h * 1000 + w + d).items():
        check(O, pred, gt, None, d)


@pytest.mark.parametrize("h,w", [(63, 63), (64, 64), (65, 65), (63, 65), (65, 63), (127, 129), (129, 127)])
def test_tile_side_plus_and_minus_one(O, h, w):
    rs = np.random.RandomState(h * 7 + w)
    for d in (1, 5):
        check(O, cases.blobs(rs, h, w, side=5), cases.blobs(rs, h, w, side=6), None, d)


@pytest.mark.parametrize("offset", [3, 13])
def test_rows_and_buffers_off_the_16_byte_grid(O, offset):
    """w = 131 and w = 37 (no multiple of 16, of 4 or of 2: every row starts at another misalignment), the buffers themselves
    3 and 13 bytes behind a 16-byte boundary, so that the first and the last bytes of the maps share their aligned words with
    bytes outside them."""
    rs = np.random.RandomState(offset)
    for h, w, d in ((70, 131, 7), (33, 37, 2), (5, 3, 1)):
        check(O, cases.blobs(rs, h, w, side=4), cases.blobs(rs, h, w, side=7), None, d, offset=offset)


def test_fused_cap_and_the_general_path_behind_it(O):
    cap = O.fused_cap()
    rs = np.random.RandomState(2)
    pred, gt = cases.blobs(rs, 150, 200, side=40), cases.blobs(rs, 150, 200, side=50)
    for m in (pred, gt):  # no label 0 in the middle: the erosion by cap + 1 leaves something there
        m[30:120, 40:160] = np.maximum(m[30:120, 40:160], 1)
        assert O.erode_host(torch.from_numpy(m), cap + 1).any()
    for d in (cap, cap + 1):
        check(O, pred, gt, None, d)
    check(O, pred, gt, cases.chained_lut(), cap + 1, offset=3)  # the general path with a table and unaligned buffers
    check(O, pred, gt, None, 500)                                # a window far larger than the image


def test_full_size_image(O):
    """800 x 1333, d = 31 (what boundary_dilation gives): 13 x 21 tiles."""
    assert O.boundary_dilation(800, 1333) == 31
    rs = np.random.RandomState(4)
    check(O, cases.blobs(rs, 800, 1333, side=90), cases.blobs(rs, 800, 1333, side=110), None, 31)


def test_lut_null_against_a_chained_table(O):
    """Clusters 0 .. 27 through the table (several onto 16) == the mapped map with no table; the table acts before the erosion."""
    rs = np.random.RandomState(8)
    lut = cases.chained_lut()
    assert (lut[:28] == 16).sum() >= 2
    pred = np.repeat(np.repeat(rs.randint(0, 28, size=(9, 17)), 8, axis=0), 8, axis=1)[:70, :131].astype(np.uint8)
    gt = cases.blobs(rs, 70, 131)
    with_table = device(O, pred, gt, lut, 7)
    without = device(O, lut[pred], gt, None, 7)
    want = host(O, pred, gt, lut, 7)
    for a, b, c in zip(with_table, without, want):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert with_table[1][16].sum() + with_table[1][:, 16].sum() > 0  # the ignore label reaches the boundary matrix


def test_conf_null_changes_nothing_else(O):
    pred, gt = cases.label_maps(70, 131, seed=6)["blobs"]
    for d in (7, O.fused_cap() + 1):
        conf, bconf = device(O, pred, gt, None, d, start=3)
        conf_off, bconf_off = device(O, pred, gt, None, d, with_conf=False, start=3)
        assert np.array_equal(bconf_off, bconf)
        assert np.array_equal(conf_off, np.full((N, N), 3))  # the tensor that was not passed is as it was
        assert conf.sum() == 3 * N * N + 70 * 131


def test_three_images_accumulate_into_nonzero_matrices(O):
    rs = np.random.RandomState(9)
    conf = torch.arange(N * N, dtype=torch.int64, device=DEV).view(N, N).clone()
    bconf = (2 * torch.arange(N * N, dtype=torch.int64, device=DEV)).view(N, N).clone()
    want_c, want_b = conf.cpu().numpy().copy(), bconf.cpu().numpy().copy()
    for h, w in ((40, 33), (129, 257), (64, 200)):
        pred, gt = cases.blobs(rs, h, w), cases.blobs(rs, h, w, side=11)
        d = O.boundary_dilation(h, w)
        O.boundary_confusion(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), None, d, N, conf, bconf)
        c, b = host(O, pred, gt, None, d)
        want_c += c
        want_b += b
    assert np.array_equal(conf.cpu().numpy(), want_c) and np.array_equal(bconf.cpu().numpy(), want_b)


def test_largest_matrix_side(O):
    rs = np.random.RandomState(10)
    pred = np.repeat(rs.randint(0, 32, size=(50, 14)), 5, axis=1).astype(np.uint8)
    gt = np.repeat(rs.randint(0, 32, size=(10, 70)), 5, axis=0).astype(np.uint8)
    want_c, want_b = host(O, pred, gt, None, 2, 32)
    got_c, got_b = device(O, pred, gt, None, 2, 32)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_b, want_b)


def test_error_codes(O):
    m = torch.zeros((8, 8), dtype=torch.uint8, device=DEV)
    conf = torch.zeros((33, 33), dtype=torch.int64, device=DEV)
    bconf = torch.zeros((33, 33), dtype=torch.int64, device=DEV)
    name, pm, pc, pb = "u2_semseg_boundary_confusion", m.data_ptr(), conf.data_ptr(), bconf.data_ptr()
    assert status(name, pm, pm, None, 8, 8, 1, 33, pc, pb, None, 0) != 0
    assert status(name, pm, pm, None, 8, 8, 0, N, pc, pb, None, 0) != 0
    assert status(name, pm, pm, None, 0, 8, 1, N, pc, pb, None, 0) != 0
    assert status(name, pm, pm, None, 8, 8, 1, N, pc, None, None, 0) != 0
    assert status(name, pm, pm, None, 8, 8, O.fused_cap() + 1, N, pc, pb, None, 0) != 0  # above the cap without scratch
    torch.cuda.synchronize()
    assert not conf.any() and not bconf.any()  # nothing was launched
    assert status(name, pm, pm, None, 8, 8, 1, N, pc, pb, None, 0) == 0
    torch.cuda.synchronize()
    assert int(conf.view(-1)[0]) == 64 == int(conf.sum()) and int(bconf.view(-1)[0]) == 64 == int(bconf.sum())


def test_evaluator_on_the_device_equals_the_host(O, tmp_path, monkeypatch):
    """SemSegEvaluator(boundary_iou=True) with the predictions on the GPU (one launch per image, both matrices there) against
    the same evaluator fed the CPU copies: key for key."""
    from u2seg_amd.evaluation import SemSegEvaluator

    monkeypatch.chdir(tmp_path)
    fx, inputs, outputs, _ = cases.tiny_val_sem(tmp_path)
    on_host = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    on_host.process(inputs, outputs)
    on_dev = SemSegEvaluator("tiny_val_sem", mode="eval", boundary_iou=True)
    on_dev.process(inputs, [dict(o, sem_seg=o["sem_seg"].to(DEV)) for o in outputs])
    assert on_dev._conf_matrix.is_cuda and on_dev._b_conf_matrix.is_cuda  # the accumulation stayed on the device
    assert on_dev._conf_matrix.tolist() == on_host._conf_matrix.tolist() == fx["conf_matrix"]
    assert on_dev._b_conf_matrix.tolist() == on_host._b_conf_matrix.tolist()
    assert on_dev._b_conf_matrix.sum() == on_dev._conf_matrix.sum() > 0
    a, b = on_dev.evaluate()["sem_seg"], on_host.evaluate()["sem_seg"]
    assert list(a) == list(b) and any(k.startswith("BoundaryIoU-") for k in a)
    for k in a:
        assert (a[k] != a[k] and b[k] != b[k]) or a[k] == b[k], k
