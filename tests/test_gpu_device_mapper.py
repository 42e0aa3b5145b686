"""The device mapper on the GPU (u2seg_amd/csrc/augment.hip through the C ABI binding): the three kernels against the host
definitions of u2seg_amd/data/device_mapper.py (themselves pinned against PIL and DatasetMapper in
tests/test_device_mapper_host.py), the contract checks of the launchers, and the loader -> DevicePrefetcher path against the
host mapper's batches.  Integers throughout: every comparison is ==.  Every launched case keeps the contract; the violations
are refused on the host before anything is launched: nothing here reads or writes out of bounds."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests import device_mapper_cases as cases
from u2seg_amd.data import device_mapper as dm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def place(records, shifts=None):
    """The records' tensors in one host block (and its device copy) the way the slots lay them out, with the first byte of
    record i's image and label map shifts[i] bytes behind a 256-byte boundary: (records with device views, device block, host
    block)."""
    shifts = shifts or [0] * len(records)
    cursor, where = 0, []
    for rec, shift in zip(records, shifts):
        at = {}
        for k in dm.TENSOR_KEYS:
            if k in rec:
                at[k] = cursor + (shift if k in ("dm_image", "dm_sem_seg") else 0)
                cursor = (at[k] + rec[k].numel() * rec[k].element_size() + 255) // 256 * 256
        where.append(at)
    host = torch.zeros(max(cursor, 256), dtype=torch.uint8)
    assert host.data_ptr() % 16 == 0
    for rec, at in zip(records, where):
        for k, off in at.items():
            n = rec[k].numel() * rec[k].element_size()
            host[off:off + n] = rec[k].contiguous().reshape(-1).view(torch.uint8)
    block = host.to(DEV)
    assert block.data_ptr() % 16 == 0
    out = []
    for rec, at in zip(records, where):
        d = {k: v for k, v in rec.items() if k not in dm.TENSOR_KEYS}
        for k, off in at.items():
            n = rec[k].numel() * rec[k].element_size()
            d[k] = block[off:off + n].view(rec[k].dtype).view(rec[k].shape)
        out.append(d)
    return out, block, host


def run(records, shifts=None):
    """The kernels' outputs for every record, unfiltered, on the host: [(image, labels, masks, counts)]."""
    dev, block, host = place(records, shifts)
    pending = dm.launch_batch(dev, block, host)
    torch.cuda.synchronize()
    out = []
    for i in range(len(records)):
        image, labels, masks, counts = pending.outputs(i)
        assert image.dtype == torch.uint8 and masks.dtype == torch.bool and (labels is None or labels.dtype == torch.int64)
        out.append((image.cpu().numpy(), None if labels is None else labels.cpu().numpy(), masks.cpu().numpy(),
                    counts.numpy().copy()))
    return out


def check(records, got):
    for rec, (image, labels, masks, counts) in zip(records, got):
        want_image, want_labels, want_masks, want_counts = cases.host_outputs(rec)
        assert np.array_equal(image, want_image)
        if want_labels is not None:
            assert np.array_equal(labels, want_labels)
        assert masks.shape == want_masks.shape and np.array_equal(masks, want_masks)
        assert np.array_equal(counts, want_counts) and np.array_equal(counts, masks.sum(axis=(1, 2)))


@pytest.mark.parametrize("pair", cases.SIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_resize_kernels(hip, pair):
    """Bilinear image and nearest label map (with the value 255) of every size pair: the four flips, each with the source's
    first byte 0, 1 and 3 bytes past a 16-byte boundary - twelve images of one launch."""
    (h, w), (H, W) = pair
    records, shifts = [], []
    for (hflip, vflip), shift in itertools.product(cases.FLIPS, (0, 1, 3)):
        records.append(cases.record(h, w, H, W, hflip, vflip, kind="random"))
        shifts.append(shift)
    got = run(records, shifts)
    want = {}
    for rec, (hflip, vflip), (image, labels, _, _) in zip(records, [f for f in cases.FLIPS for _ in range(3)], got):
        if (hflip, vflip) not in want:
            want[(hflip, vflip)] = cases.host_outputs(rec)[:2]
        assert np.array_equal(image, want[(hflip, vflip)][0]), (hflip, vflip)
        assert np.array_equal(labels, want[(hflip, vflip)][1]), (hflip, vflip)
        assert (labels == 255).any() or H * W < h * w


def test_resize_extreme_images(hip):
    """All-0, all-255 (coefficient sums and the final clip) and checkerboard sources, and images without a label map, in one
    launch of different sizes."""
    records = [cases.record(h, w, H, W, hflip, vflip, kind=kind, labels=kind != "checker")
               for ((h, w), (H, W)), kind, (hflip, vflip) in zip(cases.SIZE_PAIRS[1:8] * 2, ["zeros", "full", "checker"] * 5,
                                                                 cases.FLIPS * 4)]
    assert len(records) == 14
    check(records, run(records))


def mask_records():
    rs = np.random.RandomState(3)
    shapes = lambda h, w, H, W, hf, vf: cases.mask_shapes(h, w, dm.build_tables(h, w, H, W, hf, vf))  # noqa: E731
    down = shapes(37, 53, 24, 34, True, False)
    assert "vanishing" in down and len(down["checker"]) == 37 * 53
    big = shapes(256, 300, 128, 150, False, True)
    big["long_run"] = [100, 70000, 256 * 300 - 70100]  # a run longer than 65 535
    big["zero_length_runs"] = [0, 5, 0, 7, 256 * 300 - 12, 0, 0]
    up = shapes(48, 64, 80, 107, True, True)
    many = [cases.counts_of_mask(rs.rand(5, 3) > 0.5) for _ in range(33)]
    return [cases.record(37, 53, 24, 34, True, False, list(down.values())),
            cases.record(9, 5, 4, 5),                                        # no masks, between two images that have some
            cases.record(256, 300, 128, 150, False, True, list(big.values())),
            cases.record(5, 3, 5, 9, False, False, many),                    # 33 masks in one image
            cases.record(48, 64, 80, 107, True, True, list(up.values()))], down


def test_mask_kernel(hip):
    """Empty, full, corner pixels, one-row and one-column stripes, the h * w-run checkerboard, a run longer than 65 535,
    zero-length runs, the vanishing mask, 33 masks in one image, an image without masks between two with some, five images of
    different sizes in one launch and the first three in another; the counts equal the masks' sums."""
    records, down = mask_records()
    got = run(records)
    check(records, got)
    names = list(down.keys())
    counts = got[0][3]
    assert counts[names.index("vanishing")] == 0 and counts[names.index("empty")] == 0
    assert counts[names.index("full")] == 24 * 34 and got[1][2].shape == (0, 4, 5)
    check(records[:3], run(records[:3], [1, 3, 0]))


def test_contract_violations_are_refused_before_any_launch(hip):
    """Bad run ends and out-of-range table entries come back as status codes (-2, -3; a bad size or offset -1) and the outputs
    stay as they were: the launchers check the host copy of the tables and launch nothing."""
    lib = hip.load()
    h, w, H, W = 37, 53, 24, 34
    shapes = cases.mask_shapes(h, w)
    rec = cases.record(h, w, H, W, count_lists=[shapes["row_stripe"], shapes["full"]])
    meta, o = rec[dm.RAW_KEY], rec[dm.RAW_KEY]["offsets"]
    base = rec["dm_tables"].clone()
    ends0 = int(base[o["mask_offs"]])  # where the first mask's run ends begin
    n_ends0 = int(base[o["mask_offs"] + 1]) - ends0

    def statuses(edit=None, patch=None):
        r = dict(rec)
        r["dm_tables"] = base.clone()
        if edit is not None:
            edit(r["dm_tables"])
        dev, block, host = place([r])
        descs, img_bytes, lab_elems, mask_bytes, masks = dm.describe_batch(dev, block.data_ptr())
        if patch is not None:
            patch(descs[0])
        outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV) for n in (img_bytes, lab_elems * 8, mask_bytes)]
        counts = torch.full((masks,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        need = max(int(hip.call_nostream("u2_aug_resize_bilinear_scratch_bytes", descs, 1)), 0)
        scratch = torch.zeros(max(need, 1), dtype=torch.uint8, device=DEV)
        s = hip.stream_ptr()
        rc = (lib.u2_aug_resize_bilinear_u8(block.data_ptr(), block.numel(), host.data_ptr(), outs[0].data_ptr(), img_bytes,
                                            scratch.data_ptr(), need, descs, 1, s),
              lib.u2_aug_resize_nearest_u8(block.data_ptr(), block.numel(), host.data_ptr(), outs[1].data_ptr(), lab_elems,
                                           descs, 1, s),
              lib.u2_aug_rle_masks(block.data_ptr(), block.numel(), host.data_ptr(), outs[2].data_ptr(), mask_bytes,
                                   counts.data_ptr(), masks, descs, 1, s))
        torch.cuda.synchronize()
        untouched = tuple(bool((t == 0x5A).all()) for t in outs) + (bool((counts == 0x5A5A5A5A).all()),)
        return rc, untouched

    rc, untouched = statuses()
    assert rc == (0, 0, 0) and untouched == (False, False, False, False)  # the unedited record is served

    def set_(index, value):
        def edit(t):
            t[index] = value
        return edit

    # run ends: the last one is not h * w; not monotone; a mask without runs
    for edit in (set_(ends0 + n_ends0 - 1, h * w - 1), set_(ends0 + n_ends0 - 1, h * w + 1), set_(ends0, h * w),
                 set_(o["mask_offs"] + 1, ends0)):
        rc, untouched = statuses(edit)
        assert rc == (0, 0, -2) and untouched == (False, False, True, True)
    # nearest tables: an index one past the source, a negative one - refused by both calls that read them
    for edit in (set_(o["nx"] + 5, w), set_(o["ny"] + H - 1, -1)):
        rc, untouched = statuses(edit)
        assert rc == (0, -3, -3) and untouched == (False, True, True, True)
    # bilinear tables: taps that leave the row, no tap, more taps than coefficients, a row outside the scratch rows
    for edit in (set_(o["bx_bounds"] + 2 * (W - 1), w - 1), set_(o["bx_bounds"] + 1, 0), set_(o["by_bounds"] + 1, meta["ky"] + 1),
                 set_(o["by_bounds"], h - 1)):
        rc, untouched = statuses(edit)
        assert rc == (-3, 0, 0) and untouched == (True, False, False, False)
    # descriptors: a source that does not fit the block, sizes that make no sense
    rc, untouched = statuses(patch=lambda a: setattr(a, "src_offset", 1 << 40))
    assert rc[0] == -1 and untouched[0]
    rc, untouched = statuses(patch=lambda a: setattr(a, "H", 0))
    assert rc == (-1, -1, -1) and untouched == (True, True, True, True)
    rc, untouched = statuses(patch=lambda a: setattr(a, "mask_offs", 1 << 40))
    assert rc == (0, 0, -1) and untouched == (False, False, True, True)


@pytest.fixture(scope="module")
def small(hip):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import DatasetCatalog, MetadataCatalog, register_all_coco

    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "data_golden.json")))
    os.environ["CLUSTER_NUM"] = "800"
    for name in list(DatasetCatalog.keys()):
        DatasetCatalog.remove(name)
    for name in list(MetadataCatalog.keys()):
        MetadataCatalog.remove(name)
    register_all_coco(os.path.join(ROOT, "tests", "golden", "data_small"))
    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(fx["input_opts"] + ["SOLVER.IMS_PER_BATCH", 2, "MODEL.DEVICE", DEV])
    return cfg


def batches(cfg, workers, device_mapper, n, seed=4):
    """n batches in HBM from a freshly seeded loader (torch seeds the workers' numpy streams, numpy the single-process one)."""
    from u2seg_amd.data import DevicePrefetcher, build_detection_train_loader

    cfg = cfg.clone()
    cfg.merge_from_list(["DATALOADER.NUM_WORKERS", workers])
    torch.manual_seed(seed)
    np.random.seed(seed)
    pre = DevicePrefetcher(build_detection_train_loader(cfg, seed=3, device_mapper=device_mapper), DEV)
    return list(itertools.islice(iter(pre), n)), pre


def flip_of(sample, image_format):
    """Whether the host mapper flipped this sample: its image against the unflipped PIL resize of the file."""
    from u2seg_amd.data import detection_utils as utils
    from u2seg_amd.data import transforms as T

    src = utils.read_image(sample["file_name"], format=image_format)
    H, W = sample["image"].shape[1:]
    plain = T.ResizeTransform(src.shape[0], src.shape[1], H, W).apply_image(src)
    got = sample["image"].cpu().numpy().transpose(1, 2, 0)
    if np.array_equal(got, plain):
        return False
    assert np.array_equal(got, plain[:, ::-1])
    return True


def assert_same_batches(want, got, image_format):
    """Every tensor and value equal; returns the (flipped?, image size) of every sample."""
    seen = []
    for wb, gb in zip(want, got):
        assert len(wb) == len(gb)
        for a, b in zip(wb, gb):
            assert list(a.keys()) == list(b.keys())
            for k in a:
                if k not in ("image", "sem_seg", "instances"):
                    assert a[k] == b[k], k
            for k in ("image", "sem_seg"):
                assert b[k].is_cuda and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
            ai, bi = a["instances"], b["instances"]
            assert tuple(ai.image_size) == tuple(bi.image_size) and list(ai.get_fields()) == list(bi.get_fields())
            assert type(ai.gt_boxes) is type(bi.gt_boxes) and bi.gt_boxes.tensor.dtype == torch.float32
            assert torch.equal(ai.gt_boxes.tensor, bi.gt_boxes.tensor)
            assert bi.gt_classes.dtype == torch.int64 and torch.equal(ai.gt_classes, bi.gt_classes)
            if ai.has("gt_masks"):
                assert type(ai.gt_masks) is type(bi.gt_masks) and bi.gt_masks.tensor.dtype == torch.bool
                assert ai.gt_masks.tensor.shape == bi.gt_masks.tensor.shape and torch.equal(ai.gt_masks.tensor, bi.gt_masks.tensor)
            seen.append((flip_of(a, image_format), tuple(bi.image_size)))
    return seen


@pytest.mark.parametrize("workers", [0, 2])
def test_loader_to_hbm_equals_the_host_mapper(small, workers):
    """data_small through build_detection_train_loader(device_mapper=True) and DevicePrefetcher (the list path with no
    workers, the shared-memory slots with two) == the host mapper's batches, tensor for tensor, over twelve batches in which
    flipped and unflipped samples and at least five image sizes occur."""
    want, _ = batches(small, workers, False, 12)
    got, pre = batches(small, workers, True, 12)
    assert len(want) == len(got) == 12
    seen = assert_same_batches(want, got, small.INPUT.FORMAT)
    assert {f for f, _ in seen} == {False, True} and len({size for _, size in seen}) >= 5
    assert pre.seconds_waiting_for_counts >= 0.0 and (workers == 0 or pre.slot_bytes_moved > 0)
    ids = [d["image_id"] for b in got for d in b]
    assert 30 in ids  # the crowd-only image: instances without a gt_masks field


def test_batches_whose_every_mask_is_filtered(hip):
    """The by_mask filter firing for a whole batch: both images hold only a vanishing mask, or one does and the other has no
    instance at all, so nothing that is handed out is a view of the mask buffer or of the uploaded block (the surviving rows
    are gathered into new tensors on the consumer stream).  Such batches alternate with ordinary ones through the
    prefetcher, every batch is kept until the end, and all of them equal the host definitions."""
    from u2seg_amd.data import DevicePrefetcher

    h, w, H, W = 37, 53, 24, 34
    gone = lambda hf, vf: cases.mask_shapes(h, w, dm.build_tables(h, w, H, W, hf, vf))["vanishing"]  # noqa: E731
    shapes = cases.mask_shapes(h, w)
    vanishing = [cases.record(h, w, H, W, hf, vf, [gone(hf, vf)]) for hf, vf in cases.FLIPS]
    nothing = cases.record(9, 5, 4, 5)
    ordinary = [cases.record(h, w, H, W, hf, vf, [shapes["corner_tl"], gone(hf, vf), shapes["full"]]) for hf, vf in cases.FLIPS]
    stream = [[vanishing[0], vanishing[1]], [ordinary[0], ordinary[1]], [vanishing[2], nothing], [ordinary[2], vanishing[3]],
              [nothing, vanishing[0]], [ordinary[3], ordinary[0]], [vanishing[1], vanishing[2]], [ordinary[1], ordinary[2]]]
    pre = DevicePrefetcher(stream, DEV)
    got = list(pre)
    torch.cuda.synchronize()
    assert len(got) == len(stream)
    kept = []
    for raw_batch, batch in zip(stream, got):
        assert len(raw_batch) == len(batch)
        for raw, d in zip(raw_batch, batch):
            want = dm.finish_on_host(raw)
            assert list(want.keys()) == list(d.keys())
            assert torch.equal(want["image"], d["image"].cpu()) and torch.equal(want["sem_seg"], d["sem_seg"].cpu())
            wi, di = want["instances"], d["instances"]
            assert list(wi.get_fields()) == list(di.get_fields()) and len(wi) == len(di)
            assert di.gt_boxes.tensor.shape == (len(wi), 4) and torch.equal(wi.gt_boxes.tensor, di.gt_boxes.tensor.cpu())
            assert torch.equal(wi.gt_classes, di.gt_classes.cpu())
            assert di.gt_masks.tensor.shape == (len(wi), want["image"].shape[1], want["image"].shape[2])
            assert torch.equal(wi.gt_masks.tensor, di.gt_masks.tensor.cpu())
            kept.append(len(di))
    assert kept == [0, 0, 2, 2, 0, 0, 2, 0, 0, 0, 2, 2, 0, 0, 2, 2]


def test_training_steps_from_either_loader(small):
    """Three SimpleTrainer steps on the model of the small configuration, fed by either loader from the same seeds.  The
    batches are equal bit for bit (test_loader_to_hbm_equals_the_host_mapper); the losses are not compared with ==, because a
    training step of this model does not repeat exactly on equal inputs: csrc/losses.hip and the weight-gradient kernels
    accumulate with float atomics.  Measured on the MI355X with the host loader run twice from the same seeds
    (DESIGN.md 17): the ten losses of step 0 differ by at most 5.1e-7 relative, those of steps 1 and 2 by 2e-6 .. 1.0.
    - Step 0 (same weights, same inputs) is compared: relative difference at most 5e-6, ten times that host-against-host
      spread (measured between the two loaders: at most 4.9e-7).
    - Steps 1 and 2 are a smoke check and nothing more: ten finite losses with the same names from either loader."""
    from u2seg_amd.engine.trainer import SimpleTrainer
    from u2seg_amd.layers import functional as F
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer

    def three_steps(device_mapper):
        data, _ = batches(small, 0, device_mapper, 3, seed=9)
        torch.manual_seed(0)
        model = build_model(small)
        model.train()
        opt = build_optimizer(small, model)
        trainer = SimpleTrainer(model, opt, build_lr_scheduler(small, opt))
        out = []
        for batch in data:
            losses = trainer.run_step(batch)
            out.append({k: float(v.detach()) for k, v in losses.items()})
        return out

    F.set_deterministic_stats(True)
    try:
        host, device = three_steps(False), three_steps(True)
    finally:
        F.set_deterministic_stats(False)
    for step, (a, b) in enumerate(zip(host, device)):
        print("\nstep", step, "host", a, "device", b)
    assert len(host) == len(device) == 3
    for a, b in zip(host, device):
        assert len(a) == 10 and list(a.keys()) == list(b.keys())
        assert all(np.isfinite(v) for v in a.values()) and all(np.isfinite(v) for v in b.values())
    for k in host[0]:
        assert device[0][k] == pytest.approx(host[0][k], rel=5e-6, abs=0.0), k
