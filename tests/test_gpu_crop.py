"""INPUT.CROP on the GPU: u2_aug_rle_masks_boxes (u2seg_amd/csrc/augment.hip) against the host definitions - `host_masks` through
the window and `BitMasks.get_bounding_boxes`, both pinned on the CPU in tests/test_crop_host.py -, its contract checks, the
loader -> DevicePrefetcher path with the crop against the host mapper's batches, and the calls a batch issues.  Integers
throughout: every comparison is ==.  Every launched case keeps the contract (the windows lie inside their annotations, checked
here before anything is placed); the violations are refused on the host before anything is launched."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests import device_mapper_cases as cases
from u2seg_amd.data import device_mapper as dm
from u2seg_amd.structures import BitMasks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
CROP = ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "absolute", "INPUT.CROP.SIZE", [20, 24]]
PARENT_CALLS = ["u2_aug_resize_bilinear_u8", "u2_aug_resize_nearest_u8", "u2_aug_rle_masks"]

# (annotation (mask_h, mask_w), window (x0, y0, ch, cw), output (H, W)): output widths 1, 63, 64, 65, 257 (past one 256-thread
# column block), heights 1, 31, 32, 33 (the 32-row chunk edge); windows at the origin, inside, and flush with the far corner or
# one far side; down- and up-sampling; the whole annotation as its own window
GEOMETRIES = [((80, 110), (0, 0, 40, 60), (31, 63)),
              ((80, 110), (13, 7, 40, 60), (32, 64)),
              ((80, 110), (50, 40, 40, 60), (33, 65)),
              ((80, 110), (30, 20, 50, 80), (1, 257)),
              ((37, 53), (5, 3, 20, 30), (33, 1)),
              ((80, 110), (10, 70, 10, 100), (31, 257)),
              ((80, 110), (0, 0, 80, 110), (64, 88))]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


def window_masks(mask_h, mask_w, window, tables):
    """Named masks [mask_h, mask_w] of the windowed kernel's cases."""
    x0, y0, ch, cw = window
    out = {"empty": np.zeros((mask_h, mask_w), dtype=np.uint8), "full": np.ones((mask_h, mask_w), dtype=np.uint8)}

    def pixel(y, x):
        m = np.zeros((mask_h, mask_w), dtype=np.uint8)
        m[y, x] = 1
        return m

    for name, (y, x) in {"in_tl": (y0, x0), "in_tr": (y0, x0 + cw - 1), "in_bl": (y0 + ch - 1, x0),
                         "in_br": (y0 + ch - 1, x0 + cw - 1)}.items():
        out[name] = pixel(y, x)
    for name, (y, x) in {"out_left": (y0 + ch // 2, x0 - 1), "out_right": (y0 + ch // 2, x0 + cw), "out_top": (y0 - 1, x0 + cw // 2),
                         "out_bottom": (y0 + ch, x0 + cw // 2)}.items():
        if 0 <= y < mask_h and 0 <= x < mask_w:  # a window flush with a side has nothing outside it there
            out[name] = pixel(y, x)
    skipped = cases.unsampled_pixel(ch, cw, tables)
    if skipped is not None:
        out["vanishing"] = pixel(y0 + skipped[0], x0 + skipped[1])
    m = np.zeros((mask_h, mask_w), dtype=np.uint8)
    m[::3, :] = 1
    m[:, mask_w // 2] = 1
    out["stripes"] = m
    m = np.zeros((mask_h, mask_w), dtype=np.uint8)  # a ring around the window's top-left corner: one quarter of it is inside
    ry, rx = max(ch // 3, 1), max(cw // 3, 1)
    ya, yb, xa, xb = max(y0 - ry, 0), min(y0 + ry, mask_h - 1), max(x0 - rx, 0), min(x0 + rx, mask_w - 1)
    m[ya:yb + 1, xa:xb + 1] = 1
    m[ya + 1:yb, xa + 1:xb] = 0
    out["ring"] = m
    return out


def crop_record(geometry, hflip=False, vflip=False, names=None, recompute=True):
    """A raw record of a cropped sample built without files: (record, names of its masks)."""
    (mask_h, mask_w), (x0, y0, ch, cw), (H, W) = geometry
    assert 0 <= x0 and 0 <= y0 and x0 + cw <= mask_w and y0 + ch <= mask_h
    img, lab = cases.source(mask_h, mask_w)
    tables = dm.build_tables(ch, cw, H, W, hflip, vflip)
    masks = window_masks(mask_h, mask_w, (x0, y0, ch, cw), tables)
    if names is not None:
        masks = {k: masks[k] for k in names}
    ends = [dm.run_ends(cases.counts_of_mask(m), mask_h, mask_w) for m in masks.values()]
    boxes = np.tile(np.array([[0, 0, W, H]], dtype=np.float32), (len(ends), 1))
    rec = dm.make_raw_record({"height": mask_h, "width": mask_w, "image_id": 1000 * mask_h + mask_w},
                             img[y0:y0 + ch, x0:x0 + cw], lab[y0:y0 + ch, x0:x0 + cw], tables, ends, boxes, list(range(len(ends))),
                             has_masks=True, window=(x0, y0, mask_h, mask_w), recompute_boxes=recompute)
    return rec, list(masks.keys())


def place(records):
    """The records' tensors in one host block and its device copy, 256-byte aligned like the slots lay them out: (records with
    device views, device block, host block)."""
    cursor, where = 0, []
    for rec in records:
        at = {}
        for k in dm.TENSOR_KEYS:
            if k in rec:
                at[k] = cursor
                cursor = (cursor + rec[k].numel() * rec[k].element_size() + 255) // 256 * 256
        where.append(at)
    host = torch.zeros(max(cursor, 256), dtype=torch.uint8)
    for rec, at in zip(records, where):
        for k, off in at.items():
            n = rec[k].numel() * rec[k].element_size()
            host[off:off + n] = rec[k].contiguous().reshape(-1).view(torch.uint8)
    block = host.to(DEV)
    out = []
    for rec, at in zip(records, where):
        d = {k: v for k, v in rec.items() if k not in dm.TENSOR_KEYS}
        for k, off in at.items():
            n = rec[k].numel() * rec[k].element_size()
            d[k] = block[off:off + n].view(rec[k].dtype).view(rec[k].shape)
        out.append(d)
    return out, block, host


def host_outputs(rec):
    """(image, label map, masks bool [N, H, W], counts int32 [N], tight boxes int [N, 4]) of a raw record by the host definitions."""
    meta = rec[dm.RAW_KEY]
    tables, ends = dm.unpack_tables(meta, rec["dm_tables"].numpy())
    tables["x_identity"], tables["y_identity"] = meta["x_identity"], meta["y_identity"]
    masks, counts = dm.host_masks(ends, meta["h"], tables, meta.get("window"))
    boxes = BitMasks(torch.from_numpy(masks)).get_bounding_boxes().tensor.numpy()
    assert np.array_equal(boxes, np.round(boxes))
    return (dm.host_image(rec["dm_image"].numpy(), tables), dm.host_labels(rec["dm_sem_seg"].numpy(), tables), masks, counts,
            boxes.astype(np.int32))


def test_windowed_decode_and_tight_boxes(hip):
    """Every geometry with the four flips and a record without masks in the middle: 29 images in one batch (two launches of
    the mask kernel, first_mask offsets past the gap).  Masks: empty, full, one pixel in each corner of the window, one pixel
    just outside each side (empty, zero box), a pixel of the window the nearest tables skip, stripes, a ring that the window cuts."""
    records, names = [], []
    for geometry, (hflip, vflip) in itertools.product(GEOMETRIES, cases.FLIPS):
        rec, n = crop_record(geometry, hflip, vflip)
        records.append(rec)
        names.append(n)
    no_masks, _ = crop_record(GEOMETRIES[1], names=[])
    records.insert(14, no_masks)
    names.insert(14, [])
    assert len(records) == 29 and no_masks[dm.RAW_KEY]["num_masks"] == 0
    dev, block, host = place(records)
    pending = dm.launch_batch(dev, block, host)
    torch.cuda.synchronize()
    assert pending.boxes is not None and pending.boxes.dtype == torch.int32
    all_boxes = pending.boxes.cpu().numpy()
    assert all_boxes.shape == (sum(len(n) for n in names), 4)
    seen, partial = set(), set()
    for i, (rec, mask_names) in enumerate(zip(records, names)):
        image, labels, masks, counts = pending.outputs(i)
        want_image, want_labels, want_masks, want_counts, want_boxes = host_outputs(rec)
        assert np.array_equal(image.cpu().numpy(), want_image) and np.array_equal(labels.cpu().numpy(), want_labels), i
        masks = masks.cpu().numpy()
        assert masks.shape == want_masks.shape and np.array_equal(masks, want_masks), i
        assert np.array_equal(counts.numpy(), want_counts), i
        first = pending.descs[i].first_mask
        got_boxes = all_boxes[first:first + len(mask_names)]
        assert np.array_equal(got_boxes, want_boxes), (i, got_boxes.tolist(), want_boxes.tolist())
        H, W = rec[dm.RAW_KEY]["H"], rec[dm.RAW_KEY]["W"]
        for k, name in enumerate(mask_names):
            seen.add(name)
            if name == "empty" or name == "vanishing" or name.startswith("out_"):
                assert want_counts[k] == 0 and want_boxes[k].tolist() == [0, 0, 0, 0], (i, name)
            elif name == "full":
                assert want_counts[k] == H * W and want_boxes[k].tolist() == [0, 0, W, H], (i, name)
            elif want_counts[k]:  # (a strong downscale samples neither the window's corners nor every stripe)
                partial.add(name)
                if name.startswith("in_"):
                    assert want_boxes[k][0] == 0 or want_boxes[k][2] == W, (i, name)
                    assert want_boxes[k][1] == 0 or want_boxes[k][3] == H, (i, name)
                    assert want_boxes[k][2] - want_boxes[k][0] < max(W, 2) or want_boxes[k][3] - want_boxes[k][1] < max(H, 2)
    everything = {"empty", "full", "in_tl", "in_tr", "in_bl", "in_br", "out_left", "out_right", "out_top", "out_bottom", "vanishing",
                  "stripes", "ring"}
    assert seen == everything and partial == {"in_tl", "in_tr", "in_bl", "in_br", "stripes", "ring"}
    # PendingBatch.finish: the rows with a pixel, the boxes from the device, still on the device
    for rec, out in zip(records, pending.finish()):
        want = dm.finish_on_host(rec)
        wi, gi = want["instances"], out["instances"]
        assert gi.gt_boxes.tensor.is_cuda and gi.gt_boxes.tensor.dtype == torch.float32
        assert torch.equal(wi.gt_boxes.tensor, gi.gt_boxes.tensor.cpu()) and torch.equal(wi.gt_classes, gi.gt_classes.cpu())
        assert torch.equal(wi.gt_masks.tensor, gi.gt_masks.tensor.cpu())
        assert bool((wi.gt_boxes.tensor[:, 2] > wi.gt_boxes.tensor[:, 0]).all())


def masks_call(hip, entry, records, windows=None, edit_desc=None, boxes="alloc"):
    """One of the two mask entries on sentinel-filled outputs: (status, mask_out, counts, boxes) on the host."""
    lib = hip.load()
    dev, block, host = place(records)
    descs, _, _, mask_bytes, masks = dm.describe_batch(dev, block.data_ptr())
    if edit_desc is not None:
        edit_desc(descs)
    mask_out = torch.full((max(mask_bytes, 1),), 0x5A, dtype=torch.uint8, device=DEV)
    counts = torch.full((max(masks, 1),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    box_out = torch.full((max(masks, 1), 4), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    s = hip.stream_ptr()
    if entry == "u2_aug_rle_masks":
        rc = lib.u2_aug_rle_masks(block.data_ptr(), block.numel(), host.data_ptr(), mask_out.data_ptr(), mask_bytes,
                                  counts.data_ptr(), masks, descs, len(records), s)
    else:
        rc = lib.u2_aug_rle_masks_boxes(block.data_ptr(), block.numel(), host.data_ptr(), mask_out.data_ptr(), mask_bytes,
                                        counts.data_ptr(), box_out.data_ptr() if boxes == "alloc" else None, masks, descs, windows,
                                        len(records), s)
    torch.cuda.synchronize()
    return rc, mask_out.cpu().numpy(), counts.cpu().numpy(), box_out.cpu().numpy()


def whole_windows(records):
    windows = (dm._AugWindow * len(records))()
    for win, rec in zip(windows, records):
        win.x0, win.y0, win.mask_h, win.mask_w = 0, 0, rec[dm.RAW_KEY]["h"], rec[dm.RAW_KEY]["w"]
    return windows


def test_whole_window_equals_the_plain_entry(hip):
    """With the window (0, 0, h, w) mask_out and counts are byte-equal to u2_aug_rle_masks' on the same records (the sentinel
    bytes of the alignment gaps included)."""
    shapes = lambda h, w, H, W, hf, vf: list(cases.mask_shapes(h, w, dm.build_tables(h, w, H, W, hf, vf)).values())  # noqa: E731
    records = [cases.record(37, 53, 24, 34, True, False, shapes(37, 53, 24, 34, True, False)),
               cases.record(9, 5, 4, 5),
               cases.record(48, 64, 80, 107, True, True, shapes(48, 64, 80, 107, True, True)),
               cases.record(33, 71, 65, 257, False, True, shapes(33, 71, 65, 257, False, True))]
    assert dm.describe_windows(records) is None
    rc0, masks0, counts0, _ = masks_call(hip, "u2_aug_rle_masks", records)
    rc1, masks1, counts1, boxes1 = masks_call(hip, "u2_aug_rle_masks_boxes", records, whole_windows(records))
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(masks0, masks1) and np.array_equal(counts0, counts1) and (masks0 == 1).any() and (counts0 > 0).any()
    want = np.concatenate([host_outputs(r)[4] for r in records if r[dm.RAW_KEY]["num_masks"]])
    assert np.array_equal(boxes1, want)


def test_window_violations_are_refused_before_any_launch(hip):
    """A window that leaves the annotation on any side, a negative origin, no boxes, run ends that do not total mask_h * mask_w:
    a negative status, and the sentinel-filled outputs stay as they were."""
    geometry = ((37, 53), (5, 3, 20, 30), (24, 34))
    rec, _ = crop_record(geometry, names=["full", "stripes"])

    def status(window, **kw):
        windows = (dm._AugWindow * 1)()
        windows[0].x0, windows[0].y0, windows[0].mask_h, windows[0].mask_w = window
        rc, masks, counts, boxes = masks_call(hip, "u2_aug_rle_masks_boxes", [rec], windows, **kw)
        return rc, bool((masks == 0x5A).all() and (counts == 0x5A5A5A5A).all() and (boxes == 0x5A5A5A5A).all())

    rc, untouched = status((5, 3, 37, 53))
    assert rc == 0 and not untouched  # the record as it is, is served
    assert status((53 - 30, 37 - 20, 37, 53))[0] == 0  # flush with the far corner: still inside
    for bad in ((53 - 30 + 1, 3, 37, 53),    # leaves on the right
                (5, 37 - 20 + 1, 37, 53),    # leaves at the bottom
                (-1, 3, 37, 53),             # a negative origin: leaves on the left
                (5, -1, 37, 53),             # ... at the top
                (0, 0, 19, 53 * 37 // 19)):  # an annotation lower than the window
        rc, untouched = status(bad)
        assert rc == -1 and untouched, bad
    rc, untouched = status((5, 3, 37, 53), boxes=None)
    assert rc == -1 and untouched
    # run ends of 37 x 53 under a window that states another annotation size: the last run end is not mask_h * mask_w
    for bad in ((5, 3, 38, 53), (5, 3, 37, 54), (0, 0, 20, 30)):
        rc, untouched = status(bad)
        assert rc == -2 and untouched, bad
    rc, untouched = status((5, 3, 1 << 16, 1 << 15))  # mask_h * mask_w = 2^31
    assert rc == -1 and untouched
    lib = hip.load()
    assert lib.u2_aug_rle_masks_boxes(None, 0, None, None, 0, None, None, 0, None, None, 1, None) == -1


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


def assert_same_batches(want, got):
    """Every tensor and value equal; returns (image id, instances kept, image size) of every sample."""
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
            assert bi.gt_boxes.tensor.is_cuda and torch.equal(ai.gt_boxes.tensor, bi.gt_boxes.tensor)
            assert bi.gt_classes.dtype == torch.int64 and torch.equal(ai.gt_classes, bi.gt_classes)
            if ai.has("gt_masks"):
                assert type(ai.gt_masks) is type(bi.gt_masks) and bi.gt_masks.tensor.dtype == torch.bool
                assert ai.gt_masks.tensor.shape == bi.gt_masks.tensor.shape and torch.equal(ai.gt_masks.tensor, bi.gt_masks.tensor)
                assert torch.equal(bi.gt_masks.get_bounding_boxes().tensor, bi.gt_boxes.tensor)
            seen.append((a["image_id"], len(bi), tuple(bi.image_size)))
    return seen


@pytest.mark.parametrize("workers", [0, 2])
def test_loader_to_hbm_equals_the_host_mapper_with_crop(small, workers):
    """data_small with INPUT.CROP absolute [20, 24] through build_detection_train_loader(device_mapper=True) and DevicePrefetcher
    == the host mapper's batches, field by field, over twelve batches: instances are dropped (an image keeps one of its two),
    the crowd-only image comes through without a gt_masks field, and the boxes are the tight boxes of the masks."""
    cfg = small.clone()
    cfg.merge_from_list(CROP)
    want, _ = batches(cfg, workers, False, 12)
    got, pre = batches(cfg, workers, True, 12)
    assert len(want) == len(got) == 12
    seen = assert_same_batches(want, got)
    assert any(i in (10, 20, 40) and n == 1 for i, n, _ in seen)  # every such image has two non-crowd instances
    assert any(i in (10, 20, 40) and n == 2 for i, n, _ in seen) and any(i == 30 for i, _, _ in seen)
    assert len({size for _, _, size in seen}) >= 3 and (workers == 0 or pre.slot_bytes_moved > 0)


def test_batches_whose_every_mask_the_crop_removes(hip):
    """The crop removing every mask of an image (data_small's objects are too large for that to happen there): both images of a
    batch, or one of them next to an ordinary one, through the prefetcher; all equal the host definitions."""
    from u2seg_amd.data import DevicePrefetcher

    gone = ["empty", "out_left", "out_right", "out_top", "out_bottom"]
    g = GEOMETRIES[1]
    lost = [crop_record(g, hf, vf, names=gone)[0] for hf, vf in cases.FLIPS]
    ordinary = [crop_record(g, hf, vf, names=["in_tl", "out_left", "ring", "full"])[0] for hf, vf in cases.FLIPS]
    stream = [[lost[0], lost[1]], [ordinary[0], lost[2]], [lost[3], ordinary[1]], [ordinary[2], ordinary[3]]]
    got = list(DevicePrefetcher(stream, DEV))
    torch.cuda.synchronize()
    kept = []
    for raw_batch, batch in zip(stream, got):
        for raw, d in zip(raw_batch, batch):
            want = dm.finish_on_host(raw)
            assert list(want.keys()) == list(d.keys())
            assert torch.equal(want["image"], d["image"].cpu()) and torch.equal(want["sem_seg"], d["sem_seg"].cpu())
            wi, di = want["instances"], d["instances"]
            assert list(wi.get_fields()) == list(di.get_fields()) and len(wi) == len(di)
            assert di.gt_boxes.tensor.shape == (len(wi), 4) and torch.equal(wi.gt_boxes.tensor, di.gt_boxes.tensor.cpu())
            assert torch.equal(wi.gt_classes, di.gt_classes.cpu()) and torch.equal(wi.gt_masks.tensor, di.gt_masks.tensor.cpu())
            kept.append(len(di))
    assert kept == [0, 0, 3, 0, 0, 3, 3, 3]


def test_training_steps_from_either_loader_with_crop(small):
    """Three SimpleTrainer steps with the crop on, fed by either loader from the same seeds.  The batches are equal bit for bit
    (the test above); the criterion is the one tests/test_gpu_device_mapper.py states and derives for the uncropped path: a
    step of this model does not repeat exactly on equal inputs (float atomics), so the ten losses of step 0 agree to 5e-6
    relative, ten times the measured host-against-host spread, and steps 1 and 2 give ten finite losses of the same names."""
    from u2seg_amd.engine.trainer import SimpleTrainer
    from u2seg_amd.layers import functional as F
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer

    cfg = small.clone()
    cfg.merge_from_list(CROP)

    def three_steps(device_mapper):
        data, _ = batches(cfg, 0, device_mapper, 3, seed=9)
        torch.manual_seed(0)
        model = build_model(cfg)
        model.train()
        opt = build_optimizer(cfg, model)
        trainer = SimpleTrainer(model, opt, build_lr_scheduler(cfg, opt))
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


def test_launch_census(small, hip, monkeypatch):
    """The entries a batch passes to _hip.call.  Crop off: exactly the three of the parent.  Crop on with masks:
    u2_aug_rle_masks_boxes in the place of u2_aug_rle_masks and nothing else.  Crop on without masks: no mask call at all."""
    from u2seg_amd.data import get_detection_dataset_dicts

    names = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])

    def census(cfg):
        dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=True)
        mapper = dm.DeviceMapper(cfg, True)
        np.random.seed(2)
        dev, block, host = place([mapper(d) for d in dicts[:2]])
        del names[:]
        pending = dm.launch_batch(dev, block, host)
        torch.cuda.synchronize()
        return list(names), pending

    called, pending = census(small)
    assert called == PARENT_CALLS and pending.boxes is None
    cfg = small.clone()
    cfg.merge_from_list(CROP)
    called, pending = census(cfg)
    assert called == PARENT_CALLS[:2] + ["u2_aug_rle_masks_boxes"] and pending.boxes is not None
    cfg.merge_from_list(["MODEL.MASK_ON", False])
    called, pending = census(cfg)
    assert called == PARENT_CALLS[:2] and pending.boxes is None
    for rec in pending.finish():
        assert not rec["instances"].has("gt_masks") and rec["instances"].gt_boxes.tensor.shape[1] == 4
