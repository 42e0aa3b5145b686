"""INPUT.CROP on the CPU: RandomCrop / CropTransform / BitMasks.get_bounding_boxes, `DatasetMapper` with the crop against what
the reference's mapper returned (tests/golden/crop_golden.*, made by tests/golden/make_crop_fixture.py), `DeviceMapper` + the
host definitions against `DatasetMapper`, and the guard of the default path.  Integers throughout: every comparison is ==."""
import copy
import json
import os
import zlib

import numpy as np
import pytest
import torch

from u2seg_amd.config import get_cfg
from u2seg_amd.data import DatasetCatalog, DatasetMapper, MetadataCatalog, get_detection_dataset_dicts, register_all_coco
from u2seg_amd.data import device_mapper as dm
from u2seg_amd.data import transforms as T
from u2seg_amd.structures import BitMasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def golden():
    os.environ["CLUSTER_NUM"] = "800"
    for name in list(DatasetCatalog.keys()):
        DatasetCatalog.remove(name)
    for name in list(MetadataCatalog.keys()):
        MetadataCatalog.remove(name)
    register_all_coco(os.path.join(GOLD, "data_small"))
    listing = json.load(open(os.path.join(GOLD, "crop_golden.json")))
    arrays = np.load(os.path.join(GOLD, "crop_golden.npz"))
    return listing, arrays


def crop_cfg(listing, setting=None):
    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(listing["input_opts"] + ["DATALOADER.NUM_WORKERS", 0])
    if setting is not None:
        cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", setting["type"], "INPUT.CROP.SIZE", setting["size"]])
    return cfg


def surviving(cfg):
    """The three images of data_small with a non-crowd annotation, in the order of the fixture's `index`."""
    dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=True)
    assert len(dicts) == 3
    return dicts


def test_dataset_mapper_reproduces_the_reference(golden):
    """Every case of crop_golden bit for bit under the stored seed: image, label map (pixels for seed 0, crc32 + shape for seeds
    1-4, as stored), boxes (fp32 ==), classes, masks, image_size, and the position of numpy's global stream afterwards."""
    listing, arrays = golden
    assert [(s["type"], s["dropped"]) for s in listing["settings"]] == [("relative_range", 0), ("relative", 2), ("absolute", 2),
                                                                        ("absolute_range", 1)]
    for setting in listing["settings"]:
        cfg = crop_cfg(listing, setting)
        dicts, mapper = surviving(cfg), DatasetMapper(cfg, True)
        assert mapper.recompute_boxes and isinstance(mapper.augmentations.augs[0], T.RandomCrop)
        kept = 0
        for case in setting["cases"]:
            key, d = case["key"], dicts[case["index"]]
            before = copy.deepcopy(d)
            np.random.seed(case["np_seed"])
            out = mapper(d)
            assert float(np.random.rand()) == case["next_rand"], key
            assert d == before and sorted(out.keys()) == case["keys"]
            image, sem = out["image"].numpy(), out["sem_seg"].numpy()
            assert image.dtype == np.uint8 and sem.dtype == np.int64
            assert list(image.shape) == case["image_shape"] and list(sem.shape) == case["sem_seg_shape"]
            assert crc(image) == case["image_crc32"] and crc(sem.astype(np.uint8)) == case["sem_seg_crc32"], key
            if case["pixels"]:
                assert np.array_equal(image, arrays[key + "_image"]) and np.array_equal(sem, arrays[key + "_sem_seg"]), key
            inst = out["instances"]
            assert list(inst.image_size) == case["image_size"] == list(image.shape[1:])
            assert sorted(inst.get_fields().keys()) == case["instance_fields"]
            boxes = inst.gt_boxes.tensor.numpy()
            assert boxes.dtype == np.float32 and np.array_equal(boxes, arrays[key + "_boxes"]), key
            assert np.array_equal(inst.gt_classes.numpy(), arrays[key + "_classes"]), key
            assert np.array_equal(np.packbits(inst.gt_masks.tensor.numpy(), axis=-1), arrays[key + "_masks"]), key
            assert len(inst) == case["num_instances"]
            kept += len(inst)
        assert setting["instances"] - kept == setting["dropped"]


def assert_same_sample(want, got):
    assert list(want.keys()) == list(got.keys())
    for k in want:
        if k not in ("image", "sem_seg", "instances"):
            assert want[k] == got[k], k
    assert got["image"].dtype == torch.uint8 and torch.equal(want["image"], got["image"])
    assert got["sem_seg"].dtype == torch.int64 and torch.equal(want["sem_seg"], got["sem_seg"])
    wi, gi = want["instances"], got["instances"]
    assert tuple(wi.image_size) == tuple(gi.image_size)
    assert list(wi.get_fields().keys()) == list(gi.get_fields().keys())
    assert gi.gt_boxes.tensor.dtype == torch.float32 and torch.equal(wi.gt_boxes.tensor, gi.gt_boxes.tensor)
    assert gi.gt_classes.dtype == torch.int64 and torch.equal(wi.gt_classes, gi.gt_classes)
    if wi.has("gt_masks"):
        assert gi.gt_masks.tensor.dtype == torch.bool and torch.equal(wi.gt_masks.tensor, gi.gt_masks.tensor)


def test_device_mapper_equals_dataset_mapper_with_crop(golden):
    """DeviceMapper + finish_on_host == DatasetMapper for the fixture's seeds and settings, with the same draws from numpy's
    global stream.  The raw record holds the window's pixels, the window's place and the run ends of the WHOLE annotation, for
    every non-crowd instance (nothing is dropped by its box on the host)."""
    listing, _ = golden
    for setting in listing["settings"]:
        cfg = crop_cfg(listing, setting)
        dicts, host, device = surviving(cfg), DatasetMapper(cfg, True), dm.DeviceMapper(cfg, True)
        smaller = 0
        for case in setting["cases"]:
            d = dicts[case["index"]]
            np.random.seed(case["np_seed"])
            want = host(d)
            after_host = np.random.get_state()
            np.random.seed(case["np_seed"])
            raw = device(d)
            after_device = np.random.get_state()
            assert after_host[0] == after_device[0] and np.array_equal(after_host[1], after_device[1])
            assert after_host[2:] == after_device[2:]
            meta = raw[dm.RAW_KEY]
            x0, y0, mask_h, mask_w = meta["window"]
            assert (mask_h, mask_w) == (d["height"], d["width"]) and meta["recompute_boxes"]
            assert 0 <= x0 and 0 <= y0 and x0 + meta["w"] <= mask_w and y0 + meta["h"] <= mask_h
            assert tuple(raw["dm_image"].shape) == (meta["h"], meta["w"], 3) and raw["dm_image"].is_contiguous()
            assert tuple(raw["dm_sem_seg"].shape) == (meta["h"], meta["w"]) and raw["dm_sem_seg"].is_contiguous()
            smaller += (meta["h"], meta["w"]) != (mask_h, mask_w)
            _, ends = dm.unpack_tables(meta, raw["dm_tables"].numpy())
            assert len(ends) == sum(1 for a in d["annotations"] if not a.get("iscrowd", 0)) == raw["dm_boxes"].shape[0]
            assert all(int(e[-1]) == mask_h * mask_w for e in ends)
            assert_same_sample(want, dm.finish_on_host(raw))
        assert smaller


@pytest.mark.parametrize("crop_type, crop_size, image_size, draws, want", [
    ("relative", (0.5, 0.4), (48, 64), None, (24, 26)),          # 64 * 0.4 = 25.6 -> 26
    ("relative", (0.5, 0.5), (5, 7), None, (3, 4)),              # 2.5 and 3.5 round half up, unlike round()
    ("relative", (1.0, 1.0), (36, 72), None, (36, 72)),
    ("absolute", (20, 24), (48, 64), None, (20, 24)),
    ("absolute", (50, 24), (36, 20), None, (36, 20)),            # larger than the image: the image
    ("relative_range", (0.9, 0.9), (40, 60), "rand", None),
    ("absolute_range", (12, 40), (36, 72), "randint", None),
])
def test_random_crop_sizes(crop_type, crop_size, image_size, draws, want):
    h, w = image_size
    aug = T.RandomCrop(crop_type, crop_size)
    np.random.seed(7)
    got = aug.get_crop_size((h, w))
    if draws is None:
        assert got == want
        np.random.seed(7)
        np.random.rand()  # no draw was made for the size
        state = np.random.get_state()[2]
        np.random.seed(7)
        aug.get_crop_size((h, w))
        np.random.rand()
        assert np.random.get_state()[2] == state
    elif draws == "rand":
        np.random.seed(7)
        r = np.random.rand(2)
        c = np.asarray(crop_size, dtype=np.float32)  # the fp32 detour of the reference: 0.9 is 0.89999998
        ch, cw = c + r * (1 - c)
        assert got == (int(h * ch + 0.5), int(w * cw + 0.5)) and 36 <= got[0] <= 40 and 54 <= got[1] <= 60
    else:
        np.random.seed(7)
        want = (np.random.randint(12, 36 + 1), np.random.randint(12, 40 + 1))  # min(h, 40) = 36 caps the height only
        assert got == want
    np.random.seed(3)
    t = aug.get_transform(np.zeros((h, w, 3), dtype=np.uint8))
    assert isinstance(t, T.CropTransform) and 0 <= t.x0 <= w - t.w and 0 <= t.y0 <= h - t.h
    np.random.seed(3)
    ch, cw = aug.get_crop_size((h, w))
    assert (t.h, t.w) == (ch, cw) and (t.y0, t.x0) == (np.random.randint(h - ch + 1), np.random.randint(w - cw + 1))


def test_random_crop_refuses_what_it_does_not_know():
    with pytest.raises(ValueError, match="INPUT.CROP.TYPE"):
        T.RandomCrop("relative_area", (0.5, 0.5))
    with pytest.raises(AssertionError):
        T.RandomCrop("absolute_range", (40, 12)).get_crop_size((50, 50))


def test_crop_transform():
    t = T.CropTransform(3, 2, 5, 4, 20, 10)
    img = np.arange(10 * 20 * 3, dtype=np.uint8).reshape(10, 20, 3)
    assert np.array_equal(t.apply_image(img), img[2:6, 3:8])
    assert np.array_equal(t.apply_segmentation(img[:, :, 0]), img[2:6, 3:8, 0])
    assert np.array_equal(t.apply_coords(np.array([[3.0, 2.0], [10.5, 0.0]])), np.array([[0.0, 0.0], [7.5, -2.0]]))
    assert np.array_equal(t.apply_box(np.array([[4.0, 1.0, 9.0, 7.0]])), np.array([[1.0, -1.0, 6.0, 5.0]]))
    chain = T.TransformList([t, T.HFlipTransform(5)])
    assert np.array_equal(chain.apply_box(np.array([[4.0, 3.0, 6.0, 5.0]])), np.array([[2.0, 1.0, 4.0, 3.0]]))
    with pytest.raises(NotImplementedError, match="INPUT.MASK_FORMAT"):
        t.apply_polygons([np.zeros((3, 2))])


def test_get_bounding_boxes():
    h, w = 6, 9
    masks = np.zeros((7, h, w), dtype=bool)
    masks[1, 0, 0] = masks[2, 0, w - 1] = masks[3, h - 1, 0] = masks[4, h - 1, w - 1] = True
    masks[5] = True
    masks[6, 1:5, 2] = masks[6, 4, 2:7] = True  # an L
    got = BitMasks(torch.from_numpy(masks)).get_bounding_boxes()
    assert got.tensor.dtype == torch.float32
    want = [[0, 0, 0, 0], [0, 0, 1, 1], [w - 1, 0, w, 1], [0, h - 1, 1, h], [w - 1, h - 1, w, h], [0, 0, w, h], [2, 1, 7, 5]]
    assert got.tensor.tolist() == [[float(v) for v in row] for row in want]
    assert BitMasks(torch.zeros((0, h, w), dtype=torch.bool)).get_bounding_boxes().tensor.shape == (0, 4)
    # the reference's example: the triangle (0,0), (2,0), (0,2) - pixels {xx, x.} - cropped by the box [(1,0), (2,2)].  What is
    # left is one pixel with the tight box [(1,0), (2,1)] of the source, (0, 0, 1, 1) in the window; the annotation's box
    # cropped and clipped is the whole window (0, 0, 1, 2)
    crop = T.CropTransform(1, 0, 1, 2)
    left = crop.apply_segmentation(np.array([[1, 1], [1, 0]], dtype=bool))
    assert BitMasks(torch.from_numpy(np.ascontiguousarray(left))[None]).get_bounding_boxes().tensor.tolist() == [[0.0, 0.0, 1.0, 1.0]]
    assert np.clip(crop.apply_box(np.array([[0.0, 0.0, 2.0, 2.0]])), 0, [1, 2, 1, 2]).tolist() == [[0.0, 0.0, 1.0, 2.0]]


def crowd_only(cfg):
    dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=False)
    (d,) = [x for x in dicts if all(a.get("iscrowd", 0) for a in x["annotations"])]
    return d


def test_crowd_only_image_gives_empty_instances(golden):
    """The stated deviation: the reference raises AttributeError here (no gt_masks field to recompute from)."""
    listing, _ = golden
    cfg = crop_cfg(listing, listing["settings"][2])
    d = crowd_only(cfg)
    np.random.seed(5)
    want = DatasetMapper(cfg, True)(d)
    inst = want["instances"]
    assert len(inst) == 0 and not inst.has("gt_masks") and inst.gt_boxes.tensor.shape == (0, 4)
    assert tuple(inst.image_size) == tuple(want["image"].shape[1:])
    np.random.seed(5)
    assert_same_sample(want, dm.finish_on_host(dm.DeviceMapper(cfg, True)(d)))


def test_device_mapper_takes_the_crop_at_position_0_only():
    kw = dict(image_format="RGB", use_instance_mask=True, instance_mask_format="bitmask")
    crop, resize, flip = T.RandomCrop("relative", (0.5, 0.5)), T.ResizeShortestEdge((20, 20), 1333, "choice"), T.RandomFlip()
    dm.DeviceMapper(augmentations=[crop, resize, flip], **kw)
    with pytest.raises(NotImplementedError, match="position 1.*ResizeShortestEdge"):
        dm.DeviceMapper(augmentations=[resize, crop, flip], **kw)
    with pytest.raises(NotImplementedError, match="position 2.*RandomFlip"):
        dm.DeviceMapper(augmentations=[resize, flip, crop], **kw)
    with pytest.raises(NotImplementedError, match="position 1.*HFlipTransform"):
        dm.DeviceMapper(augmentations=[T.HFlipTransform(10), T.CropTransform(0, 0, 4, 4)], **kw)


def test_default_path_is_unchanged(golden):
    """INPUT.CROP.ENABLED: False - both mappers give what data_golden holds, the raw record carries no window and the batch
    would take the plain mask entry."""
    listing = json.load(open(os.path.join(GOLD, "data_golden.json")))
    arrays = np.load(os.path.join(GOLD, "data_golden.npz"))
    cfg = crop_cfg(listing)
    assert cfg.INPUT.CROP.ENABLED is False
    dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
    host, device = DatasetMapper(cfg, True), dm.DeviceMapper(cfg, True)
    assert not host.recompute_boxes and not device.recompute_boxes and len(host.augmentations.augs) == len(device.augmentations) == 2
    seen = 0
    for case in listing["cases"]:
        if case["key"].startswith("test_"):
            continue
        key, d = case["key"], dicts[case["index"]]
        np.random.seed(case["np_seed"])
        raw = device(d)
        assert "window" not in raw[dm.RAW_KEY] and "recompute_boxes" not in raw[dm.RAW_KEY]
        assert dm.describe_windows([raw]) is None
        np.random.seed(case["np_seed"])
        for out in (host(d), dm.finish_on_host(raw)):
            inst = out["instances"]
            assert np.array_equal(out["image"].numpy(), arrays[key + "_image"])
            assert np.array_equal(out["sem_seg"].numpy(), arrays[key + "_sem_seg"])
            assert np.array_equal(inst.gt_boxes.tensor.numpy(), arrays[key + "_boxes"])
            assert np.array_equal(inst.gt_classes.numpy(), arrays[key + "_classes"])
            assert sorted(inst.get_fields().keys()) == case["instance_fields"]
            if inst.has("gt_masks"):
                assert np.array_equal(np.packbits(inst.gt_masks.tensor.numpy(), axis=-1), arrays[key + "_masks"])
        seen += 1
    assert seen == 20


def test_header_declares_and_library_exports_the_entry_point():
    import ctypes

    from u2seg_amd import _hip

    decl = _hip.declared_symbols()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert decl["u2_aug_rle_masks_boxes"] == (I, [P, LL, P, P, LL, P, P, I, P, P, I, P])
    assert decl["u2_aug_rle_masks"] == (I, [P, LL, P, P, LL, P, I, P, I, P])
    lib = ctypes.CDLL(_hip.lib_path())
    fn = lib.u2_aug_rle_masks_boxes
    fn.restype, fn.argtypes = decl["u2_aug_rle_masks_boxes"]
    assert ctypes.sizeof(dm._AugWindow) == 16
    assert fn(None, 0, None, None, 0, None, None, 0, None, None, 0, None) == 0   # no image: nothing to do
    assert fn(None, 0, None, None, 0, None, None, 0, None, None, -1, None) == -1
    assert fn(None, 0, None, None, 0, None, None, 0, None, None, 1, None) == -1  # refused on the host, nothing launched


def test_crop_config_builds_both_mappers():
    """configs/.../u2seg_R50_800_crop.yaml: the 800 config with the reference's default crop; both mappers put the RandomCrop in
    front of the resize and recompute the boxes, the test-mode mapper does neither."""
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800_crop.yaml"))
    assert cfg.INPUT.CROP.ENABLED is True and cfg.INPUT.CROP.TYPE == "relative_range" and list(cfg.INPUT.CROP.SIZE) == [0.9, 0.9]
    host, device, test = DatasetMapper(cfg, True), dm.DeviceMapper(cfg, True), DatasetMapper(cfg, False)
    for augs in (host.augmentations.augs, device.augmentations):
        assert [type(a) for a in augs] == [T.RandomCrop, T.ResizeShortestEdge, T.RandomFlip]
        assert (augs[0].crop_type, list(augs[0].crop_size)) == ("relative_range", [0.9, 0.9])
    assert host.recompute_boxes and device.recompute_boxes and not test.recompute_boxes
    assert [type(a) for a in test.augmentations.augs] == [T.ResizeShortestEdge]
