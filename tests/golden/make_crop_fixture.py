"""Generates tests/golden/crop_golden.{json,npz}: what the reference's DatasetMapper(cfg, True) returns on tests/golden/data_small
with INPUT.CROP enabled.  Runs only where the reference is checked out; the output is committed (arrays and json only) and the
tests read nothing else.

    python tests/golden/make_crop_fixture.py

The configuration is that of data_golden (u2seg_R50_800.yaml + DATA_INPUT_OPTS) plus the crop keys; the three images that
survive filter_empty, np.random.seed(1000 * index + seed) for seeds 0-4, and four settings, one per crop type:

    relative_range [0.9, 0.9]   relative [0.5, 0.4]   absolute [20, 24]   absolute_range [12, 40]

Pinned by this: RandomCrop's arithmetic and its draws from numpy's global stream (number and order: the position of the stream
behind every call is stored as the next np.random.rand()), the crop in front of the resize, the boxes recomputed from the
cropped, resized, flipped masks, and filter_empty_instances behind that (30 instances per setting; 0, 2, 2 and 1 of them are
dropped, asserted below; every stored box is integral).
Restated and therefore NOT pinned: fvcore's CropTransform, which is not installed here.  The stand-in below is its slice
(apply_image) and its subtraction (apply_coords); the reference's mapper runs over that.

Stored per case: boxes, classes, bit-packed masks, image_size, the next rand(); image and label map in full for seed 0, as
crc32 + shape for seeds 1-4 (60 cases of pixels would not fit a committed file)."""
import json
import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

SETTINGS = (("relative_range", [0.9, 0.9], 0), ("relative", [0.5, 0.4], 2), ("absolute", [20, 24], 2),
            ("absolute_range", [12, 40], 1))      # (INPUT.CROP.TYPE, INPUT.CROP.SIZE, instances dropped of 30)
SEEDS = (0, 1, 2, 3, 4)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def main():
    from make_fixtures import DATA_INPUT_OPTS, DATA_ROOT, REF, install_data_standins, install_standins

    os.environ.setdefault("CLUSTER_NUM", "800")
    work = tempfile.mkdtemp()   # the fork hard-wires the dataset root to ./datasets (builtin.py:279)
    os.symlink(DATA_ROOT, os.path.join(work, "datasets"))
    os.chdir(work)
    install_standins()
    install_data_standins()
    import fvcore.transforms.transform as FT

    class CropTransform(FT.Transform):
        def __init__(self, x0, y0, w, h, orig_w=None, orig_h=None):
            self.x0, self.y0, self.w, self.h, self.orig_w, self.orig_h = x0, y0, w, h, orig_w, orig_h

        def apply_image(self, img):
            return img[self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]

        def apply_coords(self, coords):
            coords[:, 0] -= self.x0
            coords[:, 1] -= self.y0
            return coords

    FT.CropTransform = CropTransform
    sys.path.insert(0, REF)
    sys.modules["detectron2._C"] = types.ModuleType("detectron2._C")  # the data path touches no compiled op
    from detectron2.config import get_cfg
    from detectron2.data import DatasetMapper
    from detectron2.data.build import get_detection_dataset_dicts

    arrays, listing = {}, {"input_opts": [list(x) if isinstance(x, tuple) else x for x in DATA_INPUT_OPTS], "settings": []}
    for si, (crop_type, crop_size, want_dropped) in enumerate(SETTINGS):
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(REF, "configs/COCO-PanopticSegmentation/u2seg_R50_800.yaml"))
        cfg.merge_from_list(list(DATA_INPUT_OPTS) + ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", crop_type, "INPUT.CROP.SIZE",
                                                     crop_size])
        # filter_empty: the crowd-only image goes - the reference's mapper raises AttributeError on it with recompute_boxes
        dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=True)
        assert len(dicts) == 3, len(dicts)
        mapper = DatasetMapper(cfg, True)
        assert mapper.recompute_boxes and type(mapper.augmentations.augs[0]).__name__ == "RandomCrop"
        cases, total, kept = [], 0, 0
        for idx in range(len(dicts)):
            for seed in SEEDS:
                np.random.seed(1000 * idx + seed)
                out = mapper(dicts[idx])
                after = float(np.random.rand())
                key = "s%d_%d_%d" % (si, idx, seed)
                inst = out["instances"]
                image, sem = out["image"].numpy(), out["sem_seg"].numpy().astype(np.uint8)
                assert out["sem_seg"].numpy().max() <= 255 and out["sem_seg"].numpy().min() >= 0
                boxes = inst.gt_boxes.tensor.numpy()
                assert boxes.dtype == np.float32 and np.array_equal(boxes, np.round(boxes))   # tight boxes are pixel counts
                if seed == 0:
                    arrays[key + "_image"], arrays[key + "_sem_seg"] = image, sem
                arrays[key + "_boxes"] = boxes
                arrays[key + "_classes"] = inst.gt_classes.numpy()
                arrays[key + "_masks"] = np.packbits(inst.gt_masks.tensor.numpy(), axis=-1)
                total += sum(1 for a in dicts[idx]["annotations"] if a.get("iscrowd", 0) == 0)
                kept += len(inst)
                cases.append({"key": key, "index": idx, "np_seed": 1000 * idx + seed, "image_size": list(inst.image_size),
                              "pixels": seed == 0, "image_shape": list(image.shape), "image_crc32": crc(image),
                              "sem_seg_shape": list(sem.shape), "sem_seg_crc32": crc(sem), "num_instances": len(inst),
                              "next_rand": after, "keys": sorted(out.keys()),
                              "instance_fields": sorted(inst.get_fields().keys())})
        assert (total, total - kept) == (30, want_dropped), (crop_type, total, total - kept)
        listing["settings"].append({"type": crop_type, "size": crop_size, "instances": total, "dropped": total - kept,
                                    "cases": cases})
        print(crop_type, crop_size, "dropped", total - kept, "of", total)
    json.dump(listing, open(os.path.join(HERE, "crop_golden.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "crop_golden.npz"), **arrays)
    print("wrote crop_golden: %d arrays, %d bytes" % (len(arrays), os.path.getsize(os.path.join(HERE, "crop_golden.npz"))))


if __name__ == "__main__":
    main()
