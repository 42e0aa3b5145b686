"""Inputs shared by test_semseg_boundary_host.py and test_gpu_semseg_boundary.py: the literal numpy restatement of the
reference's _mask_to_boundary (detectron2/evaluation/sem_seg_evaluation.py:396-407), label maps, shapes, and the tiny
validation set of tests/golden/eval_golden laid out for the semantic evaluator."""
import json
import os

import numpy as np
import torch
from PIL import Image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 17  # 16 classes + the ignore label

# (h, w, d): 1 x 1; windows of 3; a window larger than the image (7 x 9, d = 4: the boundary is the map itself); a map of
# several tiles with a small and a large halo; d larger than both sides; a common d on an odd size
SHAPES = ((1, 1, 1), (3, 5, 1), (5, 5, 1), (7, 9, 4), (70, 131, 7), (70, 131, 31), (40, 33, 40), (129, 257, 16))


def literal_boundary(m, d):
    """m uint8 [h, w]: a one-pixel ring of zeros, d passes of a 3 x 3 minimum (cv2.erode's default border is +inf for an
    erosion: it never lowers a value, written here as a border of 255), the ring dropped, the subtraction in uint8."""
    assert m.dtype == np.uint8 and m.ndim == 2
    p = np.pad(m, 1, constant_values=0)
    hh, ww = p.shape
    for _ in range(d):
        q = np.pad(p, 1, constant_values=255)
        p = np.min(np.stack([q[i : i + hh, j : j + ww] for i in range(3) for j in range(3)]), axis=0)
    return m - p[1:-1, 1:-1]


def literal_confusion(pred, gt, lut, d, n=N):
    """(conf, bconf) int64 [n, n] as the reference's process() accumulates them for one image; lut applied first."""
    if lut is not None:
        pred = np.asarray(lut, dtype=np.uint8)[pred]
    conf = np.bincount(n * pred.reshape(-1).astype(np.int64) + gt.reshape(-1), minlength=n * n).reshape(n, n)
    bp, bg = literal_boundary(pred, d), literal_boundary(gt, d)
    bconf = np.bincount(n * bp.reshape(-1).astype(np.int64) + bg.reshape(-1), minlength=n * n).reshape(n, n)
    return conf, bconf


def blobs(rs, h, w, side=8):
    """8 x 8 blocks of labels 0 .. 16."""
    small = rs.randint(0, N, size=((h + side - 1) // side, (w + side - 1) // side))
    return np.repeat(np.repeat(small, side, axis=0), side, axis=1)[:h, :w].astype(np.uint8)


def label_maps(h, w, seed):
    """name -> (pred, gt): blobs, a constant map, a checkerboard, a single non-zero pixel (each against blobs of its own)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    single = np.zeros((h, w), dtype=np.uint8)
    single[h // 2, w // 2] = 9
    return {"blobs": (blobs(rs, h, w), blobs(rs, h, w)),
            "constant": (np.full((h, w), 5, dtype=np.uint8), blobs(rs, h, w)),
            "checkerboard": (((yy + xx) % 2 * 7 + 3).astype(np.uint8), blobs(rs, h, w, side=3)),
            "single": (blobs(rs, h, w), single)}


def chained_lut():
    """A table as the evaluator composes it: clusters 1 .. 27 onto supercategories, some onto the ignore label 16, 0 kept;
    its values on 0 .. 27 are all < N."""
    lut = np.arange(256, dtype=np.uint8)
    lut[1:28] = [3, 16, 7, 7, 1, 16, 12, 15, 2, 4, 16, 9, 9, 10, 5, 6, 16, 8, 11, 13, 14, 1, 16, 2, 3, 15, 6]
    lut[28:] = 0
    return lut


def tiny_val_sem(tmp_path):
    """The tiny validation set of tests/golden/eval_golden (made by the reference's own evaluators) laid out under tmp_path and
    registered as "tiny_val_sem", with the reference's semantic mapping file in ./hungarian_matching of tmp_path: (fixture,
    inputs, outputs with CPU logits, ground-truth arrays).  The caller changes into tmp_path."""
    from u2seg_amd.data import DatasetCatalog, MetadataCatalog
    from u2seg_amd.data.datasets import load_sem_seg

    fx = json.load(open(os.path.join(GOLD, "eval_golden.json")))
    arrays = np.load(os.path.join(GOLD, "eval_golden.npz"))
    img_dir, gt_dir = tmp_path / "images", tmp_path / "sem_gt"
    os.makedirs(img_dir)
    os.makedirs(gt_dir)
    os.makedirs(tmp_path / "hungarian_matching")
    for im in fx["images"]:
        stem = im["file_name"][:-4]
        Image.fromarray(np.zeros((im["height"], im["width"], 3), dtype=np.uint8)).save(img_dir / im["file_name"])
        Image.fromarray(arrays["gt_" + stem], mode="L").save(gt_dir / (stem + ".png"))
    if "tiny_val_sem" in DatasetCatalog:
        DatasetCatalog.remove("tiny_val_sem")
    if "tiny_val_sem" in MetadataCatalog:
        MetadataCatalog.remove("tiny_val_sem")
    DatasetCatalog.register("tiny_val_sem", lambda: load_sem_seg(str(gt_dir), str(img_dir)))
    MetadataCatalog.get("tiny_val_sem").set(stuff_classes=[str(c) for c in range(28)], ignore_label=255)
    json.dump(fx["semantic_mapping_file"], open(tmp_path / "hungarian_matching" / "semantic_mapping.json", "w"))
    inputs = [{"image_id": im["id"], "file_name": str(img_dir / im["file_name"]), "height": im["height"], "width": im["width"]}
              for im in fx["images"]]
    outputs = [{"sem_seg": torch.from_numpy(arrays["logits_" + im["file_name"][:-4]])} for im in fx["images"]]
    gts = [arrays["gt_" + im["file_name"][:-4]] for im in fx["images"]]
    return fx, inputs, outputs, gts
