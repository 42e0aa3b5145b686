"""Generates tests/golden/train_metrics_golden.npz / .json: what the reference logs for small fixed inputs.
Runs only where the reference is checked out; the output is committed and the tests read nothing else.

    python tests/golden/make_train_metrics_fixture.py

Classification cases: logits [R, K + 1] and labels [R] go to the reference's _log_classification_stats
(roi_heads/fast_rcnn.py:88-115) under its EventStorage.  The logits are multiples of 0.25 in [-2, 2] - exact in bf16, and
coarse enough that tied maxima are frequent - with planted rows: all columns equal (argmax 0), the maximum in the background
column, the maximum tied between a foreground column and the background column.  Labels mix foreground classes, background
(= K), rows labelled with their own argmax and, in one case, nothing but background.

Mask case: logits [B, K, M, M] from the same grid (exact zeros included), classes [B] and boolean targets [B, M, M] go to the
reference's mask_rcnn_loss (roi_heads/mask_head.py:33-112).  The targets reach it through an object whose crop_and_resize
returns them as they are, so no resampling takes part; one target is all ones, one all zeros.

Stored: the inputs, and every scalar the reference put, by name."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)


def grid(rs, shape):
    return (rs.randint(-8, 9, size=shape) * 0.25).astype(np.float32)


class GivenMasks:
    """Ground-truth masks that are already at the mask head's resolution."""

    def __init__(self, masks):
        self.masks = masks

    def __len__(self):
        return len(self.masks)

    def crop_and_resize(self, boxes, side):
        assert self.masks.shape[1:] == (side, side) and len(boxes) == len(self.masks)
        return self.masks


def main():
    from make_fixtures import import_reference

    import_reference()
    from detectron2.modeling.roi_heads.fast_rcnn import _log_classification_stats
    from detectron2.modeling.roi_heads.mask_head import mask_rcnn_loss
    from detectron2.structures import Boxes, Instances
    from detectron2.utils.events import EventStorage

    rs = np.random.RandomState(20)
    arrays, scalars = {}, {}

    def cls_case(name, r, k, labels, agree=()):
        z = grid(rs, (r, k + 1))
        z[0] = 0.5                      # all equal: argmax 0
        z[1], z[1, k] = -1.0, 1.75      # the background column wins
        z[2], z[2, 3], z[2, k] = -2.0, 2.0, 2.0   # tie between column 3 and the background: column 3 wins
        z[3], z[3, k - 1], z[3, 0] = 0.0, 1.0, 1.0  # tie between the first and the last foreground column
        for i in agree:                 # rows that are classified correctly (ties resolved as argmax does)
            labels[i] = int(z[i].argmax())
        with EventStorage(0) as st:
            _log_classification_stats(torch.from_numpy(z), torch.from_numpy(labels))
            scalars[name] = {n: v for n, (v, _) in st.latest().items()}
        arrays[name + "_logits"], arrays[name + "_labels"] = z, labels

    k = 12
    lab = rs.randint(0, k + 1, size=37).astype(np.int64)
    lab[:4] = [0, 5, 3, 0]
    lab[4:12] = k
    cls_case("cls_mixed", 37, k, lab, agree=range(20, 30))
    cls_case("cls_no_fg", 9, k, np.full(9, k, dtype=np.int64))
    k = 300
    lab = rs.randint(0, k + 1, size=70).astype(np.int64)
    lab[::3] = k
    cls_case("cls_wide", 70, k, lab, agree=range(40, 64))

    # mask head: 5 instances in 2 images (3 + 2), 3 classes, 4 x 4 masks
    b, kc, m = 5, 3, 4
    z = grid(rs, (b, kc, m, m))
    z[0, :, 0, :] = 0.0                 # exact zeros: "predicted 0"
    cls = np.array([0, 2, 1, 1, 0], dtype=np.int64)
    tgt = rs.randint(0, 2, size=(b, m, m)).astype(bool)
    tgt[1], tgt[3] = True, False
    insts, start = [], 0
    for n in (3, 2):
        inst = Instances((32, 32))
        inst.gt_classes = torch.from_numpy(cls[start:start + n])
        inst.proposal_boxes = Boxes(torch.tensor([[0.0, 0.0, 32.0, 32.0]] * n))
        inst.gt_masks = GivenMasks(torch.from_numpy(tgt[start:start + n]))
        insts.append(inst)
        start += n
    with EventStorage(0) as st:
        loss = mask_rcnn_loss(torch.from_numpy(z), insts)
        scalars["mask"] = {n: v for n, (v, _) in st.latest().items()}
    scalars["mask"]["loss"] = float(loss)
    arrays["mask_logits"], arrays["mask_classes"], arrays["mask_targets"] = z, cls, tgt
    arrays["mask_per_image"] = np.array([3, 2], dtype=np.int64)

    np.savez_compressed(os.path.join(HERE, "train_metrics_golden.npz"), **arrays)
    with open(os.path.join(HERE, "train_metrics_golden.json"), "w") as f:
        json.dump(scalars, f, indent=1, sort_keys=True)
    print(json.dumps(scalars, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
