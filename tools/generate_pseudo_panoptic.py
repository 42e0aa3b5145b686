#!/usr/bin/env python
"""Command line of the reference's datasets/prepare_ours/generate_pseudo_panoptic.py (--class_num, --split), run from the
directory that holds ./datasets like the reference.  --device-merge merges on the GPU (csrc/labelprep.hip, DESIGN.md 18:
same pngs and json), --batch images at a time; with --sem-seg-root it also writes the label maps that
prepare_stuff_panoptic_fpn.py would derive from the pngs."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.data.pseudo_panoptic import generate  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-class_num", "--class_num", type=int, default=800)
    ap.add_argument("-split", "--split", type=str, default="train")
    ap.add_argument("--device-merge", action="store_true", help="merge on the GPU (HIP kernels, no host fallback)")
    ap.add_argument("--batch", type=int, default=16, metavar="N", help="images per device batch (with --device-merge)")
    ap.add_argument("--sem-seg-root", default=None, metavar="DIR", help="also write the semantic label maps here "
                    "(needs --device-merge)")
    a = ap.parse_args()
    if a.sem_seg_root is not None and not a.device_merge:
        raise SystemExit("--sem-seg-root needs --device-merge: on the host the label maps come from the second script")
    out = generate(os.getcwd(), a.class_num, a.split, device="cuda" if a.device_merge else None, batch_images=a.batch,
                   sem_seg_root=a.sem_seg_root)
    print("wrote %d images, %d annotations" % (len(out["images"]), len(out["annotations"])))
