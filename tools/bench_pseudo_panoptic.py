#!/usr/bin/env python
"""What the pseudo-panoptic merge costs on the host and on the device.  Synthetic ellipse instances
(compressed RLE, as the pseudo instance files hold them) over a blocky 27-class map at 480 x 640, with 7 and with 20 instances:

  per image: host merge_image; the device merge at batch 16, by HIP events around the launches and end to end (parsing the
  RLE strings, upload, launches, readback, segments_info); id2rgb + PNG encoding of the id image;
  images per second of generate() on a generated tree in a temporary directory: host, host followed by
  separate_semantic_from_panoptic, device, device with sem_seg_root.

Every timed window is warmed up first and ends in a device synchronise (merge_images_device returns after its readback).  The
device results are compared with the host's on the timed inputs before anything is timed.  Needs a GPU; prints one JSON line
per figure and writes them all to --out (default profiles/pseudo_panoptic.json)."""
import argparse
import copy
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from u2seg_amd.data import pseudo_panoptic as PP  # noqa: E402
from u2seg_amd.data import rle  # noqa: E402

H, W, CLASS_NUM = 480, 640, 800


def make_image(rs, n):
    sem = rs.randint(0, 27, (H // 32 + 1, W // 32 + 1)).repeat(32, 0).repeat(32, 1)[:H, :W].astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    instances = []
    for _ in range(n):
        bw, bh = rs.uniform(0.1, 0.5) * W, rs.uniform(0.1, 0.5) * H
        x0, y0 = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
        m = (((xx + 0.5 - x0 - bw / 2) / (bw / 2)) ** 2 + ((yy + 0.5 - y0 - bh / 2) / (bh / 2)) ** 2 <= 1).astype(np.uint8)
        instances.append({"bbox": [float(x0), float(y0), float(bw), float(bh)], "segmentation": rle.encode(m),
                          "category_id": int(rs.randint(1, CLASS_NUM + 1)), "iscrowd": 0, "area": int(m.sum())})
    return sem, instances


def make_tree(root, images, split="train"):
    """The reference's directory layout with `images` = [(semantic, instances)]."""
    ann_root = os.path.join(root, "datasets", "prepare_ours", "u2seg_annotations")
    sem_dir = os.path.join(ann_root, "semantic_annotations", "stego_coco_%s_semantic_seg_resized" % split)
    for d in (os.path.join(ann_root, "ins_annotations"), sem_dir, os.path.join(ann_root, "panoptic_annotations"),
              os.path.join(root, "datasets", "datasets", "panoptic_anns")):
        os.makedirs(d, exist_ok=True)
    template = {"images": [], "annotations": [], "info": {}, "licenses": []}
    pseudo = {"annotations": {}}
    with open(os.path.join(ann_root, "semantic_annotations", "coco_%s_img_file_names.txt" % split), "w") as f:
        for i, (sem, instances) in enumerate(images):
            name = "%012d" % (i + 1)
            f.write(name + ".jpg\n")
            np.save(os.path.join(sem_dir, "%d.npy" % i), sem)
            template["images"].append({"id": i + 1, "file_name": name + ".jpg", "height": H, "width": W})
            template["annotations"].append({"image_id": i + 1, "file_name": name + ".png", "segments_info": []})
            pseudo["annotations"][str(i + 1)] = {"segments_info": instances}
    json.dump(template, open(os.path.join(root, "datasets", "datasets", "panoptic_anns", "panoptic_%s2017.json" % split), "w"))
    json.dump(pseudo, open(os.path.join(ann_root, "ins_annotations", "coco%s_%d_ins_panoptic.json" % (split, CLASS_NUM)), "w"))
    return ann_root


def fresh(images):
    return [(sem, copy.deepcopy(instances)) for sem, instances in images]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20, help="timed device batches per instance count")
    ap.add_argument("--tree-images", type=int, default=64, help="images of the generated tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_panoptic.json"))
    a = ap.parse_args()
    if not (a.device.startswith("cuda") and torch.cuda.is_available()):
        raise SystemExit("bench_pseudo_panoptic.py measures the device merge: it needs a GPU")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    rs = np.random.RandomState(0)
    for n in (7, 20):
        images = [make_image(rs, n) for _ in range(a.batch)]
        # correctness on the timed inputs first (and the warm-up of every kernel and buffer)
        results, nxt = PP.merge_images_device(fresh(images), CLASS_NUM, 1, a.device, outputs=("rgb", "sem", "ids"))
        seg_id, host_maps = 1, []
        for (sem, instances), res in zip(fresh(images), results):
            ids, segments, seg_id = PP.merge_image(sem, instances, CLASS_NUM, seg_id)
            assert np.array_equal(res["ids"], ids) and np.array_equal(res["rgb"], PP.id2rgb(ids)) and res["segments_info"] == segments
            host_maps.append(ids)
        assert nxt == seg_id
        PP.merge_images_device(fresh(images), CLASS_NUM, 1, a.device)
        # host merge_image, and the RLE decode inside it
        work = fresh(images)
        t0 = time.perf_counter()
        for sem, instances in work:
            PP.merge_image(sem, instances, CLASS_NUM, 1)
        host_ms = (time.perf_counter() - t0) * 1e3 / len(work)
        t0 = time.perf_counter()
        for sem, instances in work:
            for ins in instances:
                rle.decode(ins["segmentation"])
        decode_ms = (time.perf_counter() - t0) * 1e3 / len(work)
        # device: events around the launches, wall clock around the whole call (ends in a synchronise)
        ev_ms, wall_ms, pack_ms = [], [], []
        for _ in range(a.repeats):
            work, events = fresh(images), []
            t0 = time.perf_counter()
            PP.merge_images_device(work, CLASS_NUM, 1, a.device, events=events)
            wall_ms.append((time.perf_counter() - t0) * 1e3 / a.batch)
            ev_ms.append(events[0].elapsed_time(events[1]) / a.batch)
            t0 = time.perf_counter()
            PP.pack_items(work)
            pack_ms.append((time.perf_counter() - t0) * 1e3 / a.batch)
        # id2rgb + PNG encode of the id image, one thread, into memory
        from PIL import Image

        t0 = time.perf_counter()
        for ids in host_maps:
            Image.fromarray(PP.id2rgb(ids)).save(io.BytesIO(), format="PNG")
        png_ms = (time.perf_counter() - t0) * 1e3 / len(host_maps)
        t0 = time.perf_counter()
        for res in results:
            Image.fromarray(res["rgb"]).save(io.BytesIO(), format="PNG")
        png_only_ms = (time.perf_counter() - t0) * 1e3 / len(results)
        emit({"metric": "merge ms per image", "shape": [H, W], "instances": n, "batch": a.batch,
              "host_merge_image": round(host_ms, 3), "host_rle_decode_of_it": round(decode_ms, 3),
              "device_events_median": round(float(np.median(ev_ms)), 4), "device_events_min_max": [round(min(ev_ms), 4), round(max(ev_ms), 4)],
              "device_end_to_end_median": round(float(np.median(wall_ms)), 3),
              "device_end_to_end_min_max": [round(min(wall_ms), 3), round(max(wall_ms), 3)],
              "of_it_host_rle_parse_and_pack_median": round(float(np.median(pack_ms)), 3),
              "host_id2rgb_png_encode": round(png_ms, 3), "png_encode_of_device_rgb": round(png_only_ms, 3),
              "repeats": a.repeats})
    # generate() on a tree: images per second, both paths, with and without the label maps
    images = [make_image(rs, 7 if i % 2 else 20) for i in range(a.tree_images)]
    with tempfile.TemporaryDirectory() as tmp:
        ann_root = make_tree(tmp, images)
        pan_json = os.path.join(ann_root, "panoptic_annotations", "cocotrain_%d.json" % CLASS_NUM)
        pan_root = os.path.join(ann_root, "panoptic_annotations", "cocotrain_%d" % CLASS_NUM)

        def host(with_sem):
            PP.generate(tmp, CLASS_NUM, "train")
            if with_sem:
                PP.separate_semantic_from_panoptic(pan_json, pan_root, os.path.join(tmp, "sem_host"), PP.create_cate(CLASS_NUM))

        def device(with_sem):
            PP.generate(tmp, CLASS_NUM, "train", device=a.device, batch_images=a.batch,
                        sem_seg_root=os.path.join(tmp, "sem_device") if with_sem else None)

        device(True)  # warm-up
        rates = {}
        for name, fn, with_sem in (("host", host, False), ("device", device, False), ("host_then_second_script", host, True),
                                   ("device_with_sem_seg_root", device, True), ("device_again", device, False),
                                   ("host_again", host, False)):
            t0 = time.perf_counter()
            fn(with_sem)
            rates[name] = round(a.tree_images / (time.perf_counter() - t0), 2)
        emit({"metric": "generate images per second", "shape": [H, W], "images": a.tree_images, "instances": "7 and 20 alternating",
              "batch": a.batch, "encode_workers": min(PP.ENCODE_WORKERS, os.cpu_count() or 1), **rates})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "results": lines}, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
