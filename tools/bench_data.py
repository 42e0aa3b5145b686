#!/usr/bin/env python
"""Input-pipeline throughput: DatasetMapper (JPEG decode, ResizeShortestEdge over the config's 10 short-edge choices, flip,
RLE -> bitmasks) in DataLoader workers, optionally through DevicePrefetcher into HBM.  Builds a throw-away COCO-shaped
dataset (480x640 / 640x480 JPEGs, 7 RLE instances per image, semantic label maps) under a temp dir, so it runs anywhere.
Prints one JSON line per worker count; the training step consumes ~197 img/s per GPU.

--device-mapper: every worker count runs twice in the same process, the host mapper first and then the DeviceMapper whose raw
records DevicePrefetcher finishes on the GPU; also prints the mapper time per image in one process for
both mappers, the bytes per batch that cross the shared-memory slot, and the HIP-event time of the three augmentation calls on
a full per-GPU batch, and of the two mask entries (u2_aug_rle_masks, u2_aug_rle_masks_boxes with the whole image as its window)
on one identical batch of 16 uncropped records.  --crop TYPE H W: the same runs with INPUT.CROP enabled,
so that the host-mapper and device-mapper img/s stand side by side for every worker count.
--out FILE collects every line into one JSON file."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_dataset(root, n_images, seed=0):
    from PIL import Image

    from u2seg_amd.data import rle

    rs = np.random.RandomState(seed)
    img_dir = os.path.join(root, "coco", "train2017")
    ann_dir = os.path.join(root, "prepare_ours", "u2seg_annotations", "ins_annotations")
    sem_dir = os.path.join(root, "prepare_ours", "u2seg_annotations", "panoptic_annotations", "panoptic_stuff_cocotrain_800")
    for d in (img_dir, ann_dir, sem_dir):
        os.makedirs(d, exist_ok=True)
    images, annotations, aid = [], [], 1
    for i in range(n_images):
        h, w = (480, 640) if i % 4 else (640, 480)
        name = "%012d" % (i + 1)
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.clip(np.stack([xx * 255.0 / w, yy * 255.0 / h, (xx + yy) * 255.0 / (h + w)], 2) + rs.randn(h, w, 3) * 20, 0, 255)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(img_dir, name + ".jpg"), quality=90)
        sem = rs.randint(0, 28, (h // 32 + 1, w // 32 + 1)).repeat(32, 0).repeat(32, 1)[:h, :w].astype(np.uint8)
        Image.fromarray(sem, mode="L").save(os.path.join(sem_dir, name + ".png"))
        images.append({"id": i + 1, "file_name": name + ".jpg", "height": h, "width": w})
        for _ in range(7):
            bw, bh = rs.uniform(0.1, 0.5) * w, rs.uniform(0.1, 0.5) * h
            x0, y0 = rs.uniform(0, w - bw), rs.uniform(0, h - bh)
            m = (((xx + 0.5 - x0 - bw / 2) / (bw / 2)) ** 2 + ((yy + 0.5 - y0 - bh / 2) / (bh / 2)) ** 2 <= 1).astype(np.uint8)
            annotations.append({"id": aid, "image_id": i + 1, "category_id": int(rs.randint(1, 801)), "iscrowd": 0,
                                "bbox": [float(x0), float(y0), float(bw), float(bh)], "area": float(m.sum()),
                                "segmentation": rle.encode(m)})
            aid += 1
    cats = [{"id": c + 1, "name": str(c + 1), "supercategory": str(c + 1)} for c in range(800)]
    json.dump({"images": images, "annotations": annotations, "categories": cats},
              open(os.path.join(ann_dir, "cocotrain_800.json"), "w"))


def mapper_ms_per_image(cfg, device_mapper, dicts, repeats=2):
    """Mapper time per image in this process (no loader, no transport)."""
    from u2seg_amd.data import DatasetMapper
    from u2seg_amd.data.device_mapper import DeviceMapper

    mapper = DeviceMapper(cfg, True) if device_mapper else DatasetMapper(cfg, True)
    np.random.seed(0)
    for d in dicts[:4]:
        mapper(d)
    t0 = time.perf_counter()
    for _ in range(repeats):
        for d in dicts:
            mapper(d)
    return 1e3 * (time.perf_counter() - t0) / (repeats * len(dicts))


def kernel_times(cfg, dicts, device, batch_size, repeats=20):
    """HIP-event time of the three calls of csrc/augment.hip on one per-GPU batch of raw records (ms per batch, median)."""
    from u2seg_amd import _hip
    from u2seg_amd.data import device_mapper as dm
    from u2seg_amd.data.slots import layout_batch, unpack, write_batch

    np.random.seed(0)
    mapper = dm.DeviceMapper(cfg, True)
    records = [mapper(dicts[i % len(dicts)]) for i in range(batch_size)]
    staged, nbytes, samples = layout_batch(records)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    write_batch(host.numpy(), staged)
    block = host.to(device)
    dev = unpack(block, samples)
    descs, img_bytes, lab_elems, mask_bytes, masks = dm.describe_batch(dev, block.data_ptr())
    n = len(dev)
    image = torch.empty(img_bytes, dtype=torch.uint8, device=device)
    labels = torch.empty(max(lab_elems, 1), dtype=torch.int64, device=device)
    mask_out = torch.empty(max(mask_bytes, 1), dtype=torch.bool, device=device)
    counts = torch.empty(max(masks, 1), dtype=torch.int32, device=device)
    need = int(_hip.call_nostream("u2_aug_resize_bilinear_scratch_bytes", descs, n))
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    windows = dm.describe_windows(dev)  # None without a crop: the batch takes the plain mask entry, like launch_batch
    boxes = torch.empty((max(masks, 1), 4), dtype=torch.int32, device=device)
    calls = [("bilinear", lambda: _hip.call("u2_aug_resize_bilinear_u8", block, nbytes, host.data_ptr(), image, img_bytes, scratch,
                                             need, descs, n)),
             ("nearest", lambda: _hip.call("u2_aug_resize_nearest_u8", block, nbytes, host.data_ptr(), labels, lab_elems, descs, n)),
             ("rle_masks", lambda: _hip.call("u2_aug_rle_masks", block, nbytes, host.data_ptr(), mask_out, mask_bytes, counts,
                                              masks, descs, n)) if windows is None else
             ("rle_masks_boxes", lambda: _hip.call("u2_aug_rle_masks_boxes", block, nbytes, host.data_ptr(), mask_out, mask_bytes,
                                                    counts, boxes, masks, descs, windows, n))]
    times = {name: [] for name, _ in calls}
    for it in range(repeats + 3):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:
                times[name].append(e0.elapsed_time(e1))
    out = {name: round(float(np.median(v)), 4) for name, v in times.items()}
    out["total"] = round(sum(out.values()), 4)
    out.update({"images": n, "masks": masks, "bytes_in": nbytes, "bytes_out": img_bytes + 8 * lab_elems + mask_bytes})
    return out


def mask_entry_times(cfg, dicts, device, batch_size=16, repeats=20, warmup=5):
    """HIP-event time of u2_aug_rle_masks and of u2_aug_rle_masks_boxes (window = the whole image) on one identical batch of
    uncropped raw records at the training size, alternating in one process (ms per call, median of `repeats` after `warmup`)."""
    from u2seg_amd import _hip
    from u2seg_amd.data import device_mapper as dm
    from u2seg_amd.data.slots import layout_batch, unpack, write_batch

    cfg = cfg.clone()
    cfg.merge_from_list(["INPUT.CROP.ENABLED", False])
    np.random.seed(0)
    mapper = dm.DeviceMapper(cfg, True)
    records = [mapper(dicts[i % len(dicts)]) for i in range(batch_size)]
    staged, nbytes, samples = layout_batch(records)
    host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    write_batch(host.numpy(), staged)
    block = host.to(device)
    dev = unpack(block, samples)
    descs, _, _, mask_bytes, masks = dm.describe_batch(dev, block.data_ptr())
    windows = (dm._AugWindow * len(dev))()
    for win, d in zip(windows, dev):
        win.x0, win.y0, win.mask_h, win.mask_w = 0, 0, d[dm.RAW_KEY]["h"], d[dm.RAW_KEY]["w"]
    outs = [torch.zeros(max(mask_bytes, 1), dtype=torch.bool, device=device) for _ in range(2)]  # (the alignment gaps are never written)
    counts = [torch.empty(max(masks, 1), dtype=torch.int32, device=device) for _ in range(2)]
    boxes = torch.empty((max(masks, 1), 4), dtype=torch.int32, device=device)
    calls = [("rle_masks", lambda: _hip.call("u2_aug_rle_masks", block, nbytes, host.data_ptr(), outs[0], mask_bytes, counts[0],
                                              masks, descs, len(dev))),
             ("rle_masks_boxes", lambda: _hip.call("u2_aug_rle_masks_boxes", block, nbytes, host.data_ptr(), outs[1], mask_bytes,
                                                    counts[1], boxes, masks, descs, windows, len(dev)))]
    times = {name: [] for name, _ in calls}
    for it in range(repeats + warmup):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    assert torch.equal(outs[0], outs[1]) and torch.equal(counts[0], counts[1])
    out = {name: round(float(np.median(v)), 4) for name, v in times.items()}
    out.update({name + "_min_max": [round(float(min(v)), 4), round(float(max(v)), 4)] for name, v in times.items()})
    out.update({"images": len(dev), "masks": masks, "mask_bytes": mask_bytes})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--workers", type=int, nargs="+", default=[0, 8, 32])
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--device-mapper", action="store_true", help="run every worker count with the host mapper and with the "
                    "DeviceMapper (needs a GPU: there is no host fallback)")
    ap.add_argument("--crop", nargs=3, metavar=("TYPE", "H", "W"), default=None, help="enable INPUT.CROP with this TYPE and SIZE "
                    "(relative_range 0.9 0.9, absolute 512 512, ...)")
    ap.add_argument("--out", default=None, help="also write every result line into this JSON file")
    a = ap.parse_args()
    if a.device_mapper and not a.device.startswith("cuda"):
        raise SystemExit("--device-mapper needs a GPU: raw records are finished by HIP kernels")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    os.environ["CLUSTER_NUM"] = "800"
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import DevicePrefetcher, build_detection_train_loader, register_all_coco

    root = tempfile.mkdtemp(prefix="u2seg_bench_data_")
    t0 = time.time()
    make_dataset(root, a.images)
    register_all_coco(root)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml"))
    if a.crop:
        size = [float(v) if a.crop[0].startswith("relative") else int(v) for v in a.crop[1:]]
        cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", a.crop[0], "INPUT.CROP.SIZE", size])
    emit({"crop": [a.crop[0]] + size if a.crop else None})
    emit({"dataset": "%d synthetic JPEGs 480x640 / 640x480, 7 RLE instances each" % a.images,
          "build_s": round(time.time() - t0, 1), "short_edges": list(cfg.INPUT.MIN_SIZE_TRAIN)})
    if a.device_mapper:
        from u2seg_amd.data import get_detection_dataset_dicts

        dicts = get_detection_dataset_dicts(cfg.DATASETS.TRAIN, filter_empty=cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS)
        for dm_on in (False, True, False, True):  # alternating: the spread between equal runs is part of the result
            emit({"metric": "mapper ms per image, one process", "device_mapper": dm_on,
                  "ms_per_image": round(mapper_ms_per_image(cfg, dm_on, dicts), 2)})
        emit(dict({"metric": "augmentation kernels, HIP-event ms per batch"},
                  **kernel_times(cfg, dicts, a.device, cfg.SOLVER.IMS_PER_BATCH)))
        emit(dict({"metric": "mask entries on one identical uncropped batch, window = whole image, HIP-event ms per call"},
                  **mask_entry_times(cfg, dicts, a.device)))
    for nw, dm_on in [(nw, dm_on) for nw in a.workers for dm_on in ((False, True) if a.device_mapper else (False,))]:
        cfg.defrost()
        cfg.merge_from_list(["DATALOADER.NUM_WORKERS", nw])
        loader = build_detection_train_loader(cfg, seed=1, device_mapper=dm_on)
        pre = DevicePrefetcher(loader, a.device) if a.device.startswith("cuda") else None
        stream = iter(pre if pre is not None else loader)
        for _ in range(a.warmup):  # worker start-up, pinned staging blocks, and the batches the workers prefetched
            next(stream)
        if pre is not None:
            pre.seconds_waiting_for_loader = pre.seconds_staging = pre.seconds_waiting_for_counts = 0.0
            pre.slot_bytes_moved = 0
        t0, n, px = time.time(), 0, 0
        for _ in range(a.batches):
            batch = next(stream)
            n += len(batch)
            px += sum(d["image"].shape[1] * d["image"].shape[2] for d in batch)
        if a.device.startswith("cuda"):
            torch.cuda.synchronize()
        dt = time.time() - t0
        emit({"metric": "input pipeline img/s", "workers": nw, "device_mapper": dm_on, "batch": len(batch),
              "img_per_s": round(n / dt, 1), "mean_megapixels": round(px / n / 1e6, 2), "to_device": a.device,
              "host_s_waiting_for_loader": round(pre.seconds_waiting_for_loader, 2) if pre else None,
              "host_s_staging": round(pre.seconds_staging, 2) if pre else None,
              "host_s_waiting_for_counts": round(pre.seconds_waiting_for_counts, 4) if pre else None,
              "slot_bytes_per_batch": int(pre.slot_bytes_moved / a.batches) if pre else None, "wall_s": round(dt, 2),
              "host_threads": torch.get_num_threads()})
        del stream, loader, pre
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_data.py", "args": {k: v for k, v in vars(a).items() if k != "out"}, "results": lines},
                      f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
