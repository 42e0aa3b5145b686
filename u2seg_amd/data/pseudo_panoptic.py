"""Pseudo panoptic labels = class-aware pseudo instance masks painted over an unsupervised semantic map
(datasets/prepare_ours/generate_pseudo_panoptic.py:43-173; the reference is a script, this is the same procedure as
functions plus `tools/generate_pseudo_panoptic.py` with its command line and directory layout).

Per image: instances are painted in order of decreasing box area, each with the next free segment id (ids run on across
images); instances that end up completely covered are dropped; every semantic class 1..27 claims the pixels no instance
took unless more than 70 % of the class already lies under instances; the id map is written as an RGB png
(id = R + 256 G + 256^2 B, panopticapi.utils.id2rgb)."""
import ctypes
import json
import os

import numpy as np
from PIL import Image

from . import rle

NUM_STUFF = 27
COVERED_FRACTION = 0.7


def create_cate(num):
    """Category table of the merged annotation: ids 1..num are things, the following 27 are stuff (:13-25)."""
    return [{"supercategory": str(i + 1), "id": i + 1, "name": str(i + 1), "isthing": 1 if i + 1 <= num else 0}
            for i in range(num + NUM_STUFF)]


def id2rgb(id_map):
    out = np.zeros(id_map.shape + (3,), dtype=np.uint8)
    rest = id_map.astype(np.uint32).copy()
    for c in range(3):
        out[..., c] = rest % 256
        rest //= 256
    return out


def rgb2id(color):
    c = np.asarray(color, dtype=np.uint32)
    return c[..., 0] + 256 * c[..., 1] + 256 * 256 * c[..., 2]


def merge_image(semantic, instances, class_num, first_id):
    """semantic: int array [h, w] with labels 0..26 (the unsupervised segmenter's output); instances: the image's pseudo
    instance records ({"bbox": [x, y, w, h], "segmentation": RLE, "category_id", ...}; they receive an "id").
    Returns (id map uint32 [h, w], segments_info, next free id)."""
    sem = np.asarray(semantic) + 1
    combined = np.zeros(sem.shape, dtype=np.uint32)
    masks = [rle.decode(ins["segmentation"]) for ins in instances]
    order = paint_order(instances)
    seg_id, painted = first_id, []
    for k in order:
        combined[masks[k] == 1] = seg_id
        instances[k]["id"] = seg_id
        painted.append(instances[k])
        seg_id += 1
    present = set(np.unique(combined).tolist())
    segments = [ins for ins in painted if ins["id"] in present]  # later, smaller instances may have covered one entirely
    for cat in range(1, NUM_STUFF + 1):
        is_cat = sem == cat
        free = is_cat & (combined == 0)
        if not free.any():
            continue
        if np.sum(is_cat & (combined != 0)) / np.sum(is_cat) > COVERED_FRACTION:
            continue
        combined[free] = seg_id
        segments.append({"category_id": cat + class_num, "id": seg_id, "iscrowd": 0, "bbox": [], "area": 0})
        seg_id += 1
    return combined, segments, seg_id


# ------------------------------------------------------------------------------------------------
# the same merge on the device (csrc/labelprep.hip): opt-in, merge_image stays the definition
# ------------------------------------------------------------------------------------------------
MAX_INSTANCES = 65535  # rank + 1 is kept in 16 bits while a band is painted


def coverage_skips(covered, total):
    """The device's integer form of `covered / total > COVERED_FRACTION` (total > 0): the closest a ratio other than 7/10
    comes to 0.7 is 1 / (10 total), far above a double's spacing there, and at 7/10 both say "not greater"."""
    return 10 * covered > 7 * total


def paint_order(instances):
    """Indices of the instances in the order merge_image paints them: stable, by decreasing box area in Python floats."""
    return sorted(range(len(instances)), key=lambda k: instances[k]["bbox"][-2] * instances[k]["bbox"][-1], reverse=True)


def pack_items(items):
    """Host side of the device merge, checked before anything is launched.  items: [(semantic [h, w], instances)].  Returns a
    dict: "sizes" [(h, w)], "orders" (paint order per image), "sems" (uint8 [h, w] per image, labels outside 0..26 as they are
    or 255), "counts" (int32, the uncompressed RLE counts of all instances of images with pixels, in paint order),
    "offsets" (int64 [M + 1], the first count of each of these M instances), "num" (instances per image).
    ValueError: h w >= 2^31, more than MAX_INSTANCES instances, a mask of another size than the semantic map, counts that
    are negative or do not sum to h w (rle.decode's condition)."""
    sizes, orders, sems, lists, num = [], [], [], [], []
    for i, (semantic, instances) in enumerate(items):
        sem = np.asarray(semantic)
        if sem.ndim != 2 or sem.dtype.kind not in "iub":
            raise ValueError("image %d: the semantic map must be a 2-d integer array, got %s %s" % (i, sem.dtype, sem.shape))
        h, w = int(sem.shape[0]), int(sem.shape[1])
        if h * w >= 2 ** 31:
            raise ValueError("image %d: %d x %d pixels, the device merge takes fewer than 2^31" % (i, h, w))
        if len(instances) > MAX_INSTANCES:
            raise ValueError("image %d: %d instances, the device merge takes %d" % (i, len(instances), MAX_INSTANCES))
        order = paint_order(instances)
        for k in order:
            seg = instances[k]["segmentation"]
            if [int(v) for v in seg["size"]] != [h, w]:
                raise ValueError("image %d: instance %d has a mask of size %s, the semantic map is %s"
                                 % (i, k, list(seg["size"]), [h, w]))
            counts = rle.counts_of(seg)
            if sum(counts) != h * w or any(c < 0 for c in counts):
                raise ValueError("image %d, instance %d: RLE counts sum to %d, mask has %d pixels" % (i, k, sum(counts), h * w))
            if h * w > 0:
                lists.append(counts)
        if sem.dtype != np.uint8:
            sem = np.where((sem >= 0) & (sem < NUM_STUFF), sem, 255).astype(np.uint8)
        sizes.append((h, w))
        orders.append(order)
        sems.append(np.ascontiguousarray(sem))
        num.append(len(instances))
    offsets = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in lists], out=offsets[1:])
    counts = np.fromiter((c for lst in lists for c in lst), dtype=np.int32, count=int(offsets[-1]))
    return {"sizes": sizes, "orders": orders, "sems": sems, "counts": counts, "offsets": offsets, "num": num}


class _LabelImage(ctypes.Structure):
    """Mirror of U2LabelImage (include/u2seg_hip.h)."""

    _fields_ = [("first", ctypes.c_int), ("n", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("plane_offset", ctypes.c_longlong), ("pix_offset", ctypes.c_longlong)]


_pinned = {}


def _pinned_bytes(key, nbytes):
    """A page-locked host buffer of at least nbytes, kept and grown per use (locking pages costs more than a batch)."""
    import torch

    buf = _pinned.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _pinned[key] = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8).pin_memory()
    return buf


def _align(n, a=16):
    return (n + a - 1) // a * a


def _device_merge(packed, first_id, device, outputs, events=None):
    """Upload, the launches and the single readback of one batch.  Returns (host uint8 block, offsets into it): "rgb",
    "sem", "ids" (bytes of pixel 0 of image 0; an image's pixels start pix[i] pixels on), "dec", "present", and "pix"."""
    import torch

    from .. import _hip
    from ..evaluation.mask_ops import _MaskImage, words_per_column

    sizes, num = packed["sizes"], packed["num"]
    nimg = len(sizes)
    mdescs, ldescs = (_MaskImage * nimg)(), (_LabelImage * nimg)()
    first = mfirst = words = pixels = 0
    pix = []
    for i, ((h, w), n) in enumerate(zip(sizes, num)):
        m, l = mdescs[i], ldescs[i]
        l.first, l.n, l.H, l.W, l.plane_offset, l.pix_offset = first, n, h, w, words, pixels
        nm = n if h * w > 0 else 0
        m.first, m.n, m.H, m.W, m.in_offset, m.plane_offset, m.col_offset = mfirst, nm, h, w, 0, words, 0
        pix.append(pixels)
        first += n
        mfirst += nm
        words += nm * w * words_per_column(h)
        pixels += _align(h * w)
    # one upload: label bytes | offsets (int64) | counts (int32) | instances per image (int32)
    counts, offsets = packed["counts"], packed["offsets"]
    o_offs = _align(pixels)
    o_counts = o_offs + _align(offsets.nbytes)
    o_num = o_counts + _align(counts.nbytes)
    in_bytes = o_num + _align(4 * nimg)
    stage = _pinned_bytes(("in", str(device)), in_bytes)
    host = stage.numpy()
    for p, (h, w), sem in zip(pix, sizes, packed["sems"]):
        host[p:p + h * w] = sem.reshape(-1)
    host[o_offs:o_offs + offsets.nbytes].view(np.int64)[:] = offsets
    host[o_counts:o_counts + counts.nbytes].view(np.int32)[:] = counts
    host[o_num:o_num + 4 * nimg].view(np.int32)[:] = num
    with torch.cuda.device(device):
        block = torch.empty(in_bytes, dtype=torch.uint8, device=device)
        block.copy_(stage[:in_bytes], non_blocking=True)
        sem_d = block[:max(pixels, 1)]
        offs_d = block[o_offs:o_offs + offsets.nbytes].view(torch.int64)
        counts_d = block[o_counts:o_counts + counts.nbytes].view(torch.int32)
        num_d = block[o_num:o_num + 4 * nimg].view(torch.int32)
        # one readback: id image | label map | id map | decisions | present
        o = {"pix": pix}
        cursor = 0
        for name, per_pixel in (("rgb", 3), ("sem", 1), ("ids", 4)):
            if name in outputs:
                o[name] = cursor
                cursor += _align(per_pixel * pixels)
        o["dec"] = cursor
        o["present"] = cursor = cursor + 4 * 32 * nimg
        cursor += _align(4 * first) + 16  # never empty: an empty tensor has no address to hand to the launcher
        out = torch.empty(cursor, dtype=torch.uint8, device=device)
        planes = torch.empty(max(words, 1), dtype=torch.int64, device=device)
        rank = torch.empty(max(pixels, 4), dtype=torch.int32, device=device)
        hist = torch.empty(64 * nimg, dtype=torch.int32, device=device)
        present = out[o["present"]:].view(torch.int32)
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
        if mfirst:
            cum = torch.cumsum(counts_d, 0, dtype=torch.int64)
            _hip.call("u2_mask_planes_from_counts", cum, offs_d, planes, mdescs, nimg)
        _hip.call("u2_label_paint", planes, sem_d, rank, present, hist, ldescs, nimg)
        _hip.call("u2_label_decide", hist, num_d, out[o["dec"]:], int(first_id), nimg)
        _hip.call("u2_label_emit", rank, sem_d, out[o["dec"]:], out[o["rgb"]:] if "rgb" in o else None,
                  out[o["sem"]:] if "sem" in o else None, out[o["ids"]:] if "ids" in o else None, ldescs, nimg)
        if events is not None:
            events.append(torch.cuda.Event(enable_timing=True))
            events[-1].record()
        back = _pinned_bytes(("out", str(device)), out.numel())
        back[:out.numel()].copy_(out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return back.numpy()[:out.numel()], o


def merge_images_device(items, class_num, first_id, device, outputs=("rgb", "sem"), events=None):
    """merge_image for a batch of images, called image after image, on the device: items = [(semantic, instances)].  Returns
    ([{"segments_info", and per name in `outputs`: "rgb" uint8 [h, w, 3] = id2rgb of the id map, "sem" uint8 [h, w] = the
    label map separate_semantic_from_panoptic derives (0 under an instance, c for a claimed class c, 255 elsewhere),
    "ids" uint32 [h, w] = the id map}], next free id).  The instance records receive their "id" as in merge_image.
    There is no host fallback: without a GPU this raises.  events: a list that receives two recorded torch events, before
    and after the launches (for tools/bench_pseudo_panoptic.py)."""
    import torch

    outputs = tuple(outputs)
    if not set(outputs) <= {"rgb", "sem", "ids"}:
        raise ValueError("outputs %r: choose from 'rgb', 'sem', 'ids'" % (outputs,))
    if not (str(device).startswith("cuda") and torch.cuda.is_available()):
        raise RuntimeError("the device merge runs HIP kernels: it needs a GPU (device is %r); there is no host fallback, "
                           "use merge_image" % (device,))
    packed = pack_items(items)
    first_id = int(first_id)
    if first_id < 0 or first_id + sum(n + NUM_STUFF for n in packed["num"]) > 2 ** 32:
        raise ValueError("segment ids from %d on would not fit 32 bits" % first_id)
    if not items:
        return [], first_id
    host, o = _device_merge(packed, first_id, torch.device(device), outputs, events)
    nimg = len(items)
    dec = host[o["dec"]:o["dec"] + 128 * nimg].view(np.uint32).reshape(nimg, 32)
    present = host[o["present"]:o["present"] + 4 * sum(packed["num"])].view(np.int32)
    results, at = [], 0
    for i, ((_, instances), (h, w), order) in enumerate(zip(items, packed["sizes"], packed["orders"])):
        base = int(dec[i, NUM_STUFF + 1])
        segments = []
        for r, k in enumerate(order):
            instances[k]["id"] = base + r
            if present[at + r]:
                segments.append(instances[k])
        at += len(order)
        for label in range(NUM_STUFF):
            if dec[i, label]:
                segments.append({"category_id": label + 1 + class_num, "id": int(dec[i, label]), "iscrowd": 0, "bbox": [], "area": 0})
        res = {"segments_info": segments}
        p = o["pix"][i]
        if "rgb" in o:
            res["rgb"] = host[o["rgb"] + 3 * p:o["rgb"] + 3 * (p + h * w)].reshape(h, w, 3).copy()
        if "sem" in o:
            res["sem"] = host[o["sem"] + p:o["sem"] + p + h * w].reshape(h, w).copy()
        if "ids" in o:
            res["ids"] = host[o["ids"] + 4 * p:o["ids"] + 4 * (p + h * w)].view(np.uint32).reshape(h, w).copy()
        results.append(res)
    return results, int(dec[nimg - 1, NUM_STUFF])


def semantic_file_table(names_file):
    """image file name with .png extension -> '<line number>.npy' (:55-60: the i-th line names the image whose semantic
    map is stored as i.npy)."""
    table = {}
    with open(names_file) as f:
        for i, line in enumerate(f):
            table[line[:-4] + "png"] = "%d.npy" % i
    return table


ENCODE_WORKERS = 16


def _generate_device(todo, class_num, device, batch_images, save_root, sem_seg_root):
    """generate's loop with the merge on the device: `todo` = [(template annotation, semantic file, instance records)].  While
    a batch is on the device the thread pool encodes the pngs of the batch before it.  Returns the annotations."""
    from concurrent.futures import ThreadPoolExecutor

    def save(array, folder, name):
        Image.fromarray(array).save(os.path.join(folder, name))

    annotations, seg_id, waiting = [], 1, []
    if todo:
        os.makedirs(save_root, exist_ok=True)
    if sem_seg_root is not None:
        os.makedirs(sem_seg_root, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(ENCODE_WORKERS, os.cpu_count() or 1)) as pool:
        for b in range(0, len(todo), batch_images):
            chunk = todo[b:b + batch_images]
            items = [(np.load(sem_file), segments) for _, sem_file, segments in chunk]
            results, seg_id = merge_images_device(items, class_num, seg_id, device,
                                                  ("rgb", "sem") if sem_seg_root is not None else ("rgb",))
            for f in waiting:
                f.result()  # at most two batches of arrays are alive; an encoder's error surfaces here
            waiting = []
            for (ann, _, _), res in zip(chunk, results):
                waiting.append(pool.submit(save, res["rgb"], save_root, ann["file_name"]))
                if sem_seg_root is not None:
                    waiting.append(pool.submit(save, res["sem"], sem_seg_root, ann["file_name"]))
                annotations.append({"file_name": ann["file_name"], "image_id": ann["image_id"],
                                    "segments_info": res["segments_info"]})
        for f in waiting:
            f.result()
    return annotations


def generate(root, class_num=800, split="train", device=None, batch_images=16, sem_seg_root=None):
    """The whole script over the reference's directory layout below `root` (its paths are relative to the working
    directory): reads the panoptic template, the pseudo instance file and the semantic maps, writes the png id maps and
    coco{split}_{class_num}.json under prepare_ours/u2seg_annotations/panoptic_annotations/.  Returns the json dict.
    device (e.g. "cuda"): the images are merged `batch_images` at a time by merge_images_device, same files and json.
    sem_seg_root (device path only): the label maps separate_semantic_from_panoptic(json, pngs, sem_seg_root,
    create_cate(class_num)) would write are written there directly, without reading the pngs back."""
    if device is None and sem_seg_root is not None:
        raise ValueError("sem_seg_root belongs to the device path; on the host run separate_semantic_from_panoptic")
    if batch_images < 1:
        raise ValueError("batch_images must be at least 1")
    ann_root = os.path.join(root, "datasets", "prepare_ours", "u2seg_annotations")
    template = json.load(open(os.path.join(root, "datasets", "datasets", "panoptic_anns", "panoptic_%s2017.json" % split)))
    pseudo = json.load(open(os.path.join(ann_root, "ins_annotations", "coco%s_%d_ins_panoptic.json" % (split, class_num))))
    table = semantic_file_table(os.path.join(ann_root, "semantic_annotations", "coco_%s_img_file_names.txt" % split))
    sem_dir = os.path.join(ann_root, "semantic_annotations", "stego_coco_%s_semantic_seg_resized" % split)
    save_root = os.path.join(ann_root, "panoptic_annotations", "coco%s_%d" % (split, class_num))
    out = {"images": template["images"], "info": template["info"], "licenses": template["licenses"], "annotations": [],
           "categories": create_cate(class_num)}
    seen = {img["id"]: False for img in template["images"]}
    seg_id = 1
    if device is not None:
        todo = []
        for ann in template["annotations"]:
            sem_file = os.path.join(sem_dir, table[ann["file_name"]])
            record = pseudo["annotations"].get(str(ann["image_id"]))
            if record is not None:
                todo.append((ann, sem_file, record["segments_info"]))
                seen[ann["image_id"]] = True
        out["annotations"] = _generate_device(todo, class_num, device, batch_images, save_root, sem_seg_root)
    for ann in template["annotations"] if device is None else ():
        semantic = np.load(os.path.join(sem_dir, table[ann["file_name"]]))
        record = pseudo["annotations"].get(str(ann["image_id"]))
        if record is None:
            continue  # an image without pseudo instances is left out altogether
        combined, segments, seg_id = merge_image(semantic, record["segments_info"], class_num, seg_id)
        seen[ann["image_id"]] = True
        os.makedirs(save_root, exist_ok=True)
        Image.fromarray(id2rgb(combined)).save(os.path.join(save_root, ann["file_name"]))
        out["annotations"].append({"file_name": ann["file_name"], "image_id": ann["image_id"], "segments_info": segments})
    out["images"] = [img for img in out["images"] if seen[img["id"]]]
    with open(os.path.join(ann_root, "panoptic_annotations", "coco%s_%d.json" % (split, class_num)), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False)
    return out


# ------------------------------------------------------------------------------------------------
# the other label-preparation steps of datasets/prepare_ours/
# ------------------------------------------------------------------------------------------------
def classaware_instance_annotations(template, cluster_results, mask_annotations, num_categories=300):
    """generate_classaware_instanceseg_annotations.py:36-70: class-agnostic instance masks (CutLER / MaskCut records with
    an "ins_id") receive the cluster id of their crop ("<ins_id>.jpg" in the clustering result) as category and their
    ins_id as annotation id; images without any instance are dropped.  Returns the COCO-format dict."""
    out = {"licenses": template["licenses"],
           "categories": [{"id": i + 1, "name": str(i + 1), "supercategory": str(i + 1)} for i in range(num_categories)],
           "images": template["images"], "info": template["info"], "annotations": []}
    seen = set()
    for ann in mask_annotations:
        ann["category_id"] = cluster_results[str(ann["ins_id"]) + ".jpg"]
        ann["id"] = ann["ins_id"]
        out["annotations"].append(ann)
        seen.add(ann["image_id"])
    out["images"] = [img for img in out["images"] if img["id"] in seen]
    return out


# COCO panoptic stuff category id -> 1-based index of its supercategory (get_panoptic_anns_supercategory.py:9-13); the
# contiguous-order form of the same table is evaluation/sem_seg_evaluation.py:STUFF_TO_SUPERCATEGORY
STUFF_ID_TO_SUPERCATEGORY = dict(zip(
    (92, 93, 95, 100, 107, 109, 112, 118, 119, 122, 125, 128, 130, 133, 138, 141, 144, 145, 147, 148, 149, 151, 154, 155, 156,
     159, 161, 166, 168, 171, 175, 176, 177, 178, 180, 181, 184, 185, 186, 187, 188, 189, 190, 191, 192, 193, 194, 195, 196,
     197, 198, 199, 200),
    (1, 1, 2, 3, 4, 1, 4, 5, 6, 7, 8, 2, 4, 4, 9, 1, 8, 8, 8, 10, 8, 2, 8, 10, 4, 8, 4, 2, 1, 11, 11, 11, 11, 10, 12, 12, 6, 9,
     13, 14, 4, 4, 5, 8, 15, 6, 8, 3, 7, 2, 15, 11, 1)))


def panoptic_supercategory_annotations(standard, cluster_num):
    """get_panoptic_anns_supercategory.py:15-27: in the ground-truth panoptic json every stuff category id becomes
    cluster_num + its supercategory index, in the segments and in the category table (in place; returns `standard`)."""
    for ann in standard["annotations"]:
        for seg in ann["segments_info"]:
            if seg["category_id"] in STUFF_ID_TO_SUPERCATEGORY:
                seg["category_id"] = STUFF_ID_TO_SUPERCATEGORY[seg["category_id"]] + cluster_num
    for cate in standard["categories"]:
        if cate["id"] in STUFF_ID_TO_SUPERCATEGORY:
            cate["id"] = STUFF_ID_TO_SUPERCATEGORY[cate["id"]] + cluster_num
    return standard


def separate_semantic_from_panoptic(panoptic_json, panoptic_root, sem_seg_root, categories):
    """prepare_stuff_panoptic_fpn.py:21-75: one uint8 label map per panoptic png - things 0, the stuff categories 1.. in the
    order of `categories`, everything unlabelled 255 - the `sem_seg_file_name` inputs of the training data path."""
    os.makedirs(sem_seg_root, exist_ok=True)
    stuff_ids = [k["id"] for k in categories if k["isthing"] == 0]
    assert len(stuff_ids) <= 254
    id_map = {sid: i + 1 for i, sid in enumerate(stuff_ids)}
    id_map.update({k["id"]: 0 for k in categories if k["isthing"] == 1})
    id_map[0] = 255
    with open(panoptic_json) as f:
        obj = json.load(f)
    for anno in obj["annotations"]:
        panoptic = rgb2id(np.asarray(Image.open(os.path.join(panoptic_root, anno["file_name"])), dtype=np.uint32))
        output = np.full(panoptic.shape, 255, dtype=np.uint8)
        for seg in anno["segments_info"]:
            output[panoptic == seg["id"]] = id_map[seg["category_id"]]
        Image.fromarray(output).save(os.path.join(sem_seg_root, anno["file_name"]))
    return len(obj["annotations"])
