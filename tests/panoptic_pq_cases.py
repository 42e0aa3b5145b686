"""Inputs shared by test_panoptic_pq_host.py and test_gpu_panoptic_pq.py: families of (ground-truth ids, ground-truth
segments, predicted ids, predicted segments) samples, each family built so that it holds at least one true positive, one false
positive, one false negative and one excused prediction, and the small on-disk panoptic dataset of the evaluator tests."""
import json
import os

import numpy as np
from PIL import Image

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hand_cases():
    """The three cases of test_evaluation.py::test_panoptic_quality_hand_cases restated: a perfect prediction; one with a
    shrunk segment, a wrong category, a stray segment on void and a spill onto void; the same against crowd ground truth."""
    cats = {1: {"isthing": 1}, 2: {"isthing": 1}, 7: {"isthing": 0}}
    gt = np.zeros((10, 10), dtype=np.int64)
    gt[:5, :5] = 1
    gt[5:, :] = 2
    gt[:5, 5:8] = 3
    gt_segs = [{"id": 1, "category_id": 1, "iscrowd": 0}, {"id": 2, "category_id": 7, "iscrowd": 0},
               {"id": 3, "category_id": 2, "iscrowd": 0}]
    samples = [(gt, gt_segs, gt * 10, [{"id": 10, "category_id": 1}, {"id": 20, "category_id": 7}, {"id": 30, "category_id": 2}])]
    pred = np.zeros_like(gt)
    pred[:4, :5] = 10
    pred[5:, :] = 20
    pred[:5, 5:8] = 30
    pred[:2, 8:] = 40
    pred[2:4, 8:] = 20
    samples.append((gt, gt_segs, pred, [{"id": 10, "category_id": 1}, {"id": 20, "category_id": 7},
                                        {"id": 30, "category_id": 1}, {"id": 40, "category_id": 2}]))
    crowd = [dict(s) for s in gt_segs]
    crowd[2]["iscrowd"] = 1
    samples.append((gt, crowd, pred, [{"id": 10, "category_id": 1}, {"id": 20, "category_id": 7},
                                      {"id": 30, "category_id": 2}, {"id": 40, "category_id": 2}]))
    return samples, cats


def big_id(k):
    """Segment number k re-drawn as an id that uses all three colour bytes (> 65 535)."""
    return 70001 * int(k) + 131072


def golden_cases():
    """The converted predictions of eval_golden.json ("panoptic_eval") against a ground truth derived from them: the map
    shifted by (2, 3) pixels, segment 1 kept (a match), segment 3 given another category (a false positive and a false
    negative), segment 4 made crowd (its prediction is excused), the erased region given an id that segments_info leaves
    out, every id re-drawn above 65 535."""
    fx = json.load(open(os.path.join(GOLD, "eval_golden.json")))
    samples, cats = [], {}
    for p in fx["panoptic_eval"]:
        pred = np.array(p["ids"], dtype=np.int64)
        info = {s["id"]: s for s in p["segments_info"]}
        shifted = np.roll(pred, (2, 3), axis=(0, 1))
        gt = np.where(shifted == 0, big_id(9), 0)  # the unlisted id
        gt_segs = []
        for sid, seg in info.items():
            gt[shifted == sid] = big_id(sid)
            cat = seg["category_id"]
            cats[cat] = {"isthing": int(cat < 300)}
            entry = {"id": big_id(sid), "category_id": cat, "iscrowd": 0}
            if sid == 3:
                entry["category_id"] = 399
            if sid == 4:
                entry["iscrowd"] = 1
            gt_segs.append(entry)
        gt[:2, :] = 0  # some real void
        samples.append((gt, gt_segs, pred, [dict(s) for s in p["segments_info"]]))
    cats[399] = {"isthing": 0}
    return samples, cats


def blocky_case(h, w, cell, seed, with_area, k=12):
    """A seeded map of cell x cell blocks: ground-truth ids of 24 bits, one of them not in segments_info, one crowd; the
    prediction is the map shifted by (3, 5) pixels with dense ids, two segments of another category than their ground truth
    and a stray segment where the ground truth is void."""
    rs = np.random.RandomState(seed)
    cells = rs.randint(0, k + 1, size=((h + cell - 1) // cell, (w + cell - 1) // cell))
    cells.flat[: k + 1] = np.arange(k + 1)  # every segment occurs
    seg = np.kron(cells, np.ones((cell, cell), dtype=np.int64))[:h, :w]
    ids = np.sort(rs.choice(np.arange(65536, 1 << 24), size=k, replace=False))
    cats = {c: {"isthing": int(c < 5)} for c in range(1, 9)}
    gt = np.zeros((h, w), dtype=np.int64)
    gt_segs, pred_segs = [], []
    for s in range(1, k + 1):
        gt[seg == s] = ids[s - 1]
        cat = int(rs.randint(1, 9))
        if s != 2:  # segment 2's id stays out of segments_info
            entry = {"id": int(ids[s - 1]), "category_id": cat, "iscrowd": int(s == 3)}
            if with_area:
                entry["area"] = int((seg == s).sum())
            gt_segs.append(entry)
        pred_segs.append({"id": s, "category_id": cat if s not in (4, 5) else cat % 8 + 1})
    pred = np.roll(seg, (3, 5), axis=(0, 1))
    pred[pred == 0] = k + 1  # the stray segment: almost all of it on void
    pred[:1, :] = 0
    pred_segs.append({"id": k + 1, "category_id": 1})
    rs.shuffle(gt_segs)
    return (gt, gt_segs, pred, pred_segs), cats


def num_pred_cols(pred_segs):
    return max([s["id"] for s in pred_segs] + [0]) + 1


def gt_table_of(gt_segs):
    return sorted({s["id"] for s in gt_segs})


def stat_dicts(stat):
    return {"iou": stat.iou, "tp": stat.tp, "fp": stat.fp, "fn": stat.fn}


def outcome_counts(stat, samples):
    """(true positives, false positives, false negatives, excused predictions) of a family."""
    tp, fp, fn = (sum(t.values()) for t in (stat.tp, stat.fp, stat.fn))
    return tp, fp, fn, sum(len(s[3]) for s in samples) - tp - fp


def write_tiny_dataset(root, name):
    """A panoptic dataset on disk for the evaluator: the three images of eval_golden.json, ground truth = golden_cases()'s,
    written as pngs + json; registered in the MetadataCatalog under `name`.  Returns (inputs, outputs factory, fixture): the
    outputs are the raw merge results ("panoptic_inputs": cluster categories, an unmapped cluster 298 that eval mode erases)."""
    import torch

    from u2seg_amd.data import MetadataCatalog
    from u2seg_amd.data.pseudo_panoptic import id2rgb

    fx = json.load(open(os.path.join(GOLD, "eval_golden.json")))
    samples, cats = golden_cases()
    gt_dir = os.path.join(root, "panoptic_gt")
    os.makedirs(gt_dir)
    annotations = []
    for p, (gt, gt_segs, _, _) in zip(fx["panoptic_eval"], samples):
        Image.fromarray(id2rgb(gt)).save(os.path.join(gt_dir, p["file_name"]))
        annotations.append({"image_id": p["image_id"], "file_name": p["file_name"], "segments_info": gt_segs})
    for q in fx["panoptic_inputs"]:  # hungarian_matching mode keeps the cluster ids as categories
        for s in q["segments_info"]:
            cats.setdefault(s["category_id"], {"isthing": int(bool(s["isthing"]))})
    categories = [dict(v, id=k) for k, v in sorted(cats.items())]
    gt_json = os.path.join(root, "panoptic_gt.json")
    json.dump({"images": fx["images"], "annotations": annotations, "categories": categories}, open(gt_json, "w"))
    thing_ids = sorted(c["id"] for c in fx["categories"])
    MetadataCatalog.get(name).set(panoptic_json=gt_json, panoptic_root=gt_dir,
                                  thing_dataset_id_to_contiguous_id={c: i for i, c in enumerate(thing_ids)})
    inputs = [{"image_id": im["id"], "file_name": os.path.join(root, "images", im["file_name"]), "height": im["height"],
               "width": im["width"]} for im in fx["images"]]

    def outputs(device="cpu"):
        return [{"panoptic_seg": (torch.tensor(q["ids"], dtype=torch.int32).to(device), [dict(s) for s in q["segments_info"]])}
                for q in fx["panoptic_inputs"]]

    return inputs, outputs, fx


def write_mapping_files(fx, where="hungarian_matching"):
    os.makedirs(where, exist_ok=True)
    json.dump(fx["instance_mapping_file"], open(os.path.join(where, "instance_mapping.json"), "w"))
    json.dump(fx["semantic_mapping_file"], open(os.path.join(where, "semantic_mapping.json"), "w"))


def read_tree(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def seeded_merge(sizes, n_inst, seed, dev):
    """Id maps from the real merge (combine_semantic_and_instance_outputs_batch) on seeded instances: blob masks pasted by the
    paste kernel, a blocky semantic map.  Returns [(panoptic int32 [H, W] on dev, segments_info)]."""
    import torch

    from u2seg_amd.modeling.inference import combine_semantic_and_instance_outputs_batch, paste_masks_in_images
    from u2seg_amd.structures import Boxes, Instances

    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    probs, boxes = [], []
    for h, w in sizes:
        c = torch.rand(n_inst, 2, generator=g) * 12 + 8
        s = torch.rand(n_inst, generator=g) * 6 + 4
        p = torch.exp(-((xx[None] - c[:, 0, None, None]) ** 2 + (yy[None] - c[:, 1, None, None]) ** 2) / (2 * s[:, None, None] ** 2))
        bw, bh = torch.rand(n_inst, generator=g) * w * 0.4 + 16, torch.rand(n_inst, generator=g) * h * 0.4 + 16
        x0, y0 = torch.rand(n_inst, generator=g) * (w - 16), torch.rand(n_inst, generator=g) * (h - 16)
        probs.append(p.clamp(0, 1).to(dev))
        boxes.append(torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1).to(dev))
    masks = paste_masks_in_images(probs, boxes, list(sizes), 0.5)
    insts, sems = [], []
    for (h, w), m, b in zip(sizes, masks, boxes):
        inst = Instances((h, w))
        inst.pred_masks, inst.pred_boxes = m, Boxes(b)
        inst.scores = (torch.rand(n_inst, generator=g) * 0.5 + 0.5).to(dev)
        inst.pred_classes = torch.randint(0, 800, (n_inst,), generator=g).to(dev)
        sem = torch.randint(0, 28, (h // 50 + 1, w // 50 + 1), generator=g).repeat_interleave(50, 0).repeat_interleave(50, 1)
        insts.append(inst)
        sems.append(sem[:h, :w].contiguous().to(dev))
    return combine_semantic_and_instance_outputs_batch(insts, sems, 0.5, 4096, 0.5, 28)


THING_IDS = {c + 1: c for c in range(5)}  # dataset id -> contiguous id


def seeded_mappings():
    """cluster -> contiguous thing id / stuff supercategory, -1 = no counterpart (such segments are erased in eval mode)."""
    inst = {str(c): (-1 if c % 7 == 0 else c % 5) for c in range(800)}
    sem = {str(c): (-1 if c % 9 == 0 else c % 16) for c in range(28)}
    return inst, sem


def derived_ground_truth(pan, info, inst_map, sem_map):
    """Ground truth for a merged map, derived from it as golden_cases() does: shifted by (2, 3) pixels, 24-bit ids, the
    categories the mappings give (an unmapped segment gets category 399), every fifth segment crowd, every seventh another
    category, segment 2 left out of segments_info, a band of void."""
    shifted = np.roll(np.asarray(pan, dtype=np.int64), (2, 3), axis=(0, 1))
    gt = np.zeros_like(shifted)
    segs = []
    for s in info:
        gt[shifted == s["id"]] = big_id(s["id"])
        t = (inst_map if s["isthing"] else sem_map)[str(s["category_id"])]
        cat = 399 if t == -1 else (t + 1 if s["isthing"] else (300 + t if t else 0))
        if s["id"] % 7 == 3:
            cat = 399
        if s["id"] != 2:
            segs.append({"id": big_id(s["id"]), "category_id": cat, "iscrowd": int(s["id"] % 5 == 4)})
    gt[:4, :] = 0
    return gt, segs


SEEDED_CATEGORIES = ([{"id": c, "isthing": 1} for c in THING_IDS] + [{"id": 0, "isthing": 0}] +
                     [{"id": 300 + c, "isthing": 0} for c in range(1, 16)] + [{"id": 399, "isthing": 0}])


def write_dataset(root, name, images, categories, thing_ids):
    """images: [(image id, png name, ground-truth id map, ground-truth segments)] -> pngs + json under root, registered."""
    from u2seg_amd.data import MetadataCatalog
    from u2seg_amd.data.pseudo_panoptic import id2rgb

    gt_dir = os.path.join(root, "panoptic_gt")
    os.makedirs(gt_dir)
    annotations = []
    for image_id, file_name, gt, gt_segs in images:
        Image.fromarray(id2rgb(gt)).save(os.path.join(gt_dir, file_name))
        annotations.append({"image_id": image_id, "file_name": file_name, "segments_info": gt_segs})
    gt_json = os.path.join(root, "panoptic_gt.json")
    json.dump({"annotations": annotations, "categories": categories}, open(gt_json, "w"))
    MetadataCatalog.get(name).set(panoptic_json=gt_json, panoptic_root=gt_dir, thing_dataset_id_to_contiguous_id=dict(thing_ids))
