"""Instance predictions in COCO result format and the cluster -> category mapping step of the U2Seg instance evaluation
(detectron2/evaluation/coco_evaluation.py:40-213, 227-335, 590-640).

mode "hungarian_matching": confident detections (score >= 0.6) vote for the category of every ground-truth box they
overlap with IoU > 0.7; the majority mapping of the 300 evaluated clusters is written to
./hungarian_matching/instance_mapping.json (the reference then exits).  mode "eval": the mapping is applied, detections of
unmapped clusters are dropped, category ids go back to dataset ids, the results are written in COCO format and scored by
evaluation/cocoeval.py (box AP / AR without pycocotools; its matching and accumulation are pinned to the reference's C++
evaluation core).  With "segm" among the tasks the same core also scores the masks (mask AP; the reference's evaluator skips
that task, :352-354, but carries the code for it, :672-679): process() collects, per image, the pixel counts mask IoU needs
(evaluation/mask_ops.py, on the device when the predictions are there), evaluate() turns them into IoU tables.  Ground truth
stored as polygons (COCO's instances_val2017.json: every non-crowd instance) is refused by default and, with
gt_polygons="rasterize", rasterised by data/polygon.py's restatement of cocoapi's conversion - on the device next to the
predictions' planes (csrc/polygon.hip), by the definition itself on a CPU-only evaluator.  coco_eval="device"
runs cocoeval.py's matching and accumulation stages on the GPU (csrc/cocoeval.hip) with the same results."""
import itertools
import json
import os

import numpy as np
import torch

from ..data import rle
from ..data.catalog import MetadataCatalog
from ..data.detection_utils import BoxMode
from ..structures import Instances
from . import hungarian, mask_ops
from .evaluator import DatasetEvaluator, gather_to_rank0

SCORE_THRESH = 0.6
IOU_THRESH = 0.7
NUM_EVAL_CLUSTERS = 300
NUM_GT_CLASSES = 80


def instances_to_coco_json(instances, img_id, rles=None):
    """[{"image_id", "category_id", "bbox": [x, y, w, h], "score", "segmentation": compressed RLE}] for one image.
    rles: the masks' RLEs when they were encoded elsewhere (on the device) and pred_masks was dropped."""
    n = len(instances)
    if n == 0:
        return []
    boxes = BoxMode.convert(instances.pred_boxes.tensor.numpy(), BoxMode.XYXY_ABS, BoxMode.XYWH_ABS).tolist()
    scores = instances.scores.tolist()
    classes = instances.pred_classes.tolist()
    if rles is None and instances.has("pred_masks"):
        rles = [rle.encode(np.asarray(m, dtype=np.uint8)) for m in instances.pred_masks.numpy()]
    results = []
    for k in range(n):
        r = {"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k]}
        if rles is not None:
            r["segmentation"] = rles[k]
        results.append(r)
    return results


class COCOEvaluator(DatasetEvaluator):
    def __init__(self, dataset_name, output_dir=None, *, mode="hungarian_matching",
                 mapping_path="./hungarian_matching/instance_mapping.json", tasks=("bbox",), gt_polygons="refuse",
                 coco_eval="host"):
        self._metadata = MetadataCatalog.get(dataset_name)
        self._tasks = tuple(tasks)
        if gt_polygons not in ("refuse", "rasterize"):
            raise ValueError('gt_polygons must be "refuse" or "rasterize", got %r' % (gt_polygons,))
        self._gt_polygons = gt_polygons
        if coco_eval not in ("host", "device"):
            raise ValueError('coco_eval must be "host" or "device", got %r' % (coco_eval,))
        if coco_eval == "device":  # matching and accumulation by csrc/cocoeval.hip: no GPU is an error
            from . import cocoeval_ops

            cocoeval_ops.require_gpu()
        self._coco_eval = coco_eval
        if "bbox" not in self._tasks or set(self._tasks) - {"bbox", "segm"}:
            raise ValueError('tasks must be ("bbox",) or ("bbox", "segm"), got %r' % (tasks,))
        self._output_dir = output_dir
        self.mode = mode
        self.hungarain_matching_save_path = mapping_path
        data = json.load(open(self._metadata.json_file))
        self._img_to_anns = {}
        for ann in data.get("annotations", []):
            self._img_to_anns.setdefault(ann["image_id"], []).append(ann)
        self._cpu = torch.device("cpu")
        if "segm" in self._tasks:
            for ann in data.get("annotations", []):
                if ann.get("segmentation") is None:
                    raise ValueError("annotation %s of %s has no segmentation: mask AP needs RLE ground truth"
                                     % (ann.get("id"), dataset_name))
                if mask_ops.is_polygon(ann["segmentation"]) and gt_polygons == "rasterize":
                    mask_ops.gt_polygons(ann)  # the json is read as it is: every polygon of k >= 1 points is rasterised
                elif mask_ops.is_polygon(ann["segmentation"]):
                    raise NotImplementedError(
                        "annotation %s of %s has a polygon segmentation: mask AP needs RLE ground truth, polygons are not "
                        "supported (no polygon rasteriser in this project)" % (ann.get("id"), dataset_name))
        self.reset()

    def reset(self):
        self._predictions = []

    def process(self, inputs, outputs):
        items = [(inp, out["instances"]) for inp, out in zip(inputs, outputs) if "instances" in out]
        pairs = "segm" in self._tasks and self.mode == "eval"  # the cluster mapping votes with boxes: no pair counts
        work = [k for k, (_, inst) in enumerate(items) if inst.has("pred_masks") and (pairs or inst.pred_masks.is_cuda)]
        done = {}
        # masks on a GPU are encoded (and, for "segm", intersected with the image's ground truth) there, all images of the
        # call together; what comes back are strings and counts, and pred_masks is dropped before the move to the host
        for on_gpu in (True, False):
            sel = [k for k in work if items[k][1].pred_masks.is_cuda == on_gpu]
            if not sel:
                continue
            gts = anns = None
            if pairs and self._gt_polygons == "rasterize":
                anns = [self._img_to_anns.get(items[k][0]["image_id"], []) for k in sel]
            elif pairs:
                gts = []
                for k in sel:
                    inp, inst = items[k]
                    h, w = (int(v) for v in inst.pred_masks.shape[1:])
                    gts.append([mask_ops.gt_counts(a, h, w, inp["image_id"]) for a in self._img_to_anns.get(inp["image_id"], [])])
            for k, res in zip(sel, mask_ops.mask_batch_any([items[k][1].pred_masks for k in sel], gts, gt=anns)):
                done[k] = res
        for k, (inp, inst) in enumerate(items):
            res = done.get(k)
            if res is not None:
                inst = Instances(inst.image_size, **{n: v for n, v in inst.get_fields().items() if n != "pred_masks"})
            inst = inst.to(self._cpu)
            pred = {"image_id": inp["image_id"],
                    "instances": instances_to_coco_json(inst, inp["image_id"], None if res is None else res["rles"])}
            if pairs and res is not None:
                anns = self._img_to_anns.get(inp["image_id"], [])
                h, w = (int(v) for v in items[k][1].pred_masks.shape[1:])
                area_gt = res["area_gt"] if "area_gt" in res else np.array([rle.area(a["segmentation"]) for a in anns], dtype=np.int64)
                pred["segm_pairs"] = {"gt_ids": [a["id"] for a in anns], "inter": res["inter"], "area_dt": res["area"], "area_gt": area_gt}
            self._predictions.append(pred)

    def cluster_mapping(self, coco_results, num_clusters=NUM_EVAL_CLUSTERS):
        """do_hangarain_mapping (:227-271) without the file write."""
        gt_id = dict(self._metadata.thing_dataset_id_to_contiguous_id)
        preds, targets = [], []
        for r in coco_results:
            if r["score"] < SCORE_THRESH:
                continue
            anns = self._img_to_anns.get(r["image_id"], [])
            if not anns:
                continue
            ious = hungarian.box_iou_xywh(r["bbox"], [a["bbox"] for a in anns])
            for a, iou in zip(anns, ious.tolist()):
                if iou > IOU_THRESH:
                    targets.append(gt_id[a["category_id"]])
                    preds.append(r["category_id"])
        return hungarian.majority_vote_mapping(preds, targets, range(num_clusters), NUM_GT_CLASSES)

    def evaluate(self):
        parts = gather_to_rank0(self._predictions)
        if parts is None:
            return {}  # only the main process evaluates (:189-197)
        predictions = list(itertools.chain(*parts))
        coco_results = list(itertools.chain(*[p["instances"] for p in predictions]))
        if self.mode == "hungarian_matching":
            mapping = self.cluster_mapping(coco_results)
            hungarian.save_mapping(mapping, self.hungarain_matching_save_path)
            return {"instance_mapping": mapping}
        mapping = hungarian.load_mapping(self.hungarain_matching_save_path)
        to_dataset = {v: k for k, v in self._metadata.thing_dataset_id_to_contiguous_id.items()}
        remapped, kept_rows = [], {}
        for p in predictions:
            for row, r in enumerate(p["instances"]):
                c = mapping.get(r["category_id"], -1)
                if c == -1:
                    continue
                r = dict(r)
                r["category_id"] = to_dataset[c]
                remapped.append(r)
                kept_rows.setdefault(p["image_id"], []).append(row)
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "coco_instances_results.json"), "w") as f:
                json.dump(remapped, f)
        results = {"num_results": len(remapped), "num_dropped": len(coco_results) - len(remapped)}
        results.update(self._box_metrics(remapped))
        if "segm" not in self._tasks:
            return {"bbox": results}
        return {"bbox": results, "segm": self._mask_metrics(remapped, predictions, kept_rows)}

    def _mask_metrics(self, coco_results, predictions, kept_rows):
        """The "segm" numbers: the pair counts of process(), cut down to the detections the mapping kept, through
        cocoeval.evaluate_segm."""
        from . import cocoeval

        if any("segmentation" not in r for r in coco_results):
            raise ValueError('the "segm" task needs pred_masks on every prediction')
        pair_counts = {}
        for p in predictions:
            rows = kept_rows.get(p["image_id"])
            if rows and "segm_pairs" in p:
                sp = p["segm_pairs"]
                pair_counts[p["image_id"]] = {"gt_ids": sp["gt_ids"], "inter": np.asarray(sp["inter"])[rows],
                                              "area_dt": np.asarray(sp["area_dt"])[rows], "area_gt": sp["area_gt"]}
        polygons = self._gt_polygons == "rasterize"
        return self._metrics(coco_results, lambda ds, rs: cocoeval.evaluate_segm(ds, rs, pair_counts=pair_counts, polygons=polygons,
                                                                                 engine=self._coco_eval))

    def _box_metrics(self, coco_results):
        """AP, AP50, AP75, APs, APm, APl (x 100, NaN where undefined) and the per-category APs, as _derive_coco_results
        reports them (:473-540; the reference skips the "segm" task, :346-347), from evaluation/cocoeval.py."""
        from . import cocoeval

        return self._metrics(coco_results, lambda ds, rs: cocoeval.evaluate_bbox(ds, rs, engine=self._coco_eval))

    def _metrics(self, coco_results, evaluate):
        names = ("AP", "AP50", "AP75", "APs", "APm", "APl")
        if not coco_results:
            return {n: float("nan") for n in names}  # "No predictions from the model!"
        dataset = json.load(open(self._metadata.json_file))
        out = evaluate(dataset, coco_results)
        res = {n: (out["stats"][n] * 100 if out["stats"][n] >= 0 else float("nan")) for n in names}
        cats = sorted(dataset["categories"], key=lambda c: c["id"])
        if len(cats) > 1:
            for k, cat in enumerate(cats):
                p = out["precision"][:, :, k, 0, -1]
                p = p[p > -1]
                res["AP-" + str(cat.get("name", cat["id"]))] = float(p.mean() * 100) if p.size else float("nan")
        return res
