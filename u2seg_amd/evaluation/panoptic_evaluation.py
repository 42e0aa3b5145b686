"""Panoptic predictions in COCO panoptic format, with the U2Seg cluster -> category mapping applied
(detectron2/evaluation/panoptic_evaluation.py:24-190).

The evaluator looks for ./hungarian_matching/{semantic,instance}_mapping.json when it is built: without them it is in
"hungarian_matching" mode and stores the predictions as they are; with them ("eval") every segment's category goes through
the mapping - a thing cluster to the dataset id of its category, an unsupervised stuff class to cluster_num(300) + its
supercategory - and segments whose cluster has no mapping are erased from the id map.  evaluate() gathers the ranks,
writes the pngs and predictions.json and computes PQ / SQ / RQ with panopticapi's pq_compute when that package is
importable, with the restatement in evaluation/pq.py otherwise.

pq="counts" (opt-in; "files" is the behaviour above, untouched): PQ is computed from per-image pair-count tables instead of
from the pngs read back.  process() loads the image's ground-truth png and has evaluation/panoptic_ops.py count, for the whole
batch in one launch when the id maps are on the device, how many pixels every (ground-truth segment, predicted segment)
pair shares; evaluate() finishes with pq.pq_compute_counts.  The pngs and predictions.json are written all the same: they
are the reference's output.  Still parity unpinned (evaluation/pq.py)."""
import io
import itertools
import json
import os
import tempfile

import numpy as np
from PIL import Image

from ..data.catalog import MetadataCatalog
from ..data.pseudo_panoptic import id2rgb
from . import panoptic_ops
from .evaluator import DatasetEvaluator, gather_to_rank0

EVAL_CLUSTER_NUM = 300
MAPPING_DIR = "./hungarian_matching"


class COCOPanopticEvaluator(DatasetEvaluator):
    def __init__(self, dataset_name, output_dir=None, pq="files"):
        if pq not in ("files", "counts"):
            raise ValueError("pq must be \"files\" or \"counts\", not %r" % (pq,))
        self._pq = pq
        self._metadata = MetadataCatalog.get(dataset_name)
        self._thing_dataset_id = {v: k for k, v in self._metadata.thing_dataset_id_to_contiguous_id.items()}
        self._stuff_dataset_id = {i: EVAL_CLUSTER_NUM + i for i in range(1, 16)}
        self._stuff_dataset_id[0] = 0
        self._output_dir = output_dir
        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
        sem, ins = (os.path.join(MAPPING_DIR, n) for n in ("semantic_mapping.json", "instance_mapping.json"))
        if os.path.exists(sem):
            self.mode = "eval"
            self.semantic_mapping_dict = json.load(open(sem))
            self.instance_mapping_dict = json.load(open(ins))
        else:
            self.mode = "hungarian_matching"
        if self._pq == "counts":
            # read once, here: a missing ground truth must not surface at the end of a 5 000-image run
            gt_json, gt_folder = self._metadata.get("panoptic_json"), self._metadata.get("panoptic_root")
            if not (gt_json and os.path.isfile(gt_json)):
                raise FileNotFoundError("pq=\"counts\" needs the panoptic ground-truth json of %s: %r" % (dataset_name, gt_json))
            if not (gt_folder and os.path.isdir(gt_folder)):
                raise FileNotFoundError("pq=\"counts\" needs the panoptic ground-truth folder of %s: %r" % (dataset_name, gt_folder))
            data = json.load(open(gt_json))
            self._gt_folder = gt_folder
            self._gt_categories = {c["id"]: c for c in data["categories"]}
            self._gt_annotations = data["annotations"]
            self._gt_by_image = {a["image_id"]: a for a in data["annotations"]}
        self.reset()

    def reset(self):
        self._predictions = []

    def _mapped(self, segment):
        """The segment with its dataset category id, or None when its cluster has no counterpart."""
        isthing = segment.pop("isthing", None)
        if isthing is None:
            return segment  # the model already speaks dataset ids
        table, to_dataset = ((self.instance_mapping_dict, self._thing_dataset_id) if isthing is True
                             else (self.semantic_mapping_dict, self._stuff_dataset_id))
        target = table[str(segment["category_id"])]
        if target == -1:
            return None
        segment["category_id"] = to_dataset[target]
        return segment

    def _pair_counts(self, inputs, outputs):
        """Per image (counts, gt_table) from the merge kernel's raw ids, or None for an image without ground truth."""
        todo, preds, gts, tables, cols, names = [], [], [], [], [], []
        for k, (inp, out) in enumerate(zip(inputs, outputs)):
            ga = self._gt_by_image.get(inp["image_id"])
            if ga is None:
                continue
            ids, segments = out["panoptic_seg"]
            with Image.open(os.path.join(self._gt_folder, ga["file_name"])) as im:
                gts.append(np.asarray(im.convert("RGB")))
            todo.append(k)
            preds.append(ids)
            tables.append(sorted({s["id"] for s in ga["segments_info"]}))
            cols.append(max([s["id"] for s in segments] + [0]) + 1)
            names.append(inp["file_name"])
        result = [None] * len(inputs)
        if todo:
            if all(p.is_cuda for p in preds):
                tabs = panoptic_ops.pair_counts_batch(preds, gts, tables, cols, names)
            else:
                tabs = [panoptic_ops.host_pair_counts(p, g, t, c, nm) for p, g, t, c, nm in zip(preds, gts, tables, cols, names)]
            for k, tab, table in zip(todo, tabs, tables):
                result[k] = (tab, table)
        return result

    def process(self, inputs, outputs):
        tables = self._pair_counts(inputs, outputs) if self._pq == "counts" and self.mode != "hungarian_matching" else None
        for k, (inp, out) in enumerate(zip(inputs, outputs)):
            ids, segments = out["panoptic_seg"]
            ids = ids.cpu().numpy().copy()  # edited below: never the model's own output (shared with other evaluators)
            segments = [dict(seg) for seg in segments] if segments is not None else None
            assert segments is not None, "the PanopticFPN path always returns segments_info"
            if self.mode != "hungarian_matching":
                kept = []
                for seg in segments:
                    sid = seg["id"]
                    seg = self._mapped(seg)
                    if seg is None:
                        ids[ids == sid] = 0
                        if tables is not None and tables[k] is not None:
                            # the table was counted on the raw ids: moving the erased id's column into column 0 is what
                            # zeroing its pixels amounts to
                            tab = tables[k][0]
                            tab[:, 0] += tab[:, sid]
                            tab[:, sid] = 0
                    else:
                        kept.append(seg)
                segments = kept
            with io.BytesIO() as buf:
                Image.fromarray(id2rgb(ids)).save(buf, format="PNG")
                png = buf.getvalue()
            name = os.path.splitext(os.path.basename(inp["file_name"]))[0] + ".png"
            self._predictions.append({"image_id": inp["image_id"], "file_name": name, "png_string": png,
                                      "segments_info": segments})
            if tables is not None and tables[k] is not None:
                self._predictions[-1]["pq_counts"], self._predictions[-1]["pq_gt_table"] = tables[k]

    def evaluate(self):
        parts = gather_to_rank0(self._predictions)
        if parts is None:
            return None
        predictions = list(itertools.chain(*parts))
        pred_dir = self._output_dir or tempfile.mkdtemp(prefix="panoptic_eval")
        counted = {}
        for p in predictions:
            with open(os.path.join(pred_dir, p["file_name"]), "wb") as f:
                f.write(p.pop("png_string"))
            if "pq_counts" in p:  # not part of predictions.json
                counted[p["image_id"]] = (p.pop("pq_counts"), p.pop("pq_gt_table"), p["segments_info"])
        gt_json = self._metadata.get("panoptic_json")
        json_data = json.load(open(gt_json)) if gt_json and os.path.isfile(gt_json) else {}
        json_data["annotations"] = predictions
        predictions_json = os.path.join(pred_dir, "predictions.json")
        with open(predictions_json, "w") as f:
            f.write(json.dumps(json_data))
        result = {"predictions_json": predictions_json, "num_images": len(predictions)}
        gt_folder = self._metadata.get("panoptic_root")
        if not (gt_json and os.path.isfile(gt_json) and gt_folder and os.path.isdir(gt_folder)):
            return {"panoptic_seg": result}  # no panoptic ground truth on disk: the converted predictions are the output
        if self._pq == "counts" and self.mode != "hungarian_matching":
            from .pq import pq_compute_counts

            def samples():
                for ga in self._gt_annotations:
                    if ga["image_id"] not in counted:
                        raise KeyError("no prediction for the image with id %r" % ga["image_id"])
                    counts, table, segments = counted[ga["image_id"]]
                    yield counts, table, ga["segments_info"], segments

            result["pq_implementation"] = "u2seg_amd.evaluation.pq (device counts)"
            pq = pq_compute_counts(samples(), self._gt_categories)
            for group, suffix in (("All", ""), ("Things", "_th"), ("Stuff", "_st")):
                for key in ("pq", "sq", "rq"):
                    result[key.upper() + suffix] = 100 * pq[group][key]
            return {"panoptic_seg": result}
        try:
            from panopticapi.evaluation import pq_compute
        except ImportError:
            from .pq import pq_compute  # the same procedure restated (parity unpinned, see evaluation/pq.py)

            result["pq_implementation"] = "u2seg_amd.evaluation.pq"
        pq = pq_compute(gt_json, predictions_json, gt_folder=gt_folder, pred_folder=pred_dir)
        for group, suffix in (("All", ""), ("Things", "_th"), ("Stuff", "_st")):
            for key in ("pq", "sq", "rq"):
                result[key.upper() + suffix] = 100 * pq[group][key]
        return {"panoptic_seg": result}
