from .coco_evaluation import COCOEvaluator, instances_to_coco_json
from .evaluator import DatasetEvaluator, DatasetEvaluators, inference_on_dataset
from .panoptic_evaluation import COCOPanopticEvaluator
from .sem_seg_evaluation import SemSegEvaluator



def build_evaluator(cfg, dataset_name, output_folder=None, eval_mode="eval", tasks=("bbox",), panoptic_pq="files",
                    gt_polygons="refuse", coco_eval="host", sem_seg_boundary_iou=False):
    """tools/train_net.py:42-81 of the reference for the evaluator types the U2Seg datasets carry: semantic, instance and
    panoptic evaluators for "coco_panoptic_seg".  tasks: what the instance evaluator scores, ("bbox",) or ("bbox", "segm");
    panoptic_pq: "files" (PQ from the written pngs) or "counts" (from pair counts made on the device);
    gt_polygons: "refuse" or "rasterize" polygon ground truth in the "segm" task;
    coco_eval: "host" or "device", where the instance evaluator's AP matching and accumulation run;
    sem_seg_boundary_iou: the semantic evaluator also reports the reference's Boundary IoU."""
    import os

    from ..data.catalog import MetadataCatalog

    if output_folder is None:
        output_folder = os.path.join(cfg.OUTPUT_DIR, "inference")
    kind = MetadataCatalog.get(dataset_name).evaluator_type
    evaluators = []
    if kind in ("sem_seg", "coco_panoptic_seg"):
        evaluators.append(SemSegEvaluator(dataset_name, output_dir=output_folder, mode=eval_mode,
                                          boundary_iou=sem_seg_boundary_iou))
    if kind in ("coco", "coco_panoptic_seg"):
        evaluators.append(COCOEvaluator(dataset_name, output_dir=output_folder, mode=eval_mode, tasks=tasks,
                                        gt_polygons=gt_polygons, coco_eval=coco_eval))
    if kind == "coco_panoptic_seg":
        evaluators.append(COCOPanopticEvaluator(dataset_name, output_folder, pq=panoptic_pq))
    if not evaluators:
        raise NotImplementedError("no Evaluator for the dataset {} with the type {}".format(dataset_name, kind))
    return evaluators[0] if len(evaluators) == 1 else DatasetEvaluators(evaluators)


__all__ = ["build_evaluator", "COCOPanopticEvaluator", "COCOEvaluator", "DatasetEvaluator", "DatasetEvaluators", "SemSegEvaluator", "inference_on_dataset",
           "instances_to_coco_json"]
