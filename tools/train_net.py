#!/usr/bin/env python
"""Training / evaluation entry point with the CLI contract of the reference's tools/train_net.py:113-164
(--config-file, --num-gpus, --resume, --eval-only, trailing KEY VALUE overrides).  One process per GPU: launch N > 1 with
    python -m torch.distributed.run --nproc-per-node N tools/train_net.py --num-gpus N --config-file ...
Data: when the dataset DATASETS.TRAIN names is on disk (builtin registration under ./datasets or $DETECTRON2_DATASETS,
u2seg_amd/data/datasets.py) batches come from the real pipeline - DatasetMapper in DataLoader workers, aspect-ratio
grouping, DevicePrefetcher into HBM; otherwise (or with DATASETS.TRAIN ("synthetic",)) from the synthetic generator.
Deviation (recorded in DESIGN.md): the reference hard-wires --eval-only to True (engine/defaults.py:109); here it is a flag."""
import itertools
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from u2seg_amd.checkpoint import DetectionCheckpointer  # noqa: E402
from u2seg_amd.config import get_cfg  # noqa: E402
from u2seg_amd.data import (DatasetCatalog, DevicePrefetcher, MetadataCatalog, build_detection_train_loader,  # noqa: E402
                            make_synthetic_batch, register_all_coco)
from u2seg_amd.engine import (SimpleTrainer, default_argument_parser, get_bn_modules, launch_info,  # noqa: E402
                              precise_bn_due, update_bn_stats)
from u2seg_amd.modeling import build_model  # noqa: E402
from u2seg_amd.solver import build_lr_scheduler, build_optimizer  # noqa: E402
from u2seg_amd.utils.env import configure_host_threads  # noqa: E402
from u2seg_amd.utils.events import EventStorage, JSONWriter  # noqa: E402


def setup(args):
    cfg = get_cfg()
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(args.opts)
    cfg.freeze()
    return cfg


def real_batches(cfg, device, seed=None, device_mapper=False):
    """Iterator over device-resident training batches of the real dataset, or None when it is not on disk.
    seed: the sampler's seed (default: cfg.SEED, or a shared random one when it is negative).
    device_mapper: the workers ship raw records and DevicePrefetcher finishes them with csrc/augment.hip."""
    if device_mapper and not (str(device).startswith("cuda") and torch.cuda.is_available()):
        raise RuntimeError("--device-mapper finishes the samples with HIP kernels: it needs a GPU (MODEL.DEVICE is %r); there "
                           "is no host fallback" % (device,))
    names = [n for n in cfg.DATASETS.TRAIN if n != "synthetic"]
    if not names:
        return None
    register_all_coco()
    for n in names:
        meta = MetadataCatalog.get(n)
        if n not in DatasetCatalog or not os.path.isfile(meta.get("json_file", "")) or not os.path.isdir(meta.get("image_root", "")):
            return None
    if seed is None and cfg.SEED >= 0:
        seed = cfg.SEED
    loader = build_detection_train_loader(cfg, seed=seed, device_mapper=device_mapper)
    return iter(DevicePrefetcher(loader, device) if str(device).startswith("cuda") else loader)


def precise_bn_batches(cfg, device, per_gpu, rank, world):
    """The precise-BN pass's own stream of training batches (engine/defaults.py:439-446), independent of the training stream,
    created on the first pass and continued by later ones.  Real data: a second training loader from the same config with
    DATALOADER.NUM_WORKERS = 0, as the reference builds it "to not affect training", and a sampler seed of its own.  Synthetic
    data: generator indices past every index the training stream can reach (it uses (it * world + rank) * per_gpu + i for
    it < MAX_ITER)."""
    c = cfg.clone()
    c.defrost()
    c.DATALOADER.NUM_WORKERS = 0
    stream = real_batches(c, device, seed=None if cfg.SEED < 0 else cfg.SEED + 1)
    if stream is not None:
        return stream

    def synthetic():
        base = cfg.SOLVER.MAX_ITER * world
        for k in itertools.count():
            yield make_synthetic_batch(per_gpu, start_index=(base + k * world + rank) * per_gpu, device=device)

    return synthetic()


def evaluate_on_disk_datasets(cfg, model, eval_mode, device, tasks=("bbox",), panoptic_pq="files", gt_polygons="refuse",
                              coco_eval="host", sem_seg_boundary_iou=False, output_folder=None, instances_only=False):
    """The reference's Trainer.test (engine/defaults.py:591-640) for the DATASETS.TEST entries that are on disk: first run
    with --eval-mode hungarian_matching (writes ./hungarian_matching/*.json), then with --eval-mode eval.  None when no
    test dataset is available.  output_folder: where the evaluators write (default OUTPUT_DIR/inference); instances_only: the
    instance evaluator alone, for a model that returns nothing but "instances" (test-time augmentation)."""
    from u2seg_amd.data import build_detection_test_loader
    from u2seg_amd.evaluation import COCOEvaluator, build_evaluator, inference_on_dataset

    register_all_coco()
    results = {}
    for name in cfg.DATASETS.TEST:
        meta = MetadataCatalog.get(name)
        if name not in DatasetCatalog or not os.path.isfile(meta.get("json_file", "")):
            continue
        loader = build_detection_test_loader(cfg, name)
        stream = DevicePrefetcher(loader, device) if str(device).startswith("cuda") else loader
        if instances_only:
            if meta.evaluator_type not in ("coco", "coco_panoptic_seg"):
                continue
            evaluator = COCOEvaluator(name, output_dir=output_folder or os.path.join(cfg.OUTPUT_DIR, "inference"), mode=eval_mode,
                                      tasks=tasks, gt_polygons=gt_polygons, coco_eval=coco_eval)
        else:
            evaluator = build_evaluator(cfg, name, output_folder=output_folder, eval_mode=eval_mode, tasks=tasks,
                                        panoptic_pq=panoptic_pq, gt_polygons=gt_polygons, coco_eval=coco_eval,
                                        sem_seg_boundary_iou=sem_seg_boundary_iou)
        results[name] = inference_on_dataset(model, stream, evaluator)
    return results or None


def evaluate_with_tta(cfg, model, eval_mode, device, tasks=("bbox",), gt_polygons="refuse", coco_eval="host", outputs="instances",
                      panoptic_pq="files", sem_seg_boundary_iou=False):
    """The reference's Trainer.test_with_TTA (tools/train_net.py:96-109): the instance tasks once more with the model wrapped in
    GeneralizedRCNNWithTTA, written under OUTPUT_DIR/inference_TTA, every result key with the suffix _TTA.  The wrapper returns
    instances only, so of `tasks` the instance tasks (bbox, segm) are scored; None when there is none or no dataset on disk.
    outputs="panoptic" (--tta-outputs) on a PanopticFPN: the model wrapped in PanopticFPNWithTTA, which returns the semantic and
    panoptic outputs as well, in front of every evaluator build_evaluator gives the dataset."""
    from u2seg_amd.modeling import GeneralizedRCNNWithTTA, PanopticFPN, PanopticFPNWithTTA

    impl = "device" if str(device).startswith("cuda") else "host"
    if outputs == "panoptic" and isinstance(model, PanopticFPN):
        wrapped = PanopticFPNWithTTA(cfg, model, impl=impl)
        results = evaluate_on_disk_datasets(cfg, wrapped, eval_mode, device, tasks, panoptic_pq, gt_polygons, coco_eval,
                                            sem_seg_boundary_iou, output_folder=os.path.join(cfg.OUTPUT_DIR, "inference_TTA"))
        if results is None:
            return None
        return {name: {k + "_TTA": v for k, v in res.items()} for name, res in results.items()}
    tasks = tuple(t for t in tasks if t in ("bbox", "segm"))
    if not tasks:
        return None
    wrapped = GeneralizedRCNNWithTTA(cfg, model, impl=impl)
    results = evaluate_on_disk_datasets(cfg, wrapped, eval_mode, device, tasks, gt_polygons=gt_polygons, coco_eval=coco_eval,
                                        output_folder=os.path.join(cfg.OUTPUT_DIR, "inference_TTA"), instances_only=True)
    if results is None:
        return None
    return {name: {k + "_TTA": v for k, v in res.items()} for name, res in results.items()}


def main(args):
    configure_host_threads()
    rank, local_rank, world = launch_info()
    cfg = setup(args)
    if cfg.MODEL.DEVICE.startswith("cuda"):
        torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl" if torch.cuda.is_available() else "gloo")
    c = cfg.clone()
    c.defrost()
    if cfg.MODEL.DEVICE == "cuda":
        c.MODEL.DEVICE = "cuda:%d" % local_rank
    model = build_model(c)
    per_gpu = max(1, cfg.SOLVER.IMS_PER_BATCH // world)
    if args.eval_only:
        # tools/train_net.py:135-141 of the reference: weights from MODEL.WEIGHTS (or the last checkpoint with --resume)
        if cfg.MODEL.WEIGHTS and os.path.isfile(cfg.MODEL.WEIGHTS):
            DetectionCheckpointer(model, cfg.OUTPUT_DIR).resume_or_load(cfg.MODEL.WEIGHTS, resume=args.resume)
        tasks = tuple(t for t in args.eval_tasks.split(",") if t)
        results = evaluate_on_disk_datasets(cfg, model, args.eval_mode, c.MODEL.DEVICE, tasks, args.panoptic_pq,
                                            args.eval_gt_polygons, args.coco_eval, args.sem_seg_boundary_iou)
        if results is not None:
            # tools/train_net.py:134-135 of the reference.  Only the scoring pass: the hungarian_matching pass writes the cluster
            # mapping from the plain model's detections, and a second, augmented run of it would overwrite that file
            if cfg.TEST.AUG.ENABLED and args.eval_mode == "eval":
                with_tta = evaluate_with_tta(cfg, model, args.eval_mode, c.MODEL.DEVICE, tasks, args.eval_gt_polygons, args.coco_eval,
                                             args.tta_outputs, args.panoptic_pq, args.sem_seg_boundary_iou)
                for name, res in (with_tta or {}).items():
                    results[name].update(res)
            if rank == 0:
                print(results)
            return results
        model.eval()
        with torch.no_grad():
            out = model(make_synthetic_batch(per_gpu, start_index=rank * per_gpu, device=c.MODEL.DEVICE))
        if rank == 0:
            print("inference ok: %d images, %d instances in image 0" % (len(out), len(out[0]["instances"])))
        return out
    model.train()
    opt = build_optimizer(cfg, model)
    sched = build_lr_scheduler(cfg, opt)
    trainer = SimpleTrainer(model, opt, sched)
    checkpointer = DetectionCheckpointer(model, cfg.OUTPUT_DIR, save_to_disk=rank == 0, optimizer=opt, scheduler=sched)
    start_iter = 0
    if (cfg.MODEL.WEIGHTS and os.path.isfile(cfg.MODEL.WEIGHTS)) or args.resume:
        rest = checkpointer.resume_or_load(cfg.MODEL.WEIGHTS, resume=args.resume)
        # engine/defaults.py:410-421: only a run that found its own last_checkpoint continues at iteration + 1
        start_iter = int(rest.get("iteration", -1)) + 1 if args.resume and checkpointer.has_checkpoint() else 0
        sched.resume_at(start_iter)  # lr of iteration start_iter, milestones counted from iteration 0
    elif cfg.MODEL.WEIGHTS and rank == 0:
        print("MODEL.WEIGHTS %s not found: random initialisation" % cfg.MODEL.WEIGHTS)
    stream = real_batches(cfg, c.MODEL.DEVICE, device_mapper=args.device_mapper)
    if args.device_mapper and stream is None:
        raise RuntimeError("--device-mapper needs the real dataset %s on disk: the synthetic generator has no mapper"
                           % (cfg.DATASETS.TRAIN,))
    if rank == 0:
        print("data: %s" % ("real pipeline over %s" % (cfg.DATASETS.TRAIN,) if stream is not None else "synthetic generator"))
    # engine/defaults.py:428-452: the PreciseBN hook, registered before the checkpointer, so that the checkpoint of the same
    # iteration (model_final included) holds the recomputed statistics
    precise_bn = cfg.TEST.PRECISE_BN.ENABLED and len(get_bn_modules(model)) > 0
    if cfg.TEST.PRECISE_BN.ENABLED and not precise_bn and rank == 0:
        print("PreciseBN is disabled because model doesn't contain BN layers in training mode.")
    bn_stream = None
    # OUTPUT_DIR/metrics.json, one line per 20 iterations (engine/defaults.py:build_writers): appended to on --resume, and the
    # storage starts at start_iter so that the iteration numbers continue
    writer = None
    if rank == 0:
        os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
        writer = JSONWriter(os.path.join(cfg.OUTPUT_DIR, "metrics.json"))
    t0 = time.time()
    with EventStorage(start_iter) as storage:
        for it in range(start_iter, cfg.SOLVER.MAX_ITER):
            t_data = time.perf_counter()
            if stream is not None:
                batch = next(stream)
            else:
                batch = make_synthetic_batch(per_gpu, start_index=(it * world + rank) * per_gpu, device=c.MODEL.DEVICE)
            trainer.data_time = time.perf_counter() - t_data
            trainer.run_step(batch)
            last = it == cfg.SOLVER.MAX_ITER - 1
            if it % 20 == 0 or last:
                # the loop's one wait for the device; the metrics of the period that ended at iteration it - 1 (or ends here)
                # were copied to the host behind that iteration's optimizer step and are complete by now
                if rank == 0:
                    total = trainer.check_finite()
                    print("iter %d  total_loss %.4f  lr %.6f  %.2f s/iter" % (it, total, opt.lr, (time.time() - t0) / (it - start_iter + 1)))
                new = trainer.collect_metrics(storage, write=rank == 0)
                if last:  # the rows of a period that the end of training cut short
                    trainer.flush_metrics()
                    new = trainer.collect_metrics(storage, write=rank == 0) or new
                if new and writer is not None:
                    writer.write(storage)
            if precise_bn and precise_bn_due(it, cfg.SOLVER.MAX_ITER, cfg.TEST.EVAL_PERIOD):
                if bn_stream is None:
                    bn_stream = precise_bn_batches(cfg, c.MODEL.DEVICE, per_gpu, rank, world)
                if rank == 0:
                    print("Running precise-BN for %d iterations...  Note that this could produce different statistics every time."
                          % cfg.TEST.PRECISE_BN.NUM_ITER)
                update_bn_stats(model, bn_stream, cfg.TEST.PRECISE_BN.NUM_ITER)
            if (it + 1) % cfg.SOLVER.CHECKPOINT_PERIOD == 0 or last:
                checkpointer.save("model_%07d" % it if it < cfg.SOLVER.MAX_ITER - 1 else "model_final", iteration=it)
    if writer is not None:
        writer.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(default_argument_parser().parse_args())
