#!/usr/bin/env python
"""Stage 1 of U2Seg (u2seg/Instance_Clustering/selective_labeling/usl-imagenet.py): instance crops -> DINO ViT-B/8 CLS
features -> first-order kNN density -> k-means -> cluster_labels_decode.json, on cuda:0, in one process.

usage: python tools/cluster_instances.py --crops ROOT --weights dino_vitbase8_pretrain.pth --num-centroids 800
           [--seed 0 --niter 100 --knn-k 20 --batch 8 --workers 16 --out DIR]

ROOT is an ImageFolder tree (ROOT/train/<class>/<crop> as the reference reads it, or ROOT/<class>/<crop>).  Writes into DIR:
  cluster_labels_decode.json            {"<dir>/<file>": cluster id}  (nn_utils.py:85-107, keyed as the reference keys it)
  memory_feats_list.npy                 fp32 [N, 768] features in dataset order
  cluster_labels_<K>_<seed>.npy, centroids_<K>_<seed>.npy   (nn_utils.py:380-405)
and prints the time of each phase.  --num-centroids is explicit: the reference's get_sample_info_coco does not exist.
With --num-selected S it also runs the regularised selection of one representative per cluster that the shipped USL config
takes (get_selection_with_reg_imagenet, nn_utils_imagenet.py:105-218; the --reg-* defaults are USL.REG of
configs/ImageNet_usl_dino_0.2.yaml) and writes what the reference run writes from it:
  selected_indices_<S>_<seed>.npy                                    (nn_utils.py:442-460)
  train_<p>p_gen_<run>_index.csv, train_<100-p>p_gen_<run>_index.csv  (nn_utils_imagenet.py:36-75; p from
                                      get_sample_info_imagenet(S), <run> = --run-name, + _seed<s> for a seed other than 0)
Existing files are overwritten, as the other outputs are (the reference refuses to overwrite them).
The architecture follows the checkpoint (--arch auto); --arch base|small --patch-size P forces one of dino.py's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from u2seg_amd import _hip  # noqa: E402
from u2seg_amd.cluster import dino  # noqa: E402
from u2seg_amd.cluster.kmeans import run_kmeans  # noqa: E402
from u2seg_amd.cluster import select  # noqa: E402
from u2seg_amd.cluster.knn import first_order_density, partitioned_kNN  # noqa: E402
from u2seg_amd.data.crops import CropFolder, crop_loader  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--crops", required=True)
    p.add_argument("--weights", required=True)
    p.add_argument("--num-centroids", type=int, required=True)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--niter", type=int, default=100)
    p.add_argument("--knn-k", type=int, default=20)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--workers", type=int, default=16)
    p.add_argument("--size", type=int, default=480)
    p.add_argument("--arch", choices=("auto", "base", "small"), default="auto")
    p.add_argument("--patch-size", type=int, default=8)
    p.add_argument("--out", default="output/cluster_instances")
    p.add_argument("--num-selected", type=int, default=None, help="run the regularised USL selection of S representatives")
    p.add_argument("--reg-niters", type=int, default=2)
    p.add_argument("--reg-w", type=float, default=0.05)
    p.add_argument("--reg-momentum", type=float, default=0.0)
    p.add_argument("--reg-horizon", type=int, default=32)
    p.add_argument("--reg-alpha", type=float, default=1.0)
    p.add_argument("--reg-keep-same-cluster", action="store_true",
                   help="exclude_same_cluster=False (the shipped config excludes them)")
    p.add_argument("--run-name", default="imagenet_usl_dino_0.2")
    return p.parse_args(argv)


def run(args):
    assert torch.cuda.is_available(), "cluster_instances runs on cuda:0"
    _hip.load()
    dev = torch.device("cuda:0")
    times = {}
    t = time.time()
    root = os.path.join(args.crops, "train") if os.path.isdir(os.path.join(args.crops, "train")) else args.crops
    ds = CropFolder(root, size=args.size)
    loader = crop_loader(ds, batch_size=args.batch, workers=args.workers)
    arch = {"auto": None, "base": dino.vit_base, "small": dino.vit_small}[args.arch]
    model = dino.load_dino_weights(args.weights, arch(patch_size=args.patch_size) if arch else None, device=dev)
    times["setup_s"] = time.time() - t

    t = time.time()
    feats = dino.get_feats_list(model, loader)
    torch.cuda.synchronize()
    times["features_s"] = time.time() - t
    if not torch.isfinite(feats).all():
        raise RuntimeError("non-finite features")

    t = time.time()
    d_knns, _ = partitioned_kNN(feats, K=args.knn_k)
    density = first_order_density(d_knns)
    torch.cuda.synchronize()
    times["knn_s"] = time.time() - t

    t = time.time()
    labels, centroids = run_kmeans(feats, args.num_centroids, niter=args.niter, seed=args.seed)
    torch.cuda.synchronize()
    times["kmeans_s"] = time.time() - t

    os.makedirs(args.out, exist_ok=True)
    k, s = args.num_centroids, args.seed
    np.save(os.path.join(args.out, "memory_feats_list.npy"), feats.cpu().numpy())
    np.save(os.path.join(args.out, "cluster_labels_%d_%d.npy" % (k, s)), labels.cpu().numpy())
    np.save(os.path.join(args.out, "centroids_%d_%d.npy" % (k, s)), centroids.cpu().numpy())
    table = {key: int(c) for key, c in zip(ds.keys(), labels.cpu().tolist())}
    with open(os.path.join(args.out, "cluster_labels_decode.json"), "w") as f:
        json.dump(table, f)
    if args.num_selected is not None:
        t = time.time()
        _, chosen_percent = select.get_sample_info_imagenet(args.num_selected)
        selected = select.get_selection(
            select.get_selection_with_reg_imagenet, feats, d_knns.mean(dim=1), labels, k, final_sample_num=args.num_selected,
            iters=args.reg_niters, w=args.reg_w, momentum=args.reg_momentum, horizon_num=args.reg_horizon,
            alpha=args.reg_alpha, exclude_same_cluster=not args.reg_keep_same_cluster, seed=s, run_dir=args.out)
        select.save_split_csvs(args.out, selected, ds.keys(), chosen_percent, args.run_name, seed=s)
        times["selection_s"] = time.time() - t
    for name, v in times.items():
        print("%-12s %.3f" % (name, v))
    print("crops %d  features %s  clusters used %d  mean density %.4g" % (
        len(ds), tuple(feats.shape), int(torch.unique(labels).numel()), float(density.mean())))
    return feats, labels, centroids, table


if __name__ == "__main__":
    run(parse_args())
