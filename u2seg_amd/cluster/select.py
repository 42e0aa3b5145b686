"""Density-based pick of one representative per cluster (u2seg/Instance_Clustering/shared/utils/nn_utils.py:408-439,
called from selective_labeling/usl-imagenet.py:139-152 right after k-means with neighbors_dist = d_knns.mean(1)), and the
regularised variant that the shipped stage-1 config runs (get_selection_with_reg_imagenet, shared/utils/nn_utils_imagenet.py:
105-218, USL.REG.NITERS 2 in configs/ImageNet_usl_dino_0.2.yaml), with the files the reference run writes from its result.

The reference loops over the clusters and masks the full label vector once per cluster (K passes over N); here one stable
two-key sort puts every cluster's rows together in order of increasing key (ties: smaller row index), and the first
row of each run is the answer - the same result in O(N log N) on whatever device the tensors live on.  The regularizer
(the H nearest selected representatives of every row) runs in usl.hip."""
import csv
import ctypes
import os

import numpy as np
import torch

from .. import _hip


def _first_per_cluster(labels, key):
    """(cluster ids in increasing order, the row with the smallest key in each; equal keys: the smaller row index)."""
    by_key = torch.sort(key, stable=True).indices               # rows by key, equal keys by row index
    by_label = torch.sort(labels[by_key], stable=True)          # ... then grouped by cluster, order inside a group kept
    rows = by_key[by_label.indices]
    sorted_labels = by_label.values
    first = torch.ones_like(sorted_labels, dtype=torch.bool)
    first[1:] = sorted_labels[1:] != sorted_labels[:-1]
    return sorted_labels[first], rows[first]


def get_selection_without_reg(cluster_labels, neighbors_dist, centroid_ordering, final_sample_num):
    """For every cluster id in `centroid_ordering` (an int n means range(n)) that has members: the row with the smallest
    neighbors_dist.  Returns a numpy int array in the order of `centroid_ordering`, cut to final_sample_num; fewer
    non-empty clusters than that is an error, as in the reference."""
    labels = torch.as_tensor(cluster_labels).reshape(-1).long()
    dist = torch.as_tensor(neighbors_dist).reshape(-1).to(labels.device)
    if isinstance(centroid_ordering, int):
        centroid_ordering = range(centroid_ordering)
    ordering = torch.as_tensor(list(centroid_ordering), dtype=torch.long, device=labels.device)
    best_label, best_row = _first_per_cluster(labels, dist)
    k = int(max(int(ordering.max()) if ordering.numel() else -1, int(best_label.max()) if best_label.numel() else -1)) + 1
    table = torch.full((max(k, 1),), -1, dtype=torch.long, device=labels.device)
    table[best_label] = best_row
    picked = table[ordering]
    selected = picked[picked >= 0].cpu().numpy()
    assert selected.shape[0] >= final_sample_num, "Insufficient data: expected: {}, actual: {}".format(
        final_sample_num, selected.shape[0])
    return selected[:final_sample_num]


def cluster_label_table(names, cluster_labels):
    """{"<crop file name>": cluster id}: the form in which the clustering result enters the label preparation
    (datasets/prepare_ours/generate_classaware_instanceseg_annotations.py:38,55 reads `cluster_results[str(ins_id) + ".jpg"]`)."""
    labels = np.asarray(torch.as_tensor(cluster_labels).cpu()).tolist()
    assert len(names) == len(labels)
    return {str(n): int(c) for n, c in zip(names, labels)}


# ---- regularised selection (nn_utils_imagenet.py:105-218) ---------------------------------------------------------------

HORIZON_MAX = 64  # usl.hip keeps H + 4 candidates per row in LDS; the reference's default of 256 is not served


def _check_horizon(horizon_num):
    if isinstance(horizon_num, bool) or not isinstance(horizon_num, (int, np.integer)) or not 1 <= horizon_num <= HORIZON_MAX:
        raise ValueError("horizon_num must be an int in [1, %d] (got %r)" % (HORIZON_MAX, horizon_num))
    return int(horizon_num)


def selection_regularizer(data, selected_data, cluster_labels, reg, horizon_num, alpha=1, momentum=0.5,
                          exclude_same_cluster=False):
    """One update of the selection regularizer (nn_utils_imagenet.py:147-212): for every row of `data` [N, D] the
    `horizon_num` smallest squared distances to the rows of `selected_data` [S, D], masked as the reference masks them
    (exclude_same_cluster: 1e10 where the POSITION in selected_data equals the row's cluster label; otherwise 1e10 where
    the distance is 0), new = sum 1 / v ** alpha, and reg * momentum + new * (1 - momentum).  Returns a new fp32 [N]
    tensor.  A distance of 0 that survives the mask raises the reference's AssertionError."""
    horizon_num = _check_horizon(horizon_num)
    if data.dim() != 2 or selected_data.dim() != 2 or selected_data.shape[1] != data.shape[1]:
        raise ValueError("data [N, D] and selected_data [S, D] expected (got %s, %s)"
                         % (tuple(data.shape), tuple(selected_data.shape)))
    n, d = data.shape
    s = selected_data.shape[0]
    if d % 16 != 0:
        raise ValueError("the feature dimension must be a multiple of 16 (got %d)" % d)
    if horizon_num > s:
        raise ValueError("horizon_num = %d exceeds the %d selected rows" % (horizon_num, s))
    assert data.is_cuda, "selection_regularizer runs on the GPU"
    x = data.float().contiguous()
    y = selected_data.to(x.device).float().contiguous()
    labels = torch.as_tensor(cluster_labels).to(x.device).reshape(-1).long().contiguous()
    reg_in = torch.as_tensor(reg).to(x.device).reshape(-1).float().contiguous()
    assert labels.numel() == n and reg_in.numel() == n
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    zero_count = torch.zeros(1, dtype=torch.int32, device=x.device)
    ws_n = ctypes.c_longlong(0)
    if _hip.call_nostream("u2_usl_reg_workspace_ints", n, s, d, horizon_num, ctypes.addressof(ws_n)) != 0:
        raise ValueError("selection_regularizer: unsupported shape N %d, S %d, D %d, H %d" % (n, s, d, horizon_num))
    ws = torch.empty(ws_n.value, dtype=torch.int32, device=x.device)
    # the reference's scalars: torch rounds both factors to fp32; 1 - momentum is formed in double first
    _hip.call("u2_usl_regularizer", x, y, labels, reg_in, out, zero_count, ws, n, s, d, horizon_num, float(alpha),
              float(momentum), float(1 - momentum), 1 if exclude_same_cluster else 0)
    zeros = int(zero_count.item())
    if zeros > 0:
        raise AssertionError("%d rows keep a zero distance to a selected row after the same-cluster mask" % zeros)
    return out


def get_selection_with_reg_imagenet(data, neighbors_dist, cluster_labels, num_centroids, iters=1, final_sample_num=None,
                                    w=1, momentum=0.5, horizon_num=256, alpha=1, exclude_same_cluster=False, verbose=False):
    """nn_utils_imagenet.py:105-218 on the GPU: `iters` rounds of "pick, in every non-empty cluster c = 0 .. num_centroids-1,
    the member with the largest 1 / neighbors_dist - w * reg (first row on a tie), stop at final_sample_num picks", with
    the regularizer updated between rounds.  Returns the last round's picks (numpy int64, cluster order).

    Deviations: horizon_num must lie in [1, 64] and not exceed the number of picks (ValueError; the reference default 256
    included), a NaN score raises ValueError where the reference's argmax would pick it, and final_sample_num=None fails
    the reference's closing assertion before any device work."""
    del verbose
    horizon_num = _check_horizon(horizon_num)
    assert final_sample_num is not None, "final_sample_num is required (the reference asserts len(selected) == it)"
    final_sample_num = int(final_sample_num)
    if int(iters) < 1:
        raise ValueError("iters must be >= 1 (got %r)" % iters)
    assert torch.cuda.is_available(), "get_selection_with_reg_imagenet runs on the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(data).to(dev).float().contiguous()
    nd = torch.as_tensor(neighbors_dist).to(dev).reshape(-1).float()
    labels = torch.as_tensor(cluster_labels).to(dev).reshape(-1).long()
    if not (x.shape[0] == nd.numel() == labels.numel()):
        raise ValueError("data, neighbors_dist and cluster_labels disagree in length")
    reg = torch.zeros_like(nd)
    inv_nd = torch.reciprocal(nd)  # 1 / nd as torch evaluates the reference's expression
    # the reference walks cls_ind in range(num_centroids) only: other labels go to a bucket past the last cluster
    walk_labels = torch.where((labels >= 0) & (labels < num_centroids), labels, torch.full_like(labels, num_centroids))
    for it in range(int(iters)):
        score = inv_nd - reg * w  # fp32 product with w as fp32, then the difference (no fma)
        if bool(torch.isnan(score).any()):
            raise ValueError("NaN in the selection score (neighbors_dist or the regularizer)")
        # per-cluster argmax, first row on a tie = the smallest -score; + 0.0 turns -0.0 into 0.0, so that the sort keeps
        # the two in row order as argmax's comparison does
        best_label, best_row = _first_per_cluster(walk_labels, -score + 0.0)
        sel = best_row[best_label < num_centroids][:final_sample_num]  # cluster order; empty clusters have no entry
        if it < iters - 1:
            reg = selection_regularizer(x, x[sel], labels, reg, horizon_num, alpha=alpha, momentum=momentum,
                                        exclude_same_cluster=exclude_same_cluster)
    sel = sel.cpu().numpy().astype(np.int64)
    assert len(sel) == final_sample_num
    return sel


def get_sample_info_imagenet(final_sample_num):
    """nn_utils_imagenet.py:88-102: (num_centroids, chosen_percent)."""
    if final_sample_num == 12820:
        num_centroids, chosen_percent = 12900, 1
    elif final_sample_num == 2911:
        num_centroids, chosen_percent = 2911, 0.2
    else:
        num_centroids, chosen_percent = final_sample_num, 0.2 * final_sample_num / 2911
    return num_centroids, chosen_percent


def get_selection(selection_fn, *args, seed=None, recompute=True, save=True, pass_seed=False, run_dir=".", **kwargs):
    """nn_utils.py:442-460: runs selection_fn, saved as / loaded from <run_dir>/selected_indices_<final>[_<seed>].npy
    (overwritten when it exists; the reference's save_npy refuses to)."""
    seed_suffix = "_{}".format(seed) if seed is not None else ""
    path = os.path.join(run_dir, "selected_indices_{}{}.npy".format(kwargs["final_sample_num"], seed_suffix))
    if not recompute:
        return np.load(path)
    selected = selection_fn(*args, seed=seed, **kwargs) if pass_seed else selection_fn(*args, **kwargs)
    if save:
        os.makedirs(run_dir, exist_ok=True)
        np.save(path, selected)
    return selected


def split_csv_names(chosen_percent, run_name, seed=0):
    """The two file names of save_data (nn_utils_imagenet.py:55-75, usl-imagenet.py:166): selected, then remaining."""
    part = run_name if seed == 0 else "{}_seed{}".format(run_name, seed)
    return ("train_{}p_gen_{}_index.csv".format(chosen_percent, part),
            "train_{}p_gen_{}_index.csv".format(100 - chosen_percent, part))


def write_index_csv(path, indices, image_ids):
    """gen_csv_data (nn_utils_imagenet.py:36-53): rows `Index,ImageID` in increasing index order, the bytes pandas'
    to_csv(index=False) writes (csv module, minimal quoting, '\\n' line ends, utf-8)."""
    rows = np.sort(np.asarray(indices, dtype=np.int64))
    with open(path, "w", encoding="utf-8", newline="") as f:
        wr = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
        wr.writerow(["Index", "ImageID"])
        for i in rows.tolist():
            wr.writerow([i, image_ids[i]])


def save_split_csvs(run_dir, selected, image_ids, chosen_percent, run_name, seed=0):
    """save_data(gen_mode="ours") (nn_utils_imagenet.py:55-75): the selected rows and the sorted remainder, as two CSVs in
    run_dir (overwritten when they exist; the reference refuses to).  image_ids[i] = "<class dir>/<file>" of row i.
    Returns the two paths."""
    sel_name, rem_name = split_csv_names(chosen_percent, run_name, seed)
    selected = np.asarray(selected, dtype=np.int64)
    remaining = np.setdiff1d(np.arange(len(image_ids), dtype=np.int64), selected)
    os.makedirs(run_dir, exist_ok=True)
    paths = os.path.join(run_dir, sel_name), os.path.join(run_dir, rem_name)
    write_index_csv(paths[0], selected, image_ids)
    write_index_csv(paths[1], remaining, image_ids)
    return paths
