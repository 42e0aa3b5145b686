"""Float64 torch version of USL's regularised selection (get_selection_with_reg_imagenet,
u2seg/Instance_Clustering/shared/utils/nn_utils_imagenet.py:105-218), the yardstick of tests/test_usl_select_host.py and
tests/test_gpu_usl_select.py.

The regularizer is computed in float64 (difference form, exact zeros for duplicated rows); the per-cluster pick uses the
reference's own fp32 expression 1 / nd - w * reg on the fp32 rounding of reg, walked cluster by cluster as the reference
walks them, so that a planted fp32 tie resolves as it does there."""
import torch

F64 = torch.float64


def horizon_dists(x, y, horizon_num, chunk=16):
    """[N, H] float64: the H smallest sum_d (x_i - y_j)^2 of every row, ascending, and their positions j (ties: smaller j)."""
    x64, y64 = x.to(F64), y.to(F64)
    vals, inds = [], []
    for i0 in range(0, x64.shape[0], chunk):
        d = ((x64[i0:i0 + chunk, None, :] - y64[None, :, :]) ** 2).sum(-1)
        s = torch.sort(d, dim=1, stable=True)
        vals.append(s.values[:, :horizon_num])
        inds.append(s.indices[:, :horizon_num])
    if not vals:
        return x64.new_zeros((0, horizon_num)), torch.zeros((0, horizon_num), dtype=torch.long, device=x.device)
    return torch.cat(vals), torch.cat(inds)


def masked_horizon(v, j, labels, exclude_same_cluster):
    """The reference's mask (nn_utils_imagenet.py:169, 191-198): 1e10 where the position j equals the row's label
    (exclude_same_cluster) or where the distance is 0 (otherwise); a 0 left after it is the reference's AssertionError."""
    v = v.clone()
    if exclude_same_cluster:
        v[j == labels.to(j.device).reshape(-1, 1)] = 1e10
        if bool((v == 0).any()):
            raise AssertionError("zero distance left after the same-cluster mask")
    else:
        v[v == 0] = 1e10
    return v


def regularizer64(x, y, labels, reg, horizon_num, alpha=1, momentum=0.5, exclude_same_cluster=False):
    """One update of the selection regularizer in float64 (reg as given, any dtype): reg * m + new * (1 - m)."""
    v, j = horizon_dists(x, y, horizon_num)
    v = masked_horizon(v, j, labels, exclude_same_cluster)
    new = (1 / v).sum(1) if alpha == 1 else (1 / v ** alpha).sum(1)
    return reg.to(F64) * momentum + new * (1 - momentum)


def select_loop(neighbors_dist, reg32, labels, num_centroids, final_sample_num, w):
    """The reference's per-cluster walk (nn_utils_imagenet.py:123-143) in fp32: list of picked rows."""
    nd = neighbors_dist.float()
    scores_all = 1 / nd - w * reg32.float().to(nd.device)
    labels = labels.to(nd.device)
    picks = []
    for c in range(num_centroids):
        if len(picks) == final_sample_num:
            break
        match = torch.where(labels == c)[0]
        if len(match) == 0:
            continue
        picks.append(int(match[scores_all[match].argmax()]))
    return picks


def get_selection_with_reg64(data, neighbors_dist, cluster_labels, num_centroids, iters=1, final_sample_num=None, w=1,
                             momentum=0.5, horizon_num=256, alpha=1, exclude_same_cluster=False, return_regs=False):
    """The contract end to end: (picks of the last round as a list, [reg after every update] if return_regs)."""
    reg = torch.zeros(neighbors_dist.shape[0], dtype=F64, device=neighbors_dist.device)
    regs = []
    for it in range(iters):
        picks = select_loop(neighbors_dist, reg.float(), cluster_labels, num_centroids, final_sample_num, w)
        if it < iters - 1:
            sel = torch.tensor(picks, dtype=torch.long, device=data.device)
            reg = regularizer64(data, data[sel], cluster_labels, reg, horizon_num, alpha, momentum, exclude_same_cluster)
            regs.append(reg)
    assert len(picks) == final_sample_num
    return (picks, regs) if return_regs else picks


def score_leads(neighbors_dist, reg32, labels, num_centroids, final_sample_num, w):
    """Per visited cluster with two or more members: (best - second) / |best| of the fp32 scores (inf for one member)."""
    scores_all = (1 / neighbors_dist.float() - w * reg32.float()).to(F64)
    out, n = [], 0
    for c in range(num_centroids):
        if n == final_sample_num:
            break
        s = scores_all[labels == c]
        if s.numel() == 0:
            continue
        n += 1
        if s.numel() == 1:
            out.append(float("inf"))
            continue
        top = torch.topk(s, 2).values
        out.append(float((top[0] - top[1]) / top[0].abs()))
    return out
