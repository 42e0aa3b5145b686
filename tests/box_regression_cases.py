"""Inputs of the box regression option tests (tests/test_box_regression_options_host.py, tests/test_gpu_box_regression_options.py):
the RPN levels and the class-specific head rows, drawn on the host so that every machine tests the same numbers, and the
views of them that box_expect / check_box of tests/test_gpu_box_loss_options.py take (rows of four deltas against a source
box and a ground truth, foreground label < 800).  The float64 side of the GPU tests runs on these on the CPU as well: the
host test holds the ambiguity cap on the reference alone before the GPU test relies on it."""
import math

import torch

from tests import box_loss_refs as refs

F64 = torch.float64
BF16 = torch.bfloat16
CLAMP = math.log(1000.0 / 16)
BETA = 0.5
KINDS = ["smooth_l1", "giou", "diou", "ciou"]
RPN_WEIGHTS = [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)]
HEAD_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
N_PLANTED = 8

# ---- RPN ---------------------------------------------------------------------------------------------
RPN_B, RPN_A, RPN_G, RPN_LP = 2, 3, 3, 32
RPN_LEVELS = ((5, 7, 8, 32.0), (2, 3, 16, 64.0))     # (h, w, stride, anchor size): 105 anchors (no multiple of 64) and 18 (< a wave)
RPN_NORM = 16.0                                       # batch_size_per_image * B of a small RPN


def level_anchors(h, w, stride, size):
    """Position-major, the aspect ratios 0.5 / 1 / 2 innermost: the order of the maps' columns."""
    out = []
    for y in range(h):
        for x in range(w):
            for ratio in (0.5, 1.0, 2.0):
                aw, ah = size / math.sqrt(ratio), size * math.sqrt(ratio)
                out.append([x * stride - aw / 2, y * stride - ah / 2, x * stride + aw / 2, y * stride + ah / 2])
    return torch.tensor(out, dtype=torch.float32)


def rpn_case(weights, seed, empty_level=False):
    """Two images over two levels; the second image has no ground truth (labels 0 / -1, its gt rows are zero).  The first
    level carries the N_PLANTED constructed positives of the box-head tests as its first positions' anchors, and a few drawn
    ones; the second level carries two drawn positives, or with `empty_level` none.  The cases are built through the
    PREDICTION (the three ground-truth boxes are shared by all anchors): deltas that decode to a box far away, inside the
    ground truth, around it, onto it (gt 1 IS that anchor, deltas 0: ambiguous by construction), a dw above the clamp, a
    ground truth 1 px wide, and |d| below and above beta.
    Returns CPU tensors: anchors (per level), labels int8 [B, Atot], match int32 [B, Atot], gt [B, G, 4], obj bf16 [B, Atot],
    deltas bf16 [B, Atot, 4], planted (anchor indices, in order)."""
    g = torch.Generator().manual_seed(seed)
    anchors = [level_anchors(*lv) for lv in RPN_LEVELS]
    n0, n1 = anchors[0].shape[0], anchors[1].shape[0]
    atot = n0 + n1
    cat = torch.cat(anchors)
    planted = [3 * p + 1 for p in (8, 9, 10, 11, 12, 15, 16, 17)]            # the square anchors of eight positions, rising
    gt = torch.zeros((RPN_B, RPN_G, 4))
    gt[0, 0] = torch.tensor([1.5, 3.25, 37.0, 29.5])
    gt[0, 1] = cat[planted[3]]
    gt[0, 2] = torch.tensor([20.0, 2.0, 21.0, 40.0])                         # 1 px wide
    labels = torch.where(torch.rand((RPN_B, atot), generator=g) < 0.4, 0, -1).to(torch.int8)
    match = torch.randint(0, RPN_G, (RPN_B, atot), generator=g).to(torch.int32)   # of non-positives: takes no part
    deltas = torch.randn((RPN_B, atot, 4), generator=g) * torch.tensor([0.5, 0.5, 0.3, 0.3])
    obj = torch.randn((RPN_B, atot), generator=g) * 2
    obj[0, 0], obj[0, 1] = 30.0, -30.0                                        # saturated objectness
    w = torch.tensor(weights, dtype=F64)

    def toward(a, box):
        return refs.get_deltas(cat[a][None].to(F64), box[None].to(F64), weights)[0]

    g0 = gt[0, 0].to(F64)
    side = torch.tensor([g0[2] - g0[0], g0[3] - g0[1]]).repeat(2)
    grow = side * torch.tensor([-0.3, -0.3, 0.3, 0.3], dtype=F64)
    rows = {
        planted[0]: (0, toward(planted[0], g0 + 5000.0)),                     # disjoint
        planted[1]: (0, toward(planted[1], g0 - 0.5 * grow)),                 # the prediction inside the ground truth
        planted[2]: (0, toward(planted[2], g0 + grow)),                       # the ground truth inside the prediction
        planted[3]: (1, torch.zeros(4, dtype=F64)),                           # prediction = ground truth
        planted[4]: (0, toward(planted[4], g0 + grow) * torch.tensor([1, 1, 0, 1]) + torch.tensor([0, 0, 5.0, 0]) * w),  # dw = 5
        planted[5]: (2, torch.zeros(4, dtype=F64)),                           # against the 1 px wide ground truth
        planted[6]: (0, toward(planted[6], g0) + torch.tensor([0.5, -0.5, 0.9, -0.9], dtype=F64) * BETA),   # |d| < beta
        planted[7]: (0, toward(planted[7], g0) + torch.tensor([1.1, -1.1, 3.0, -3.0], dtype=F64) * BETA),   # |d| > beta
    }
    for a, (gi, d) in rows.items():
        labels[0, a], match[0, a], deltas[0, a] = 1, gi, d.float()
    drawn = [3 * p + r for p, r in ((20, 0), (26, 2), (31, 1))] + ([] if empty_level else [n0 + 4, n0 + 11])
    for a in drawn:                                                           # drawn positives: near gt 0, deltas of the usual size
        labels[0, a], match[0, a] = 1, 0
        deltas[0, a] = (toward(a, g0) + torch.randn(4, generator=g).to(F64) * 0.2 * w / w[0]).float()
    if empty_level:
        labels[:, n0:] = torch.where(labels[:, n0:] == 1, 0, labels[:, n0:])
    assert int((labels[1] == 1).sum()) == 0
    return dict(anchors=anchors, labels=labels, match=match, gt=gt, obj=obj.to(BF16), deltas=deltas.to(BF16), planted=planted,
                weights=tuple(weights))


def rpn_maps(case, fused, device, pad=1e4):
    """The level maps the kernels read, on `device`: fused -> [(map [B, H, W, 32], None)] with objectness in columns 0-2 and the
    deltas in 3-14, else [(obj map, delta map)] with A and 4 A valid columns.  The pad columns hold `pad`."""
    out, off = [], 0
    for (h, w, _, _), anc in zip(RPN_LEVELS, case["anchors"]):
        n = anc.shape[0]
        o = case["obj"][:, off:off + n].reshape(RPN_B, h, w, RPN_A)
        d = case["deltas"][:, off:off + n].reshape(RPN_B, h, w, 4 * RPN_A)
        if fused:
            m = torch.full((RPN_B, h, w, RPN_LP), pad, dtype=BF16)
            m[..., :RPN_A], m[..., RPN_A:5 * RPN_A] = o, d
            out.append((m.to(device), None))
        else:
            mo = torch.full((RPN_B, h, w, RPN_LP), pad, dtype=BF16)
            md = torch.full((RPN_B, h, w, RPN_LP), pad, dtype=BF16)
            mo[..., :RPN_A], md[..., :4 * RPN_A] = o, d
            out.append((mo.to(device), md.to(device)))
        off += n
    return out


def rpn_split_grads(go, gd, fused):
    """One level's gradient map(s) -> (objectness gradient [B, n], delta gradient [B, n, 4], the pad columns flattened)."""
    b = go.shape[0]
    if fused:
        return (go[..., :RPN_A].reshape(b, -1), go[..., RPN_A:5 * RPN_A].reshape(b, -1, 4), go[..., 5 * RPN_A:].reshape(-1))
    return (go[..., :RPN_A].reshape(b, -1), gd[..., :4 * RPN_A].reshape(b, -1, 4),
            torch.cat([go[..., RPN_A:].reshape(-1), gd[..., 4 * RPN_A:].reshape(-1)]))


def rpn_level_rows(case, lvl):
    """One level as rows for box_expect / check_box: (pred bf16 [n, 4], source boxes, ground truth, labels int64 with 3 for a
    positive and 800 otherwise, number of planted rows), n = B * anchors of the level, image-major.  The planted rows are the
    level's first positives.  Rows that take no part get their anchor as ground truth (finite targets; they are masked)."""
    off = sum(a.shape[0] for a in case["anchors"][:lvl])
    anc = case["anchors"][lvl]
    n = anc.shape[0]
    lab8 = case["labels"][:, off:off + n]
    m = case["match"][:, off:off + n].long()
    pred = case["deltas"][:, off:off + n].reshape(-1, 4)
    prop = anc[None].expand(RPN_B, n, 4).reshape(-1, 4).contiguous()
    gtm = torch.gather(case["gt"], 1, m[..., None].expand(-1, -1, 4)).reshape(-1, 4)
    pos = (lab8 == 1).reshape(-1)
    gtm = torch.where(pos[:, None], gtm, prop)
    lab = torch.where(pos, 3, 800).to(torch.int64)
    return pred, prop, gtm, lab, (N_PLANTED if lvl == 0 else 0)


# ---- class-specific head rows ----------------------------------------------------------------------------
def cls_case(R, K, LP, weights, seed):
    """Rows drawn as box_inputs of tests/test_gpu_box_loss_options.py draws them, with labels in [0, K) for the 25 % foreground
    and K for the background, and 4 K valid columns of deltas; with R >= 65 the first N_PLANTED rows are its constructed ones,
    planted in their label's columns.  The other classes' columns and the pads hold noise.  CPU tensors:
    pred bf16 [R, LP], prop, gt fp32 [R, 4], lab int64 [R]."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((R, 2), generator=g) * torch.tensor([1300.0, 780.0])
    wh = 2 + torch.rand((R, 2), generator=g) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((R, 4), generator=g) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    lab = torch.where(torch.rand(R, generator=g) < 0.25, torch.randint(0, K, (R,), generator=g), torch.full((R,), K))
    pred = torch.randn((R, LP), generator=g)
    if R == 1:
        lab[0] = K - 1
    if R >= 65:
        own = torch.tensor([0, 1, K - 1, 3, K - 2, 5 % K, 2, 7 % K])     # even and odd classes: both halves of a 16-byte piece
        lab[:N_PLANTED] = own
        mine = torch.zeros((N_PLANTED, 4))
        grow = wh[:N_PLANTED].repeat(1, 2) * torch.tensor([-0.3, -0.3, 0.3, 0.3])
        gt[0] = prop[0] + 5000.0
        gt[1] = prop[1] + grow[1]
        gt[2] = prop[2] - 0.5 * grow[2]
        gt[3] = prop[3]
        gt[4] = prop[4] + grow[4]
        mine[4, 2] = 5.0 * weights[2]
        gt[5] = prop[5]
        gt[5, 2] = gt[5, 0] + 1
        tgt = refs.get_deltas(prop[6:8].to(F64), gt[6:8].to(F64), weights)
        mine[6] = (tgt[0] + torch.tensor([0.5, -0.5, 0.9, -0.9], dtype=F64) * BETA).float()
        mine[7] = (tgt[1] + torch.tensor([1.1, -1.1, 3.0, -3.0], dtype=F64) * BETA).float()
        for i in range(N_PLANTED):
            pred[i, 4 * int(own[i]):4 * int(own[i]) + 4] = mine[i]
    return pred.to(BF16), prop, gt, lab


def cls_columns(lab, K):
    """int64 [R, 4]: the four columns of each row's label; background rows point at columns 0-3 (they are masked)."""
    return 4 * torch.where(lab < K, lab, torch.zeros_like(lab))[:, None] + torch.arange(4, device=lab.device)


def cls_gathered(pred, lab, K):
    """(pred's labelled columns [R, 4], labels with 800 for the background): the class-agnostic problem of the same rows."""
    return pred.gather(1, cls_columns(lab, K)), torch.where(lab < K, lab, torch.full_like(lab, 800))
