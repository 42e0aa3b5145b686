"""Case tables and input generators of tests/test_gpu_losses_float64.py: the smallest shapes that reach every branch of the
head-loss kernels of u2seg_amd/csrc/losses.hip and of their launchers.  Everything here runs on the CPU from seeded generators,
so tests/test_loss_cases_host.py can hold the tables to the branches they are meant to reach - and count the near-ties of the
L1 cases - without a GPU.  Inputs are rounded to the formats the kernels read (bf16 activations, fp32 boxes and weights)."""
import numpy as np
import torch

from tests.box_loss_refs import get_deltas

F64 = torch.float64
BF16 = torch.bfloat16
PAD = 1e4            # what the pad columns of the row-wise inputs hold: finite in bf16, ruinous if read


def f32(v):
    """The fp32 value a launcher receives for the Python float v, as a Python float."""
    return float(np.float32(v))


def bf16_of(v):
    """The bf16 value a kernel stores for the fp32 scalar v, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32).to(BF16))


# ----------------------------------------------------------------------------------------------------------------------------
# u2_softmax_ce / u2_softmax_ce_stats: (R, NC, LP)
# ----------------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [
    (1, 2, 8),            # smallest accepted row
    (4, 8, 8),            # NC == LP, no pad columns
    (5, 81, 88),          # the default box head
    (70, 301, 320),       # u2seg_R50_300
    (9, 512, 512),        # 64 chunks, the second piece empty
    (9, 513, 520),        # one valid column in the second piece
    (6, 1017, 1024),      # the widest register-resident row, with a partly valid last chunk
    (6, 1025, 1032),      # general form through LP > 1024
    (37, 11, 13),         # general form through LP % 8 != 0
    (2051, 301, 320),     # grid capped at 512, waves walk several rows, R % 4 = 3
    (2050, 1025, 1032),   # general form with 513 work-groups, the last one half empty
]
SOFTMAX_THIRD = (70, 301, 320)      # the case whose gradient scale is float32(1 / 3) instead of 1 / R
SOFTMAX_WRAPPER = [(70, 301, 320), (37, 11, 13)]   # one wrapper call per form
SOFTMAX_KINDS = 8


def softmax_geometry(r, nc, lp):
    """The launcher's choices restated: (register form, work-groups, rows a wave walks at most, loss atomics at most, exp terms a
    lane sums)."""
    reg = lp <= 1024 and lp % 8 == 0
    grid = -(-r // 4)
    if reg:
        grid = min(grid, 512)
        return True, grid, -(-r // (4 * grid)), 4 * grid, 16
    return False, grid, 1, r, -(-nc // 64)


def softmax_gscale(case):
    return f32(1.0 / 3) if case == SOFTMAX_THIRD else f32(1.0 / case[0])


def softmax_case(r, nc, lp):
    """logits bf16 [r, lp], labels int64 [r].  Row i is of kind i % 8: gaussian; saturated (|z| up to 60); p -> 1 on the label;
    p -> 1 off the label; uniform; ties with the maximum in column 0; ties with the maximum in column nc - 1; labels 0 and nc - 1
    in turn.  Pad columns hold PAD."""
    g = torch.Generator().manual_seed(1000 * nc + r)
    z = torch.randn((r, lp), generator=g) * 3
    lab = torch.randint(0, nc, (r,), generator=g)
    sat = (torch.randn((r, nc), generator=g) * 25).clamp(-60, 60)
    rows = torch.arange(r)
    kind = rows % SOFTMAX_KINDS
    zz = z[:, :nc]
    zz[kind == 1] = sat[kind == 1]
    one = (kind == 2) | (kind == 3)
    hot = torch.where(kind == 3, (lab + 1) % nc, lab)
    zz[one] = -60.0
    zz[rows[one], hot[one]] = 60.0
    zz[kind == 4] = 1.5
    tie = (kind == 5) | (kind == 6)
    zz[tie] = zz[tie].round()
    mx = zz.amax(1)
    zz[rows[kind == 5], 0] = mx[kind == 5]
    zz[rows[kind == 6], nc - 1] = mx[kind == 6]
    ends = rows[kind == 7]
    lab[ends] = torch.where(ends % (2 * SOFTMAX_KINDS) == 7, 0, nc - 1)
    z[:, nc:] = PAD
    return z.to(BF16), lab


# ----------------------------------------------------------------------------------------------------------------------------
# u2_semseg_upsample_ce: (B, h, w, NC, LP, ignore, saturated)
# ----------------------------------------------------------------------------------------------------------------------------
SS_OW, SS_OH, SS_MAXC = 15, 7, 32
SEM_MAPS = [(1, 1), (1, 16), (8, 1), (7, 15), (8, 16), (15, 31)]
SEM_CLASSES = [(1, 8), (8, 8), (9, 16), (28, 32), (32, 32), (17, 64), (3, 40)]
SEM_PAD = 7.0


def _sem_cases():
    cases = [(b, h, w, 28, 32, 255, False) for (h, w) in SEM_MAPS for b in (1, 3)]
    cases += [(1 if i % 2 else 3, 8, 16, nc, lp, 255, False) for i, (nc, lp) in enumerate(SEM_CLASSES) if (nc, lp) != (28, 32)]
    cases += [(3, 15, 31, 32, 32, 255, False), (1, 8, 16, 28, 32, 255, True)]      # the widest case; the saturated one
    cases += [(1, 7, 15, 28, 32, 0, False), (3, 8, 16, 9, 16, 0, False)]           # ignore = 0
    return cases


SEM_CASES = _sem_cases()
SEM_WRAPPER = [(3, h, w, 28, 32, 255, False) for (h, w) in SEM_MAPS]


def sem_tiles(h, w):
    return -(-h // SS_OH), -(-w // SS_OW)


def sem_owner(h, w):
    """(tile row of every pixel row [4h], tile column of every pixel column [4w]): a pixel's loss is counted by the work-group
    that owns its upper-left tap, tap = max(floor((pixel - 2) / 4), 0)."""
    ys, xs = torch.arange(4 * h), torch.arange(4 * w)
    ty = torch.div(ys - 2, 4, rounding_mode="floor").clamp_min(0) // SS_OH
    tx = torch.div(xs - 2, 4, rounding_mode="floor").clamp_min(0) // SS_OW
    return ty, tx


def sem_case(b, h, w, nc, lp, ignore=255, saturated=False):
    """logits bf16 [b, h, w, lp] ~ N(0, 2) (saturated: a random class of every tap raised or lowered by 40), pads SEM_PAD;
    targets uint8 [b, 4h, 4w]: random valid labels (never `ignore`), about 10 % ignored; on a map of more than one tile every
    pixel owned by the last tile of every image is ignored."""
    g = torch.Generator().manual_seed(((h * 37 + w) * 41 + nc) * 3 + b + (7 if saturated else 0) + ignore)
    z = torch.randn((b, h, w, lp), generator=g) * 2
    if saturated:
        pick = torch.randint(0, nc, (b, h, w, 1), generator=g)
        sign = torch.where(torch.rand((b, h, w, 1), generator=g) < 0.5, -40.0, 40.0)
        z.scatter_add_(3, pick, sign)
    z[..., nc:] = SEM_PAD
    lo = 1 if ignore == 0 else 0
    assert nc > lo or ignore != 0
    t = torch.randint(lo, nc, (b, 4 * h, 4 * w), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.1] = ignore
    ny, nx = sem_tiles(h, w)
    if ny * nx > 1:
        ty, tx = sem_owner(h, w)
        t[:, (ty[:, None] == ny - 1) & (tx[None, :] == nx - 1)] = ignore
    return z.to(BF16), t.to(torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------------
# u2_scale_to_bf16
# ----------------------------------------------------------------------------------------------------------------------------
SCALE_N = [1, 255, 257, 4096 * 256 + 3]
SCALE_ARGS = [(True, True, 1.0), (False, True, 0.5), (True, False, 1.0), (True, True, 0.5)]   # (num given, den given, mult)
SCALE_NUM, SCALE_DEN = 0.37, 1234.0


# ----------------------------------------------------------------------------------------------------------------------------
# u2_mask_predict_bce / u2_mask_predict_bce_stats: (N, side, phased, classes); C = 256
# ----------------------------------------------------------------------------------------------------------------------------
MASK_C = 256
MASK_CASES = [
    (1, 2, False, 1),      # P = 4, one slice: smallest P, one class
    (3, 7, False, 5),      # 49, one slice: odd side, P below 128
    (2, 11, False, 3),     # 121, one slice: on the P = 128 threshold
    (2, 12, True, 80),     # 144, four slices: on the P = 128 threshold, phased
    (3, 14, True, 80),     # 196, four slices: 196 % 16 != 0
    (2, 22, False, 3),     # 484, four slices: on the P = 512 threshold
    (2, 23, False, 3),     # 529, eight slices: on the P = 512 threshold, odd side
    (1, 24, True, 1),      # 576, eight slices: N = 1, phased, one class
]


def mask_slices(p):
    return 8 if p >= 512 else (4 if p >= 128 else 1)


def mask_case(n, side, phased, k):
    """x bf16 [n, P, 256] in pixel order, w fp32 [k, 256], bias fp32 [k], cls int64 [n], target uint8 [n, P].  ROIs 0 and 1 share
    a class; the last ROI of a case with n >= 2 has a constant target (all 1 on an odd side, else all 0); positions 0 and 1 of
    ROI 0 are aligned with their class's weights: logits near +-80."""
    p = side * side
    g = torch.Generator().manual_seed(side * 100 + n * 10 + k)
    x = torch.randn((n, p, MASK_C), generator=g)
    w = torch.randn((k, MASK_C), generator=g) * 0.05
    bias = torch.randn(k, generator=g) * 0.1
    cls = torch.randint(0, k, (n,), generator=g)
    if n >= 2:
        cls[1] = cls[0]
    tgt = (torch.rand((n, p), generator=g) < 0.5).to(torch.uint8)
    if n >= 2:
        tgt[n - 1] = side % 2
    sgn = torch.sign(w[cls[0]])
    x[0, 0], x[0, 1] = 8 * sgn, -8 * sgn
    return x.to(BF16), w, bias, cls, tgt


def to_phases(x, side):
    """Pixel order [n, side * side, C] -> the deconvolution's unshuffled order: position ((h * S + w) * 4 + dy * 2 + dx) holds
    pixel (2 h + dy, 2 w + dx), S = side / 2."""
    n, _, c = x.shape
    s = side // 2
    return x.view(n, s, 2, s, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, side * side, c).contiguous()


def from_phases(x, side):
    n, _, c = x.shape
    s = side // 2
    return x.view(n, s, s, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, side * side, c).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------
# u2_rpn_loss_level: separate maps (B, HW, A, LPo, LPd), fused maps (B, HW, LPo) with A = 3
# ----------------------------------------------------------------------------------------------------------------------------
RPN_SEPARATE = [(1, 1, 1, 8, 16), (3, 255, 2, 8, 16), (2, 257, 3, 8, 16), (2, 64, 4, 8, 16), (2, 257, 3, 16, 32)]
RPN_FUSED = [(2, 257, 16), (1, 1, 32), (3, 255, 40)]
RPN_CASES = [(b, hw, a, lpo, lpd, False) for (b, hw, a, lpo, lpd) in RPN_SEPARATE]      # (B, HW, A, LPo, LPd, fused)
RPN_CASES += [(b, hw, 3, lpo, 0, True) for (b, hw, lpo) in RPN_FUSED]
RPN_FIRST_HW = 5          # positions of the level in front: lvl_off = 5 A


def rpn_grid(b, hw):
    return min(2048, -(-b * hw // 256))


def rpn_case(b, hw, a, lpo, lpd, fused):
    """One level, launched as the second of two.  Returns a dict: obj bf16 [b, hw, lpo] (fused: objectness in columns 0-2, deltas
    in 3-14), dlt bf16 [b, hw, lpd] or None, labels int8 / match int32 [b, atot], gt fp32 [b, G, 4], anchors fp32 [hw a, 4],
    lvl_off, atot, G (1 or 5) and ties: the number of delta elements tied by construction (an anchor equal to its gt box with
    zero deltas: 4 where G = 5 and image 0 has room for it).  The labels of the level in front are all 1: a launch that forgot
    lvl_off would count them.  With b >= 2 the last image has no positive (b = 2 and hw odd: no label at all); with b = 3 image
    1 has no positive and image 2 no label.  Pad columns hold PAD."""
    g = torch.Generator().manual_seed(hw * 100 + a * 10 + b + lpo)
    off = RPN_FIRST_HW * a
    atot = off + hw * a
    n_gt = 5 if (lpo != 8 or a == 2) else 1
    lab = torch.multinomial(torch.tensor([0.5, 0.3, 0.2]), b * hw * a, replacement=True, generator=g).view(b, hw * a) - 1
    if hw * a <= 4:
        lab = (torch.tensor([1, 0, -1, 1])[: hw * a])[None].repeat(b, 1)
    if b == 3:
        lab[1] = lab[1].clamp_max(0)
        lab[2] = -1
    elif b == 2:
        lab[1] = -1 if hw % 2 else lab[1].clamp_max(0)
    match = torch.randint(0, n_gt, (b, hw * a), generator=g)
    xy = torch.rand((hw * a, 2), generator=g) * 80
    anchors = torch.cat([xy, xy + 8 + torch.rand((hw * a, 2), generator=g) * 40], 1)
    gxy = torch.rand((b, n_gt, 2), generator=g) * 80
    gt = torch.cat([gxy, gxy + 6 + torch.rand((b, n_gt, 2), generator=g) * 50], 2)
    m = torch.randn((b, hw, 15), generator=g)
    m[..., :a] *= torch.where(torch.rand((b, hw, 1), generator=g) < 0.1, 12.0, 2.0)
    ties = 0
    if n_gt == 5 and hw * a > 4:
        lab[0, 0], match[0, 0], gt[0, 4] = 1, 4, anchors[0]
        ties = 4
    labels = torch.cat([torch.ones((b, off), dtype=torch.long), lab], 1).to(torch.int8)
    matches = torch.cat([torch.zeros((b, off), dtype=torch.long), match], 1).to(torch.int32)
    if fused:
        obj = torch.full((b, hw, lpo), PAD)
        obj[..., :15] = m
        if ties:
            obj[0, 0, 3:7] = 0
        dlt = None
    else:
        obj = torch.full((b, hw, lpo), PAD)
        obj[..., :a] = m[..., :a]
        dlt = torch.full((b, hw, lpd), PAD)
        dlt[..., : 4 * a] = torch.randn((b, hw, 4 * a), generator=g)
        if ties:
            dlt[0, 0, :4] = 0
        dlt = dlt.to(BF16)
    return dict(obj=obj.to(BF16), dlt=dlt, labels=labels, match=matches, gt=gt.float(), anchors=anchors.float(), lvl_off=off,
                atot=atot, G=n_gt, ties=ties, a=a)


def rpn_views(c):
    """(objectness [b, hw, a], deltas [b, hw, 4 a], labels / match of the level [b, hw a]) of a case."""
    a = c["a"]
    lab, mt = c["labels"][:, c["lvl_off"]:], c["match"][:, c["lvl_off"]:]
    if c["dlt"] is None:
        return c["obj"][..., :a], c["obj"][..., a: 5 * a], lab, mt
    return c["obj"][..., :a], c["dlt"][..., : 4 * a], lab, mt


# ----------------------------------------------------------------------------------------------------------------------------
# u2_box_reg_l1: (R, LP, every row background)
# ----------------------------------------------------------------------------------------------------------------------------
BOX_CASES = [(1, 8, False), (255, 32, False), (257, 32, False), (300, 8, True)]
BOX_WEIGHTS = [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)]   # the three cascade stages
BOX_BG = 80
BOX_TIED_ROWS = 8       # rows 0-7: proposal == gt and prediction 0 (the difference is exactly 0); rows 8-15: pred = bf16(target)


def box_grid(r):
    return min(1024, -(-r // 256))


def box_case(r, lp, all_bg, weights):
    """pred bf16 [r, lp] (columns 4 .. hold PAD), proposals / gt fp32 [r, 4], labels int64 [r] (25 % foreground), and the number
    of elements tied by construction (4 per foreground row with proposal == gt and prediction 0)."""
    g = torch.Generator().manual_seed(r * 10 + lp + int(weights[0]))
    xy = torch.rand((r, 2), generator=g) * torch.tensor([1300.0, 780.0])
    wh = 2 + torch.rand((r, 2), generator=g) ** 2 * 500
    prop = torch.cat([xy, xy + wh], 1)
    gt = prop + torch.randn((r, 4), generator=g) * wh.repeat(1, 2) * 0.1
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    lab = torch.where(torch.rand(r, generator=g) < 0.25, torch.randint(0, BOX_BG, (r,), generator=g), torch.full((r,), BOX_BG))
    pred = torch.randn((r, lp), generator=g)
    pred[:, 4:] = PAD
    ties = 0
    if all_bg:
        lab[:] = BOX_BG
    elif r >= 2 * BOX_TIED_ROWS:
        k = BOX_TIED_ROWS
        gt[:k] = prop[:k]
        lab[: 2 * k] = 3
        pred[:k, :4] = 0
        prop[k: 2 * k, :2] = torch.rand((k, 2), generator=g) * 40          # large boxes near the origin: get_deltas' fp32 error
        prop[k: 2 * k, 2:] = prop[k: 2 * k, :2] + 100 + torch.rand((k, 2), generator=g) * 200   # is far below a bf16 step there
        size = prop[k: 2 * k, 2:] - prop[k: 2 * k, :2]                       # and every target is of order 1: no small bf16 step
        ctr = prop[k: 2 * k, :2] + 0.5 * size + size * (0.1 + 0.2 * torch.rand((k, 2), generator=g))
        half = 0.5 * size * (1.4 + 0.6 * torch.rand((k, 2), generator=g))
        gt[k: 2 * k] = torch.cat([ctr - half, ctr + half], 1)
        pred[k: 2 * k, :4] = get_deltas(prop[k: 2 * k].to(F64), gt[k: 2 * k].to(F64), weights).float()
        ties = 4 * k
    else:
        lab[:] = 3
    return pred.to(BF16), prop, gt, lab, ties
