"""Training metrics on the device: the three counting entry points against counts made with torch on the same values (integer
comparisons are ==), the unchanged loss / gradient of the entry points they extend, the fixture the reference produced
(tests/golden/train_metrics_golden.*), and the ring that carries one row per step to the host once per period."""
import collections
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
BF16 = torch.bfloat16
SENTINEL = 1000   # counters start from it: the kernels add, they never store
# the narrowest model the kernels serve (tests/test_gpu_bookkeeping.py:WIDE_OPTS)
REDUCED = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 32, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64, "MODEL.RESNETS.WIDTH_PER_GROUP", 32,
           "MODEL.ROI_BOX_HEAD.FC_DIM", 64, "MODEL.ROI_MASK_HEAD.CONV_DIM", 256]


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


@pytest.fixture(scope="module")
def fixture_data():
    arrays = np.load(os.path.join(GOLDEN, "train_metrics_golden.npz"))
    with open(os.path.join(GOLDEN, "train_metrics_golden.json")) as f:
        return arrays, json.load(f)


def grid(shape, gen):
    """Multiples of 0.25 in [-2, 2]: exact in bf16, ties between columns are frequent."""
    return ((torch.randint(-8, 9, shape, generator=gen, device=DEV).float()) * 0.25).to(BF16)


def counters():
    return torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)


# ---- u2_softmax_ce_stats ------------------------------------------------------------------------
def cls_counts(z, labels, nc):
    """fast_rcnn.py:88-115's five numbers with torch.argmax on the valid columns."""
    pred = z[:, :nc].float().argmax(dim=1)
    bg = nc - 1
    fg = (labels >= 0) & (labels < bg)
    return [int(labels.numel()), int((pred == labels).sum()), int(fg.sum()), int((fg & (pred == labels)).sum()),
            int((fg & (pred == bg)).sum())]


def run_both(H, z, labels, nc, cnt):
    r, lp = z.shape
    out = []
    for name, extra in (("u2_softmax_ce", ()), ("u2_softmax_ce_stats", (cnt, nc - 1))):
        d = torch.full_like(z, 7.0)
        loss = torch.zeros(1, dtype=torch.float32, device=DEV)
        H.call(name, z, labels, d, loss, r, nc, lp, 1.0 / max(r, 1), *extra)
        out.append((d, loss))
    return out


def check_cls(H, z, labels, nc, want=None):
    r = z.shape[0]
    cnt = counters()
    (d0, l0), (d1, l1) = run_both(H, z, labels, nc, cnt)
    expect = cls_counts(z, labels, nc)
    if want is not None:
        assert expect == want
    assert (cnt[:5] - SENTINEL).tolist() == expect
    assert (cnt[5:] == SENTINEL).all()
    assert torch.equal(d0.view(torch.int16), d1.view(torch.int16))          # dlogits bit-equal
    # the same per-row terms, summed by fp32 atomics in another order
    assert abs(float(l1) - float(l0)) <= r * 2.0 ** -24 * abs(float(l0)), (float(l0), float(l1))
    run_both(H, z, labels, nc, cnt)                                          # counters accumulate
    assert (cnt[:5] - SENTINEL).tolist() == [2 * v for v in expect]
    H.call("u2_softmax_ce_stats", z, labels, d1, l1, 0, nc, z.shape[1], 1.0, cnt, nc - 1)   # R == 0: nothing is written
    assert (cnt[:5] - SENTINEL).tolist() == [2 * v for v in expect]
    return expect


@pytest.mark.parametrize("r,nc,lp", [(7, 801, 832), (1030, 301, 320), (5, 1100, 1104), (9, 12, 12)])
def test_softmax_ce_stats(H, r, nc, lp):
    """(7, 801, 832), (1030, 301, 320): the register path, R no multiple of 4, one and 258 work-groups; (5, 1100, 1104),
    (9, 12, 12): the general path by LP > 1024 and by LP % 8 != 0.  (A wave of the register path walks more than one row only
    beyond 2048 rows: test_softmax_ce_stats_row_loop.)"""
    gen = torch.Generator(device=DEV).manual_seed(r * 31 + nc)
    z = grid((r, lp), gen)
    z[:, nc:] = 100.0                                  # pad columns: they must not win
    bg = nc - 1
    z[0, :nc] = 0.5                                    # all equal: pred 0
    z[1, :nc], z[1, bg] = -1.0, 1.75                   # the background column wins
    z[2, :nc], z[2, 3], z[2, bg] = -2.0, 2.0, 2.0      # tie between column 3 and the background: 3
    z[3, :nc], z[3, bg - 1], z[3, bg] = -2.0, 1.0, 1.0  # tie between the last two columns
    z[4, :nc], z[4, min(nc - 2, 70)] = 0.0, 0.25       # a maximum beyond the first 64 columns where the row has them
    labels = torch.randint(0, nc, (r,), generator=gen, device=DEV)
    labels[::3] = bg
    labels[:5] = torch.tensor([bg, 5, 3, bg - 1, min(nc - 2, 70)], device=DEV)   # row 1: a false negative; rows 2-4: correct
    half = r // 2
    labels[half:half + 3] = z[half:half + 3, :nc].float().argmax(dim=1)   # rows classified correctly
    expect = check_cls(H, z, labels, nc)
    assert expect[0] == r and 0 < expect[2] < r and expect[3] >= 3 and expect[4] >= 1
    # one launch with no foreground at all
    none = check_cls(H, z, torch.full_like(labels, bg), nc)
    assert none[2:] == [0, 0, 0] and none[1] >= 1


def test_softmax_ce_stats_row_loop(H):
    """More rows than one pass of the grid (512 work-groups x 4 waves): every wave walks two or three rows."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    r, nc, lp = 4100, 13, 16
    z = grid((r, lp), gen)
    z[:, nc:] = 100.0
    labels = torch.randint(0, nc, (r,), generator=gen, device=DEV)
    check_cls(H, z, labels, nc)


@pytest.mark.parametrize("case", ["cls_mixed", "cls_no_fg", "cls_wide"])
def test_softmax_ce_stats_reproduces_the_reference_scalars(H, fixture_data, case):
    from u2seg_amd.engine.metrics import scalars_from_counters
    from u2seg_amd.utils.events import N_COUNTERS, STAGE_SLOTS

    arrays, want = fixture_data
    logits, labels = arrays[case + "_logits"], arrays[case + "_labels"]
    r, nc = logits.shape
    lp = (nc + 31) // 32 * 32
    z = torch.full((r, lp), 100.0, dtype=BF16, device=DEV)
    z[:, :nc] = torch.from_numpy(logits).to(DEV)
    assert torch.equal(z[:, :nc].float().cpu(), torch.from_numpy(logits))   # the fixture's values are exact in bf16
    expect = check_cls(H, z.contiguous(), torch.from_numpy(labels).to(DEV), nc)
    row = [0] * N_COUNTERS
    row[STAGE_SLOTS[0]:STAGE_SLOTS[0] + 5] = expect
    got = {k[len("stage0/"):]: v for k, v in scalars_from_counters(row, 1).items() if k.startswith("stage0/fast_rcnn")}
    assert got == want[case]


# ---- u2_mask_predict_bce_stats ------------------------------------------------------------------
def mask_counts(zk, tgt):
    on = tgt.reshape(zk.shape) != 0
    wrong = (zk.float() > 0) != on
    return [int((wrong & ~on).sum()), int((wrong & on).sum()), int(on.sum()), int(on.numel())]


def run_mask(H, x, w, b, cls, tgt, n, p, phased_side):
    """-> (the existing entry point's logits in pixel order and loss sum, the new one's loss sum and counters)."""
    zk = torch.empty((n, p), dtype=BF16, device=DEV)
    l0 = torch.zeros(1, dtype=torch.float32, device=DEV)
    H.call("u2_mask_predict_bce", x, w, b, cls, tgt, None, None, None, l0, zk, n, p, 256, 1.0 / (n * p), phased_side, None)
    cnt = counters()
    l1 = torch.zeros(1, dtype=torch.float32, device=DEV)
    H.call("u2_mask_predict_bce_stats", x, w, b, cls, tgt, l1, cnt, n, p, 256, phased_side)
    return zk, l0, l1, cnt


@pytest.mark.parametrize("phased", [False, True], ids=["plain", "phased"])
@pytest.mark.parametrize("n,side,k", [(3, 28, 5), (3, 14, 5), (2, 4, 1)])
def test_mask_predict_bce_stats(H, n, side, k, phased):
    """P = 784, 196, 16: the launcher's 8, 4 and 1 position slices per ROI."""
    gen = torch.Generator(device=DEV).manual_seed(side * 7 + n)
    p, c = side * side, 256
    x = grid((n, p, c), gen)
    w = torch.randn((k, c), generator=gen, device=DEV) * 0.05
    b = torch.randn(k, generator=gen, device=DEV) * 0.1
    cls = torch.randint(0, k, (n,), generator=gen, device=DEV)
    b[cls[0]] = 0.0
    x[0, ::5] = 0.0                                   # x = 0 and bias 0: z == 0 exactly, "predicted 0"
    tgt = (torch.rand((n, p), generator=gen, device=DEV) < 0.5).to(torch.uint8)
    tgt[-2] = 1                                       # a ROI whose target is all ones
    tgt[-1] = 0                                       # and one that is all zeros
    if n > 2:
        tgt[0, ::10] = 1                              # z == 0 on a positive: a false negative
    zk, l0, l1, cnt = run_mask(H, x, w, b, cls, tgt, n, p, side if phased else 0)
    assert int((zk[0].float() == 0).sum()) >= p // 5
    expect = mask_counts(zk, tgt)
    assert (cnt[:4] - SENTINEL).tolist() == expect and (cnt[4:] == SENTINEL).all()
    assert expect[3] == n * p and expect[0] > 0 and expect[1] > 0
    assert abs(float(l1) - float(l0)) <= n * p * 2.0 ** -24 * abs(float(l0)), (float(l0), float(l1))
    H.call("u2_mask_predict_bce_stats", x, w, b, cls, tgt, l1, cnt, n, p, 256, side if phased else 0)
    assert (cnt[:4] - SENTINEL).tolist() == [2 * v for v in expect]


def test_mask_predict_bce_stats_reproduces_the_reference_scalars(H, fixture_data):
    """The fixture's logits [B, K, M, M] as the first K channels of x and a one-hot predictor: z is the fixture's value."""
    from u2seg_amd.engine.metrics import scalars_from_counters
    from u2seg_amd.utils.events import MASK_SLOT, N_COUNTERS

    arrays, want = fixture_data
    logits = torch.from_numpy(arrays["mask_logits"])
    nb, k, m, _ = logits.shape
    p = m * m
    x = torch.zeros((nb, p, 256), dtype=BF16, device=DEV)
    x[:, :, :k] = logits.reshape(nb, k, p).permute(0, 2, 1).to(DEV)
    w = torch.zeros((k, 256), device=DEV)
    w[torch.arange(k), torch.arange(k)] = 1.0
    b = torch.zeros(k, device=DEV)
    cls = torch.from_numpy(arrays["mask_classes"]).to(DEV)
    tgt = torch.from_numpy(arrays["mask_targets"]).to(DEV).to(torch.uint8).reshape(nb, p).contiguous()
    zk, l0, l1, cnt = run_mask(H, x, w, b, cls, tgt, nb, p, 0)
    assert torch.equal(zk.float().cpu().reshape(nb, m, m), logits[torch.arange(nb), torch.from_numpy(arrays["mask_classes"])])
    row = [0] * N_COUNTERS
    row[MASK_SLOT:MASK_SLOT + 4] = (cnt[:4] - SENTINEL).tolist()
    got = {name: v for name, v in scalars_from_counters(row, 2).items() if name.startswith("mask_rcnn")}
    assert got == {name: v for name, v in want["mask"].items() if name != "loss"}


# ---- u2_count_labels_i8 -------------------------------------------------------------------------
@pytest.mark.parametrize("b,a,offset", [(2, 4099, 0), (1, 7, 0), (2, 4099, 3)])
def test_count_labels_i8(H, b, a, offset):
    """offset: the labels start 3 bytes behind a 16-byte boundary (the kernel reads whole vectors only between boundaries)."""
    gen = torch.Generator(device=DEV).manual_seed(a + offset)
    buf = torch.randint(-1, 2, (b * a + 64,), generator=gen, device=DEV).to(torch.int8)
    labels = buf[offset:offset + b * a]
    assert labels.is_contiguous() and labels.data_ptr() % 16 == offset
    cnt = counters()
    H.call("u2_count_labels_i8", labels, labels.numel(), cnt)
    expect = [int((labels == 1).sum()), int((labels == 0).sum())]
    assert (cnt[:2] - SENTINEL).tolist() == expect and (cnt[2:] == SENTINEL).all()
    H.call("u2_count_labels_i8", labels, labels.numel(), cnt)
    assert (cnt[:2] - SENTINEL).tolist() == [2 * v for v in expect]
    H.call("u2_count_labels_i8", labels, 0, cnt)
    assert (cnt[:2] - SENTINEL).tolist() == [2 * v for v in expect]


# ---- the ring, on a reduced model ---------------------------------------------------------------
def build_trainer():
    from u2seg_amd.config import get_cfg
    from u2seg_amd.engine import SimpleTrainer
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_optimizer

    cfg = get_cfg()
    cfg.merge_from_file(CFG)
    cfg.merge_from_list(["MODEL.DEVICE", DEV] + REDUCED)
    torch.manual_seed(0)
    model = build_model(cfg)
    model.train()
    return SimpleTrainer(model, build_optimizer(cfg, model))


def batch(i):
    from u2seg_amd.data import make_synthetic_batch

    return make_synthetic_batch(2, start_index=40 + 2 * i, height=256, width=320, device=DEV)


class Capture:
    """Records what the three hooks were given, through the functions of layers/functional.py they call."""

    def __init__(self, monkeypatch):
        from u2seg_amd.layers import functional as F

        self.cls, self.mask, self.rpn = [], [], []
        ce, bce, cnt = F.softmax_cross_entropy, F.mask_predict_bce_loss, F.count_labels_i8

        def softmax_cross_entropy(logits, labels, num_classes, counters=None):
            self.cls.append((logits.detach().clone(), labels.clone(), num_classes, counters is not None))
            return ce(logits, labels, num_classes, counters)

        def mask_predict_bce_loss(x, weight, bias, classes, target_u8, phased=False, counters=None):
            self.mask.append((x.detach().clone(), weight.detach().clone(), bias.detach().clone(), classes.clone(),
                              target_u8.clone(), phased, counters is not None))
            return bce(x, weight, bias, classes, target_u8, phased, counters)

        def count_labels_i8(labels, counters):
            self.rpn.append(labels.clone())
            return cnt(labels, counters)

        monkeypatch.setattr(F, "softmax_cross_entropy", softmax_cross_entropy)
        monkeypatch.setattr(F, "mask_predict_bce_loss", mask_predict_bce_loss)
        monkeypatch.setattr(F, "count_labels_i8", count_labels_i8)

    def take(self):
        out = (self.cls, self.mask, self.rpn)
        self.cls, self.mask, self.rpn = [], [], []
        return out


def expected_scalars(H, cls_calls, mask_calls, rpn_calls, images):
    """The reference's definitions (rpn.py:396-403, roi_heads.py:290-300, cascade_rcnn.py:243-255, fast_rcnn.py:88-115,
    mask_head.py:90-102) on what the step's hooks were given."""
    out = {}
    (labels,) = rpn_calls
    out["rpn/num_pos_anchors"] = int((labels == 1).sum()) / images
    out["rpn/num_neg_anchors"] = int((labels == 0).sum()) / images
    assert len(cls_calls) == 3
    for k, (z, gt, nc, with_counters) in enumerate(cls_calls):
        assert with_counters
        rows, acc, fg, fg_acc, fn = cls_counts(z, gt, nc)
        pre = "" if k == 0 else "stage%d/" % k
        out[pre + "roi_head/num_fg_samples"] = fg / images
        out[pre + "roi_head/num_bg_samples"] = (rows - fg) / images
        out["stage%d/fast_rcnn/cls_accuracy" % k] = acc / rows
        if fg > 0:
            out["stage%d/fast_rcnn/fg_cls_accuracy" % k] = fg_acc / fg
            out["stage%d/fast_rcnn/false_negative" % k] = fn / fg
    ((x, weight, bias, classes, tgt, phased, with_counters),) = mask_calls
    assert with_counters and phased
    n, side = x.shape[0], 2 * x.shape[1]
    p = side * side
    kk = weight.shape[0]
    zk = torch.empty((n, p), dtype=BF16, device=DEV)
    H.call("u2_mask_predict_bce", x.contiguous(), weight.reshape(kk, 256).float().contiguous(), bias.float().contiguous(),
           classes.contiguous(), tgt.contiguous(), None, None, None, None, zk, n, p, 256, 1.0, side, None)
    false_pos, false_neg, pos, total = mask_counts(zk, tgt)
    out["mask_rcnn/accuracy"] = 1 - (false_pos + false_neg) / max(total, 1.0)
    out["mask_rcnn/false_positive"] = false_pos / max(total - pos, 1.0)
    out["mask_rcnn/false_negative"] = false_neg / max(pos, 1.0)
    return out


def test_ring_three_steps_period_two(H, monkeypatch):
    """Steps 0 and 1 fill the two rows and are read out together; step 2 reuses step 0's row (zeroed behind step 1) and is
    read out by the flush.  Every scalar of every step equals the one recomputed from what the hooks were given."""
    from u2seg_amd.utils.events import EventStorage

    trainer = build_trainer()
    trainer.metrics_period = 2
    cap = Capture(monkeypatch)
    want, losses = {}, {}
    with EventStorage(0) as st:
        for it in range(3):
            trainer.data_time = 0.25 + it
            loss_dict = trainer.run_step(batch(it))
            want[it] = expected_scalars(H, *cap.take(), images=2)
            losses[it] = {k: float(v.detach()) for k, v in loss_dict.items()}
            assert st.iter == it + 1 and st.counters is None
            if it == 1:
                assert trainer.collect_metrics(st)
                assert all(i in (0, 1) for h in st.histories().values() for _, i in h.values())
        assert not trainer.collect_metrics(st)
        trainer.flush_metrics()
        assert trainer.collect_metrics(st)
    got = collections.defaultdict(dict)
    for name, h in st.histories().items():
        for value, it in h.values():
            assert it not in got[name], "a scalar is put once per iteration"
            got[name][it] = value
    host = {"total_loss", "lr", "time", "data_time"} | set(losses[0])
    for it in range(3):
        assert {n: v[it] for n, v in got.items() if it in v and n not in host} == want[it], it
        for name, value in losses[it].items():
            assert got[name][it] == value                       # the ring's loss row == the step's loss dict
        assert got["total_loss"][it] == sum(losses[it].values())
        assert got["data_time"][it] == 0.25 + it and got["lr"][it] == trainer.optimizer.lr
    assert sorted(got["time"]) == [1, 2] and all(v > 0 for v in got["time"].values())
    assert len(losses[0]) == 10
    full = set(want[0]) | set(want[1]) | set(want[2])
    assert len(full) >= 16 and {"mask_rcnn/accuracy", "rpn/num_pos_anchors", "stage2/roi_head/num_fg_samples"} <= full


def test_no_storage_no_stats_launches(H, monkeypatch):
    """Without an active EventStorage a step makes the calls it made before the metrics existed; inside one, the three hooks
    take the counting entry points."""
    from u2seg_amd.utils.events import EventStorage

    calls = collections.Counter()
    real = H.call

    def counting(name, *args):
        calls[name] += 1
        return real(name, *args)

    monkeypatch.setattr(H, "call", counting)
    trainer = build_trainer()
    trainer.run_step(batch(0))
    new = ("u2_softmax_ce_stats", "u2_mask_predict_bce_stats", "u2_count_labels_i8")
    assert all(calls[n] == 0 for n in new), calls
    assert calls["u2_softmax_ce"] == 3 and calls["u2_mask_predict_bce"] == 2      # (the mask head: forward and backward)
    assert trainer.metrics is None
    calls.clear()
    with EventStorage(0) as st:
        trainer.run_step(batch(1))
        trainer.flush_metrics()
        assert trainer.collect_metrics(st)
    assert calls["u2_softmax_ce_stats"] == 3 and calls["u2_mask_predict_bce_stats"] == 1 and calls["u2_count_labels_i8"] == 1
    assert calls["u2_softmax_ce"] == 0 and calls["u2_mask_predict_bce"] == 1      # (the backward launch)
    torch.cuda.synchronize()


def test_filling_the_ring_and_starting_the_readout_never_waits():
    """Twenty rows from tensors that already exist and the read-out copy, with torch set to raise on every synchronising call."""
    from u2seg_amd.engine.metrics import MetricsRing
    from u2seg_amd.utils.events import EventStorage

    names = ["loss_%d" % i for i in range(10)]
    rows = torch.rand((20, 10), device=DEV)
    add = torch.ones(5, dtype=torch.int32, device=DEV)
    ring = MetricsRing(DEV, period=20)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with EventStorage(0) as st:
            for it in range(20):
                ring.begin_step(st, it)
                st.counters[2:7] += add
                ring.end_step(st, rows[it], names, it, 0.02, 0.1, 0.01, 2)
                st.step()
            assert ring.pending is not None       # the copy was started behind row 19
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert ring.collect(st)
    assert st.history("loss_3").values() == [(float(rows[i, 3]), i) for i in range(20)]
    assert st.history("roi_head/num_fg_samples").values() == [(0.5, i) for i in range(20)]
