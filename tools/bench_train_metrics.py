#!/usr/bin/env python
"""What the training metrics cost.  GPU only: fails without a device.

  kernels   device-event times of u2_softmax_ce against u2_softmax_ce_stats (R = 8192, NC = 801, LP = 832) and of the loss-only
            u2_mask_predict_bce against u2_mask_predict_bce_stats (N = 260, P = 784), and of u2_count_labels_i8 on the training
            shape's anchor labels: per launch, median / min / max over the repetitions, each repetition a run of back-to-back
            launches between two events, the two forms alternating.
  step      the training step at the benchmark's shape (u2seg_R50_800, 16 synthetic 800 x 1333 images) without and with an
            active EventStorage, in alternating blocks inside one process; a block ends in a device synchronise, and a block
            with the storage includes the read-out and the one wait a period ends with.  `on_minus_off_ms` stands next to
            `off_spread_ms` (max - min of the blocks without storage): a difference inside that spread is not resolved.
  bench     (--bench-tree / --bench-parent: files holding the JSON line of `python bench.py --gpus 1 --steps 20 --warmup 5`
            from this tree and from its parent commit, run alternately on the same machine) both triples and whether this
            tree's median lies below the parent's lowest run.

    python tools/bench_train_metrics.py [--blocks 3] [--steps 10] [--out profiles/train_metrics.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
BF16 = torch.bfloat16


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "each": [round(x, 5) for x in v]}


def time_pair(forms, launches=200, reps=7):
    """forms: {name: callable launching once}.  -> {name: per-launch ms summary}; the forms alternate repetition by repetition."""
    for fn in forms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                fn()
            e.record()
            e.synchronize()
            out[name].append(s.elapsed_time(e) / launches)
    return {k: summary(v) for k, v in out.items()}


def bench_kernels():
    from u2seg_amd import _hip as H

    g = torch.Generator(device=DEV).manual_seed(0)
    res = {}
    r, nc, lp = 8192, 801, 832
    z = torch.randn((r, lp), generator=g, device=DEV).to(BF16)
    labels = torch.randint(0, nc, (r,), generator=g, device=DEV)
    d = torch.empty_like(z)
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(8, dtype=torch.int32, device=DEV)
    res["softmax_ce R=8192 NC=801 LP=832"] = time_pair({
        "u2_softmax_ce": lambda: H.call("u2_softmax_ce", z, labels, d, loss, r, nc, lp, 1.0 / r),
        "u2_softmax_ce_stats": lambda: H.call("u2_softmax_ce_stats", z, labels, d, loss, r, nc, lp, 1.0 / r, cnt, nc - 1)})
    n, p, c, k = 260, 784, 256, 800
    x = torch.randn((n, p, c), generator=g, device=DEV).to(BF16)
    w = torch.randn((k, c), generator=g, device=DEV) * 0.05
    b = torch.zeros(k, device=DEV)
    cls = torch.randint(0, k, (n,), generator=g, device=DEV)
    tgt = (torch.rand((n, p), generator=g, device=DEV) < 0.5).to(torch.uint8)
    res["mask_predict_bce forward N=260 P=784"] = time_pair({
        "u2_mask_predict_bce": lambda: H.call("u2_mask_predict_bce", x, w, b, cls, tgt, None, None, None, loss, None, n, p, c,
                                              1.0 / (n * p), 28, None),
        "u2_mask_predict_bce_stats": lambda: H.call("u2_mask_predict_bce_stats", x, w, b, cls, tgt, loss, cnt, n, p, c, 28)})
    a = 16 * 267069   # anchors of 16 images of 800 x 1344 over the five FPN levels, three per cell
    lab = torch.randint(-1, 2, (a,), generator=g, device=DEV).to(torch.int8)
    res["count_labels_i8 n=%d" % a] = time_pair({"u2_count_labels_i8": lambda: H.call("u2_count_labels_i8", lab, a, cnt)})
    return res


def bench_step(blocks, steps):
    from u2seg_amd.config import get_cfg
    from u2seg_amd.data import make_synthetic_batch
    from u2seg_amd.engine import SimpleTrainer
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer
    from u2seg_amd.utils.events import EventStorage
    import time

    batch = 16
    torch.manual_seed(1234)
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", DEV, "SOLVER.IMS_PER_BATCH", batch])
    model = build_model(cfg)
    model.train()
    opt = build_optimizer(cfg, model)
    trainer = SimpleTrainer(model, opt, build_lr_scheduler(cfg, opt))
    batches = [make_synthetic_batch(batch, start_index=i * batch, device=DEV) for i in range(2)]
    state = {"i": 0}

    def run(n, storage):
        """n steps of the loop of tools/train_net.py: every 20th iteration waits for the device (check_finite) and, with a
        storage, collects the period that was read out one step before; a block with a storage ends with the rest of its rows."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            it = state["i"] if storage is None else storage.iter   # (the storage counts the steps taken inside it)
            trainer.run_step(batches[state["i"] % 2])
            if it % 20 == 0:
                trainer.check_finite()
                if storage is not None:
                    trainer.collect_metrics(storage)
            state["i"] += 1
        if storage is not None:
            if trainer.metrics.pending is not None:
                trainer.collect_metrics(storage)
            trainer.flush_metrics()
            trainer.collect_metrics(storage)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    st_on = EventStorage(0)
    run(5, None)
    with st_on:
        run(5, st_on)
    off, on = [], []
    for _ in range(blocks):
        off.append(run(steps, None))
        with st_on:
            on.append(run(steps, st_on))
    trainer.check_finite()
    names = sorted(st_on.latest())
    return {"shape": "u2seg_R50_800, %d synthetic 800 x 1333 images per step, %d steps per block" % (batch, steps),
            "off_ms_per_step": summary(off), "on_ms_per_step": summary(on),
            "on_minus_off_ms": statistics.median(on) - statistics.median(off), "off_spread_ms": max(off) - min(off),
            "scalars_logged": len(names), "names": names}


def bench_lines(tree_files, parent_files):
    def value(path):
        for line in reversed(open(path).read().strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)["value"]
        raise ValueError("no JSON line in " + path)

    tree, parent = [value(p) for p in tree_files], [value(p) for p in parent_files]
    return {"command": "python bench.py --gpus 1 --steps 20 --warmup 5", "unit": "img/s", "order": "parent, tree, parent, tree, ...",
            "tree": tree, "parent": parent, "tree_median": statistics.median(tree), "parent_min": min(parent),
            "tree_median_not_below_parent_min": statistics.median(tree) >= min(parent)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--bench-tree", nargs="*", default=[])
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_metrics.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_metrics.py measures on the GPU"
    out = {"device": torch.cuda.get_device_name(0), "kernels_ms_per_launch": bench_kernels()}
    if not args.skip_step:
        out["step"] = bench_step(args.blocks, args.steps)
    if args.bench_tree and args.bench_parent:
        out["bench"] = bench_lines(args.bench_tree, args.bench_parent)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
