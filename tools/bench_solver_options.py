#!/usr/bin/env python
"""What the solver's options cost per optimizer step.  GPU only: fails without a device.

One flat arena of about the real model's size (44 M fp32 elements cut into 168 tensors of the sizes a ResNet-50 Panoptic-FPN has: a
few large weights, many small ones), seeded gradients, and per form one optimizer step:

  default            u2_sgd_clip_step: the L2 norm pass + the step (what the shipped configs run)
  no clipping        u2_sgd_clip_step with clip 0: the step alone
  value / L1 / inf   u2_sgd_step_opts with that clipping (value has no norm pass)
  L2 via opts        u2_sgd_step_opts in mode 2: the option kernel on the default's work
  nesterov, bias lr  u2_sgd_step_opts, L2 clipping, with that option
  torch ...          the torch definition on the same tensors: per-parameter clip_grad_norm_ / clip_grad_value_ as the
                     reference's clipper calls them, then torch.optim.SGD(foreach=True).step()

Per form: device-event time per step, median / min / max over the repetitions (each a run of back-to-back steps between two
events, the forms alternating), and the ratio of its median to the default pair's, timed in the same run.  No pass / fail
threshold: the file records what was measured.

    python tools/bench_solver_options.py [--calls 50] [--reps 7] [--torch-calls 3] [--out profiles/solver_options.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
CHUNK = 1 << 16


def tensor_sizes():
    """About 44 M elements in 168 tensors: 3x3 and 1x1 conv weights of the four ResNet stages, the FPN, the heads' two large
    linear layers, and a norm weight + bias (or a bias) per layer."""
    sizes = []
    for c, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for _ in range(blocks):
            sizes += [4 * c * c, c, c, 9 * c * c, c, c, 4 * c * c, 4 * c, 4 * c]
    sizes += [256 * 256 * 9, 256] * 8                      # FPN laterals / outputs, RPN, mask head convs
    sizes += [256 * 49 * 1024, 1024, 1024 * 1024, 1024]    # box head
    sizes += [1024 * 801, 801, 1024 * 3200, 3200]          # predictors
    return sizes


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "each": [round(x, 5) for x in v]}


def time_forms(forms, reps):
    """forms: {name: (fn, calls)}."""
    for fn, _ in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in forms}
    for _ in range(reps):
        for name, (fn, calls) in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(calls):
                fn()
            e.record()
            e.synchronize()
            out[name].append(s.elapsed_time(e) / calls)
    return {k: summary(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_options.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_solver_options.py measures on the GPU"
    from u2seg_amd import _hip

    _hip.load()
    sizes = tensor_sizes()
    total = sum(sizes)
    chunk_tensor, chunk_begin, chunk_len, first_chunk = [], [], [], []
    off = 0
    for t, n in enumerate(sizes):
        first_chunk.append(len(chunk_tensor))
        for s in range(0, n, CHUNK):
            chunk_tensor.append(t)
            chunk_begin.append(off + s)
            chunk_len.append(min(CHUNK, n - s))
        off += n
    first_chunk.append(len(chunk_tensor))
    n_chunks = len(chunk_tensor)
    ct = torch.tensor(chunk_tensor, dtype=torch.int32, device=DEV)
    cb = torch.tensor(chunk_begin, dtype=torch.int64, device=DEV)
    cl = torch.tensor(chunk_len, dtype=torch.int32, device=DEV)
    fc = torch.tensor(first_chunk, dtype=torch.int32, device=DEV)
    g0 = torch.Generator(device=DEV).manual_seed(0)
    p = torch.randn(total, generator=g0, device=DEV) * 0.05
    g = torch.randn(total, generator=g0, device=DEV) * 1e-3
    m = torch.zeros(total, device=DEV)
    wd = torch.tensor([1e-4 if n > 4096 else 0.0 for n in sizes], device=DEV)
    cls = torch.tensor([int(n <= 4096 and i % 2 == 1) for i, n in enumerate(sizes)], dtype=torch.int32, device=DEV)
    no_cls = torch.zeros_like(cls)
    partial = torch.zeros(n_chunks, device=DEV)
    lr, mom = 1e-4, 0.9   # a small rate: hundreds of steps must not drive the parameters anywhere

    def clip_step(clip):
        return lambda: _hip.call("u2_sgd_clip_step", p, g, m, ct, cb, cl, n_chunks, partial, fc, wd, lr, mom, clip, 1.0)

    def opts(mode, clip, nesterov=0, classes=no_cls, lr_bias=lr):
        return lambda: _hip.call("u2_sgd_step_opts", p, g, m, ct, cb, cl, n_chunks, partial, fc, wd, classes, lr, lr_bias, mom, nesterov,
                                 mode, clip, 1.0)

    # the torch definition on views of the same arenas
    views, off = [], 0
    for n in sizes:
        v = torch.nn.Parameter(p[off: off + n])
        v.grad = g[off: off + n]
        views.append(v)
        off += n
    sgd = torch.optim.SGD(views, lr=lr, momentum=mom, weight_decay=1e-4, foreach=True)

    def torch_step(clipper):
        def run():
            if clipper is not None:
                for v in views:
                    clipper(v)
            sgd.step()
        return run

    norm_clip = lambda nt: (lambda v: torch.nn.utils.clip_grad_norm_(v, 1.0, nt))
    forms = {
        "default (L2 clip, u2_sgd_clip_step)": (clip_step(1.0), args.calls),
        "no clipping (u2_sgd_clip_step)": (clip_step(0.0), args.calls),
        "value clip": (opts(1, 1e-3), args.calls),
        "L1 clip": (opts(3, 1.0), args.calls),
        "inf clip": (opts(4, 1.0), args.calls),
        "L2 clip via u2_sgd_step_opts": (opts(2, 1.0), args.calls),
        "L2 clip + nesterov": (opts(2, 1.0, nesterov=1), args.calls),
        "L2 clip + bias lr": (opts(2, 1.0, classes=cls, lr_bias=2 * lr), args.calls),
        "torch  SGD foreach, no clipping": (torch_step(None), args.torch_calls),
        "torch  L2 clip_grad_norm_ per parameter + SGD foreach": (torch_step(norm_clip(2.0)), args.torch_calls),
        "torch  clip_grad_value_ per parameter + SGD foreach": (torch_step(lambda v: torch.nn.utils.clip_grad_value_(v, 1e-3)),
                                                               args.torch_calls),
    }
    res = time_forms(forms, args.reps)
    base = res["default (L2 clip, u2_sgd_clip_step)"]["median"]
    for v in res.values():
        v["ratio_to_default"] = round(v["median"] / base, 4)
    out = {"device": torch.cuda.get_device_name(0),
           "shape": "%d elements in %d tensors, %d chunks of at most %d" % (total, len(sizes), n_chunks, CHUNK),
           "bytes_streamed_by_the_step": 20 * total, "bytes_streamed_by_a_norm_pass": 4 * total,
           "unit": "ms per optimizer step", "forms": res}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
