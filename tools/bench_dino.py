#!/usr/bin/env python
"""Throughput of the DINO ViT-B/8 feature extractor (u2seg_amd/cluster/dino.py) at the stage-1 crop size, 480 x 480
(T = 3601 tokens), on cuda:0, random weights with the reference's initialisation, device events around each timed region.

For each batch size (default 8 and 16):
  crops_per_s             whole DinoViT.extract (uint8 NHWC in, fp32 CLS features out)
  attention_ms            the 12 attention launches of one forward (11 full, the last block's CLS-only one), replayed alone
  attention_tflops        4 B H T^2 64 / t of one full launch
  linears_ms              patch-embed + the 48 linears of one forward (the last block's proj / fc1 / fc2 on B rows), replayed
  other_ms                forward - attention - linears: patchify, embed, residual + LayerNorm, GELU, host work
  forward_tflops          model FLOPs of one forward / t, against the 2.5 PF dense-bf16 peak
  reference_fp32_ms       the same forward as the reference computes it (fp32 torch ops, attention matrix materialised,
                          dino.reference_forward), at --ref-batch images, per crop
usage: python tools/bench_dino.py [--batches 8,16] [--iters 5] [--warmup 2] [--ref-batch 2]   (one JSON line per batch size)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from u2seg_amd import _hip  # noqa: E402
from u2seg_amd.cluster import dino  # noqa: E402

PEAK_TFLOPS = 2500.0


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def model_flops(B, T, D, depth, hidden, patch):
    """Multiply-adds x 2 of one forward with the last block on the CLS rows only (what extract computes)."""
    P = T - 1
    f = 2.0 * B * P * 3 * patch * patch * D
    full = 2.0 * B * T * (3 * D * D + D * D + 2 * D * hidden) + 4.0 * B * T * T * D
    last = 2.0 * B * T * 3 * D * D + 4.0 * B * T * D + 2.0 * B * (D * D + 2 * D * hidden)
    return f + (depth - 1) * full + last


def bench(model, B, size, iters, warmup, ref_batch):
    dev = model.cls_token.device
    D, H, depth = model.embed_dim, model.num_heads, len(model.blocks)
    p = model.patch_embed.patch_size
    T = (size // p) ** 2 + 1
    hidden = model.blocks[0].mlp.fc1.weight.shape[0]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    imgs = torch.randint(0, 256, (B, size, size, 3), dtype=torch.uint8, device=dev, generator=g)
    for _ in range(warmup):
        model.extract(imgs)
    fwd = timed(lambda: model.extract(imgs), iters)

    qkv = torch.randn((B * T, 3 * D), device=dev, generator=g).bfloat16()
    out = torch.empty((B * T, D), dtype=torch.bfloat16, device=dev)
    att_full = timed(lambda: _hip.call("u2_vit_attention", qkv, out, B, T, H, 64, 3 * D, T), iters * 2)
    att_cls = timed(lambda: _hip.call("u2_vit_attention", qkv, out, B, T, H, 64, 3 * D, 1), iters * 2)
    attention = (depth - 1) * att_full + att_cls

    blk = model.blocks[0]
    a = torch.randn((B * T, D), device=dev, generator=g).bfloat16()
    h = torch.randn((B * T, hidden), device=dev, generator=g).bfloat16()
    pt = torch.randn(((T - 1) * B, 3 * p * p), device=dev, generator=g).bfloat16()

    def lin(rows):
        model._linear(a[:rows], blk.attn.qkv)
        model._linear(a[:rows], blk.attn.proj, bias=False)
        model._linear(a[:rows], blk.mlp.fc1)
        model._linear(h[:rows], blk.mlp.fc2, bias=False)

    full_l = timed(lambda: lin(B * T), iters)
    cls_l = timed(lambda: (model._linear(a, blk.attn.qkv), model._linear(a[:B], blk.attn.proj, bias=False),
                           model._linear(a[:B], blk.mlp.fc1), model._linear(h[:B], blk.mlp.fc2, bias=False)), iters)
    pe_l = timed(lambda: model._linear(pt, model.patch_embed.proj, bias=False), iters)
    linears = (depth - 1) * full_l + cls_l + pe_l
    del qkv, out, a, h, pt

    flops = model_flops(B, T, D, depth, hidden, p)
    res = {
        "workload": "dino_vitb8_extract", "batch": B, "image": size, "tokens": T,
        "forward_ms": round(fwd, 3), "crops_per_s": round(B / fwd * 1e3, 2),
        "attention_ms": round(attention, 3), "attention_full_launch_ms": round(att_full, 3),
        "attention_tflops": round(4.0 * B * H * T * T * 64 / (att_full * 1e-3) / 1e12, 1),
        "linears_ms": round(linears, 3), "other_ms": round(fwd - attention - linears, 3),
        "forward_tflops": round(flops / (fwd * 1e-3) / 1e12, 1),
        "forward_fraction_of_peak": round(flops / (fwd * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
    }
    if ref_batch > 0:
        torch.backends.cuda.matmul.allow_tf32 = False
        mean = torch.tensor(dino.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
        std = torch.tensor(dino.IMAGENET_STD, device=dev).view(1, 3, 1, 1)
        x = ((imgs[:ref_batch].permute(0, 3, 1, 2).float() / 255.0) - mean) / std
        dino.reference_forward(model, x)
        ref = timed(lambda: dino.reference_forward(model, x), max(1, iters // 2))
        res["reference_fp32_batch"] = ref_batch
        res["reference_fp32_ms_per_crop"] = round(ref / ref_batch, 3)
        res["speedup_vs_reference_fp32"] = round((ref / ref_batch) / (fwd / B), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-batch", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dino needs cuda:0"
    _hip.load()
    torch.manual_seed(0)
    model = dino.vit_base(patch_size=8).cuda().eval()
    for b in (int(v) for v in args.batches.split(",")):
        print(json.dumps(bench(model, b, args.size, args.iters, args.warmup, args.ref_batch)), flush=True)


if __name__ == "__main__":
    main()
