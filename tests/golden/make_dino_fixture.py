"""Generates tests/golden/dino_golden.npz / dino_golden.json by running the reference's DINO ViT
(u2seg/Instance_Clustering/selective_labeling/dino.py) on the CPU in fp32.  Runs only where the reference is checked out;
the outputs are committed and the tests read nothing else.

    python tests/golden/make_dino_fixture.py --reference PATH_TO_REFERENCE_ROOT

Contents:
  * a tiny VisionTransformer (D = 128, 2 heads of 64, depth 2, patch 8, qkv_bias, LayerNorm eps 1e-6) whose pos_embed is made
    for a 4 x 4 grid (img_size 32), so the 64 x 64 and 48 x 64 inputs go through interpolate_pos_encoding; its state dict;
  * parameters and inputs lie on the grids k / 1024 and k / 256 and are stored as the int16 k;
  * inputs (B = 2, fp32 NCHW) and the reference's CLS outputs (forward(): x[:, 0] after the final norm) for both sizes;
  * the interpolated positional embeddings of both sizes;
  * the state-dict names and shapes of vit_base(patch_size=8) (JSON)."""
import argparse
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((64, 64), (48, 64))
PSCALE = 1024.0  # parameters are k / PSCALE
XSCALE = 256.0   # inputs are k / XSCALE


def load_reference_dino(ref_root):
    path = os.path.join(ref_root, "u2seg", "Instance_Clustering", "selective_labeling", "dino.py")
    spec = importlib.util.spec_from_file_location("ref_dino", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    dino = load_reference_dino(args.reference)
    from functools import partial

    torch.manual_seed(0)
    model = dino.VisionTransformer(img_size=[32], patch_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
                                   qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    # non-trivial LayerNorm affine and biases, so that a swapped or dropped parameter shows
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias") or "norm" in name:
                p.add_(0.05 * torch.randn_like(p))
            # every parameter on the grid k / 1024 (|k| < 2^15): stored as int16 (the fixture stays under 1 MiB), and exact in
            # bf16 where |k| < 256, so weight rounding plays almost no part in the comparison
            p.copy_(torch.round(p * PSCALE) / PSCALE)
    model.eval()
    out = {"param_scale": np.float32(PSCALE), "input_scale": np.float32(XSCALE)}
    for name, t in model.state_dict().items():
        k = torch.round(t * PSCALE)
        assert k.abs().max() < 32768 and torch.equal(k / PSCALE, t)
        out["sd/" + name] = k.numpy().astype(np.int16)
    for (h, w) in SIZES:
        x = torch.round(torch.randn(2, 3, h, w) * XSCALE) / XSCALE
        with torch.no_grad():
            y = model(x)
            tok = model.patch_embed(x)
            tok = torch.cat((model.cls_token.expand(2, -1, -1), tok), dim=1)
            pos = model.interpolate_pos_encoding(tok, h, w)
        out["x_%dx%d" % (h, w)] = torch.round(x * XSCALE).numpy().astype(np.int16)
        out["y_%dx%d" % (h, w)] = y.numpy()
        out["pos_%dx%d" % (h, w)] = pos.numpy()
    np.savez_compressed(os.path.join(HERE, "dino_golden.npz"), **out)

    base = dino.vit_base(patch_size=8, num_classes=0)
    meta = {
        "tiny": {"img_size": 32, "patch_size": 8, "embed_dim": 128, "depth": 2, "num_heads": 2, "eps": 1e-6,
                 "sizes": [list(s) for s in SIZES], "keys": list(model.state_dict().keys())},
        "vit_base8": {k: list(v.shape) for k, v in base.state_dict().items()},
    }
    with open(os.path.join(HERE, "dino_golden.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote dino_golden.npz / dino_golden.json")


if __name__ == "__main__":
    main()
