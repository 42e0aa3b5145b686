"""DINO ViT feature extraction for stage 1 of the pipeline (u2seg/Instance_Clustering/selective_labeling/dino.py:77-308,
usl-imagenet.py:44-63 and shared/utils/nn_utils.py:155-199).

``DinoViT`` holds the reference's parameters under the reference's state-dict names, so the official
``dino_vitbase8_pretrain.pth`` loads with ``strict=True``.  ``extract`` runs ``ViTFeat.forward`` (dino.py:296-308): the
768-d CLS token after the final LayerNorm.  The hot path is HIP (u2seg_amd/csrc/vit.hip): patchify, embedding,
residual + LayerNorm, flash-style attention and GELU, with the linears on u2_conv_igemm.  Precision: bf16 GEMM / attention
operands with fp32 accumulation, fp32 residual stream, LayerNorm statistics, softmax and biases, fp32 output.

The last block runs for the CLS queries only: its K and V still need every token's qkv, but the attention, proj, LayerNorm
and MLP of the other T - 1 rows cannot reach row 0, so they are skipped (exact for the returned feature)."""
import math
from functools import partial

import torch
import torch.nn as nn

from .. import _hip
from ..layers import functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
BF16 = torch.bfloat16


class _Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = _Attention(dim, num_heads, qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) * (img_size // patch_size)
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class DinoViT(nn.Module):
    """dino.py:162-200 (VisionTransformer with num_classes=0): parameters only; the forward is ``extract``."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.,
                 qkv_bias=False, norm_layer=nn.LayerNorm):
        super().__init__()
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise ValueError("DinoViT: the attention kernel serves head dim 64 only (got %d / %d)" % (embed_dim, num_heads))
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.reset_parameters()
        self._pos_cache = {}
        self._ws = {}

    def reset_parameters(self):
        """The reference's initialisation (dino.py:190-200): truncated normal(std 0.02) for pos_embed, cls_token and every
        Linear weight, zero Linear biases, LayerNorm (1, 0); the patch Conv2d keeps torch's default."""
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    # -- positional embedding -------------------------------------------------------------------------------------------
    def interpolate_pos_encoding(self, npatch, w, h):
        """dino.py:202-222 for an input of w x h pixels (the reference's naming: w is the size of dim 2, h of dim 3):
        [1, 1 + npatch, D].  Cached per (w, h) until the parameters change."""
        key = (w, h, self.pos_embed._version, self.pos_embed.data_ptr(), self.pos_embed.device)
        hit = self._pos_cache.get((w, h))
        if hit is not None and hit[0] == key:
            return hit[1]
        with torch.no_grad():
            pos = self.pos_embed.detach()
            N = pos.shape[1] - 1
            if npatch == N and w == h:
                out = pos
            else:
                class_pos_embed = pos[:, 0]
                patch_pos_embed = pos[:, 1:]
                dim = pos.shape[-1]
                w0 = w // self.patch_embed.patch_size
                h0 = h // self.patch_embed.patch_size
                w0, h0 = w0 + 0.1, h0 + 0.1
                patch_pos_embed = nn.functional.interpolate(
                    patch_pos_embed.reshape(1, int(math.sqrt(N)), int(math.sqrt(N)), dim).permute(0, 3, 1, 2),
                    scale_factor=(w0 / math.sqrt(N), h0 / math.sqrt(N)),
                    mode="bicubic",
                )
                assert int(w0) == patch_pos_embed.shape[-2] and int(h0) == patch_pos_embed.shape[-1]
                patch_pos_embed = patch_pos_embed.permute(0, 2, 3, 1).reshape(1, -1, dim)
                out = torch.cat((class_pos_embed.unsqueeze(0), patch_pos_embed), dim=1)
            out = out.float().contiguous()
        self._pos_cache[(w, h)] = (key, out)
        return out

    # -- forward --------------------------------------------------------------------------------------------------------
    def _workspace(self, B, T, device):
        key = (B, T, device)
        ws = self._ws.get(key)
        if ws is None:
            D = self.embed_dim
            self._ws = {}  # one shape at a time: a new (B, T) releases the previous buffers
            ws = self._ws[key] = {
                "x": torch.empty((B, T, D), dtype=torch.float32, device=device),
                "ln": torch.empty((B * T, D), dtype=BF16, device=device),
                "att": torch.empty((B * T, D), dtype=BF16, device=device),
                "feat_ln": torch.empty((B, D), dtype=BF16, device=device),
            }
        return ws

    def _norm_const(self, device):
        t = self._ws.get(("norm", device))
        if t is None:
            t = self._ws[("norm", device)] = torch.tensor(IMAGENET_MEAN + IMAGENET_STD, dtype=torch.float32, device=device)
        return t

    def _linear(self, x2d, lin, bias=True):
        """bf16 [R, K] -> bf16 [R, N] through u2_conv_igemm; `bias`: the fp32 bias goes into the epilogue unrounded."""
        r, k = x2d.shape
        n = lin.weight.shape[0]
        out = F.conv2d(x2d.view(1, r, 1, k), lin.weight.view(n, k, 1, 1), lin.bias if bias else None, param=lin.weight,
                       round_bias=False)
        return out.view(r, -1)

    @torch.no_grad()
    def extract(self, images):
        """images: uint8 NHWC RGB [B, H, W, 3] (ToTensor + ImageNet Normalize applied here) or fp32 NCHW [B, 3, H, W] already
        normalised.  Returns the fp32 CLS feature after the final norm, [B, D], on the device."""
        device = self.cls_token.device
        assert device.type == "cuda", "DinoViT.extract runs on the GPU (move the module with .cuda())"
        images = images.to(device)
        if images.dtype == torch.uint8:
            assert images.dim() == 4 and images.shape[3] == 3, "uint8 input must be NHWC RGB"
            B, H, W = images.shape[0], images.shape[1], images.shape[2]
            in_u8 = 1
            norm = self._norm_const(device)
        else:
            assert images.dim() == 4 and images.shape[1] == 3, "float input must be NCHW with 3 channels"
            images = images.float()
            B, H, W = images.shape[0], images.shape[2], images.shape[3]
            in_u8 = 0
            norm = None
        images = images.contiguous()
        p = self.patch_embed.patch_size
        D, heads = self.embed_dim, self.num_heads
        P = (H // p) * (W // p)
        T = P + 1
        pos = self.interpolate_pos_encoding(P, H, W)
        ws = self._workspace(B, T, device)
        x, ln, att = ws["x"], ws["ln"], ws["att"]

        patches = torch.empty((B * P, 3 * p * p), dtype=BF16, device=device)
        _hip.call("u2_vit_patchify", images, norm, patches, B, H, W, 3, p, in_u8)
        pe = self.patch_embed.proj
        g = self._linear(patches, pe, bias=False)
        _hip.call("u2_vit_embed", g, g.shape[1], pe.bias.detach().float().contiguous(), self.cls_token.detach().float().contiguous(),
                  pos, x, B, T, D)
        del patches, g

        nb = len(self.blocks)
        b0 = self.blocks[0]
        _hip.call("u2_vit_residual_layernorm", x, D, None, 0, None, b0.norm1.weight, b0.norm1.bias, ln, D, 0, B * T, D,
                  float(b0.norm1.eps))
        for i, blk in enumerate(self.blocks):
            last = i == nb - 1
            qkv = self._linear(ln, blk.attn.qkv)
            q_rows = 1 if last else T
            _hip.call("u2_vit_attention", qkv, att, B, T, heads, 64, qkv.shape[1], q_rows)
            del qkv
            rows = B if last else B * T
            xs = T * D if last else D  # the last block touches only the CLS rows of the residual
            a_in = att[:rows]
            lnr = ws["feat_ln"] if last else ln
            y = self._linear(a_in, blk.attn.proj, bias=False)
            _hip.call("u2_vit_residual_layernorm", x, xs, y, y.shape[1], blk.attn.proj.bias, blk.norm2.weight, blk.norm2.bias,
                      lnr, D, 0, rows, D, float(blk.norm2.eps))
            h1 = self._linear(lnr, blk.mlp.fc1)
            _hip.call("u2_vit_gelu", h1, h1.numel())
            y = self._linear(h1, blk.mlp.fc2, bias=False)
            del h1
            if last:
                feats = torch.empty((B, D), dtype=torch.float32, device=device)
                _hip.call("u2_vit_residual_layernorm", x, xs, y, y.shape[1], blk.mlp.fc2.bias, self.norm.weight, self.norm.bias,
                          feats, D, 1, rows, D, float(self.norm.eps))
            else:
                nxt = self.blocks[i + 1].norm1
                _hip.call("u2_vit_residual_layernorm", x, xs, y, y.shape[1], blk.mlp.fc2.bias, nxt.weight, nxt.bias, ln, D, 0,
                          rows, D, float(nxt.eps))
        return feats

    def forward(self, images):
        return self.extract(images)


def vit_small(patch_size=16, **kwargs):
    """dino.py:264-269."""
    return DinoViT(patch_size=patch_size, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True,
                   norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def vit_base(patch_size=8, **kwargs):
    """dino.py:272-276 (patch 8: dino_config.ini's vit_arch = base, patch_size = 8)."""
    return DinoViT(patch_size=patch_size, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                   norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


def build_from_state_dict(state_dict):
    """A DinoViT shaped like the checkpoint: width from cls_token, depth from the block count, patch size from the patch
    Conv2d, img_size from pos_embed, MLP width from fc1, qkv_bias from its presence (heads: width / 64).  The official
    dino_vitbase8_pretrain.pth gives vit_base(patch_size=8)."""
    D = state_dict["cls_token"].shape[-1]
    depth = len({k.split(".")[1] for k in state_dict if k.startswith("blocks.")})
    patch = state_dict["patch_embed.proj.weight"].shape[-1]
    n = state_dict["pos_embed"].shape[1] - 1
    hidden = state_dict["blocks.0.mlp.fc1.weight"].shape[0]
    return DinoViT(img_size=int(round(math.sqrt(n))) * patch, patch_size=patch, embed_dim=D, depth=depth, num_heads=D // 64,
                   mlp_ratio=hidden / D, qkv_bias="blocks.0.attn.qkv.bias" in state_dict,
                   norm_layer=partial(nn.LayerNorm, eps=1e-6))


def load_dino_weights(path, model=None, device=None):
    """ViTFeat.__init__ (dino.py:277-295) with the checkpoint on a local path (the reference fetches it with torch.hub):
    strict loading into ``model`` (default: build_from_state_dict, vit_base(patch_size=8) for the official checkpoint).
    Returns the model in eval mode, moved to ``device`` if given."""
    state_dict = torch.load(path, map_location="cpu")
    if model is None:
        model = build_from_state_dict(state_dict)
    model.load_state_dict(state_dict, strict=True)
    if device is not None:
        model = model.to(device)
    return model.eval()


@torch.no_grad()
def get_feats_list(model, loader):
    """nn_utils.py:155-199: the features of every batch of ``loader`` in dataset order, fp32 [N, D], on the device.  A batch is
    an image tensor or a tuple whose first element is one (the reference's (images, targets) pairs)."""
    feats = []
    for batch in loader:
        images = batch[0] if isinstance(batch, (tuple, list)) else batch
        feats.append(model.extract(images))
    if not feats:
        return torch.empty((0, model.embed_dim), dtype=torch.float32, device=model.cls_token.device)
    return torch.cat(feats, dim=0)


@torch.no_grad()
def reference_forward(model, x, attn_chunk=None):
    """The reference's fp32 forward (VisionTransformer.forward, dino.py:108-142, 224-260) restated with plain torch ops on
    ``model``'s parameters, attention matrix materialised: the yardstick for the tests and tools/bench_dino.py, never part of
    ``extract``.  x: fp32 NCHW normalised.  ``attn_chunk``: images per attention matrix (memory), default all."""
    tf = torch.nn.functional
    B, _, w, h = x.shape
    pe = model.patch_embed.proj
    t = tf.conv2d(x, pe.weight, pe.bias, stride=model.patch_embed.patch_size).flatten(2).transpose(1, 2)
    t = torch.cat((model.cls_token.expand(B, -1, -1), t), dim=1)
    t = t + model.interpolate_pos_encoding(t.shape[1] - 1, w, h)
    H = model.num_heads
    for blk in model.blocks:
        y = tf.layer_norm(t, (t.shape[-1],), blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        N, C = y.shape[1], y.shape[2]
        qkv = tf.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias).reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        step = attn_chunk or B
        o = torch.empty_like(q)
        for i in range(0, B, step):
            a = (q[i:i + step] @ k[i:i + step].transpose(-2, -1)) * ((C // H) ** -0.5)
            o[i:i + step] = a.softmax(dim=-1) @ v[i:i + step]
            del a
        y = tf.linear(o.transpose(1, 2).reshape(B, N, C), blk.attn.proj.weight, blk.attn.proj.bias)
        t = t + y
        y = tf.layer_norm(t, (C,), blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        y = tf.linear(tf.gelu(tf.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias)), blk.mlp.fc2.weight, blk.mlp.fc2.bias)
        t = t + y
    t = tf.layer_norm(t, (t.shape[-1],), model.norm.weight, model.norm.bias, model.norm.eps)
    return t[:, 0]
