"""Fixtures of RESNETS.NUM_GROUPS (ResNeXt), written from the reference (imported through make_fixtures.py's stand-ins).

  resnext_golden.json       the ordered state-dict keys with their shapes and the parameter count of the reference's model under
                            the reduced ResNeXt configuration (OPTS below: stage widths 32 / 64 / 128 / 256 in 4 groups, so
                            8 / 16 / 32 / 64 channels per group).
  resnext_block_golden.npz  fp32 CPU known answers of the reference's BottleneckBlock(num_groups=4): a projection-shortcut stride-2
                            block (32 -> 64, bottleneck 32) and an identity-shortcut block (64 -> 64, bottleneck 32) on a
                            2 x 12 x 20 input, with norm="FrozenBN" (non-trivial buffers, one negative weight per norm; keys
                            "frozen.<block>..."): output, and the gradients w.r.t. the input and the conv weights for a recorded output gradient.
                            Every block obeys the seed-rejection rule of make_freeze_fixture.py: no ReLU input within its fp32
                            bound of zero (tests/grouped_conv_refs.py block_chain); see gen_block for what makes that possible.

  resnext_block_bn_proj_golden.npz, resnext_block_bn_ident_golden.npz
                            the same two blocks with norm="BN" in training mode (keys "bn.<block>..."): output, dx, every conv's
                            dweight, and the reference's intermediates (gen_bn_block), one file per block.

All files hold data only.  Run: python tests/golden/make_resnext_fixture.py"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as MF  # noqa: E402
from make_freeze_fixture import import_reference_light  # noqa: E402
from tests import grouped_conv_refs as G  # noqa: E402  (this repository's tests package: before the reference joins sys.path)

OPTS = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 32, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64, "MODEL.RESNETS.NUM_GROUPS", 4,
        "MODEL.RESNETS.WIDTH_PER_GROUP", 8]


def gen_model_fixture():
    os.environ.setdefault("CLUSTER_NUM", "800")
    from detectron2.config import get_cfg
    from detectron2.modeling import build_model

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(MF.REF, "configs/COCO-PanopticSegmentation/u2seg_R50_800.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHTS", ""] + OPTS)
    model = build_model(cfg)
    sd = model.state_dict()
    with open(os.path.join(HERE, "resnext_golden.json"), "w") as f:
        f.write('{"opts": %s,\n"num_params": %d,\n"state_dict": [\n' % (json.dumps(OPTS), sum(p.numel() for p in model.parameters())))
        f.write(",\n".join(" " + json.dumps([k, list(v.shape)]) for k, v in sd.items()))
        f.write("\n]}\n")
    print("model:", len(sd), "entries")


MARGIN = {"conv1": 5.0, "conv2": 5.0, "conv3": 8.0, "shortcut": 0.0}


def _signs(c, g):
    """+1 for three channels in four: most ReLUs are on, some channels are off."""
    return torch.where(torch.rand(c, generator=g) < 0.75, 1.0, -1.0)


def gen_block(out, kind, name, seed):
    """One block and its known answers under the keys "<kind>.<name>....".  The norms' shifts put every channel's values
    MARGIN standard deviations away from zero (conv3 further, the shortcut not at all: the tail's ReLU sees their sum), on either
    side: with zero-mean pre-activations a block of this size always has ReLU inputs inside the chain's fp32 bound, and no
    seed would pass the rejection rule (600 were tried).  The shifts are set layer by layer from the values the layer's
    norm receives."""
    from detectron2.modeling.backbone.resnet import BottleneckBlock

    cin, cout, cb, stride = G.BLOCKS[name]
    pre = "%s.%s" % (kind, name)
    g = torch.Generator().manual_seed(sum(map(ord, pre)) + seed)
    blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, num_groups=G.BLOCK_GROUPS,
                          norm="FrozenBN")
    blk.train()
    convs = [("conv1", blk.conv1), ("conv2", blk.conv2), ("conv3", blk.conv3)]
    if blk.shortcut is not None:
        convs.append(("shortcut", blk.shortcut))
    x = torch.randn(2, cin, 12, 20, generator=g).requires_grad_(True)
    for cname, conv in convs:
        n = conv.norm
        c = n.num_features
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / conv.weight[0].numel()) ** 0.5)
            n.weight.copy_(0.5 + torch.rand(c, generator=g))
            n.weight[c // 3] *= -1.0
            sign = _signs(c, g)
            n.running_mean.copy_(0.2 * torch.randn(c, generator=g))
            n.running_var.copy_(0.5 + torch.rand(c, generator=g))
            seen = []
            handle = n.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach()))
            blk(x.detach())
            handle.remove()
            y = seen[0]
            s = n.weight * (n.running_var + n.eps).rsqrt()
            n.bias.copy_(MARGIN[cname] * sign * s.abs() * y.std((0, 2, 3)) - s * (y.mean((0, 2, 3)) - n.running_mean)
                         + 0.3 * torch.randn(c, generator=g))
        conv.weight.requires_grad_(True)
    for cname, conv in convs:
        n = conv.norm
        for key in ("weight", "bias", "running_mean", "running_var"):
            out["%s.%s.norm.%s" % (pre, cname, key)] = getattr(n, key).detach().numpy().copy()
        out["%s.%s.norm.eps" % (pre, cname)] = np.float64(n.eps)
        out["%s.%s.weight" % (pre, cname)] = conv.weight.detach().numpy().copy()
    y = blk(x)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    out[pre + ".x"], out[pre + ".gy"], out[pre + ".y"] = x.detach().numpy().copy(), gy.numpy().copy(), y.detach().numpy().copy()
    out[pre + ".dx"] = x.grad.numpy().copy()
    for cname, conv in convs:
        out["%s.%s.dweight" % (pre, cname)] = conv.weight.grad.numpy().copy()
    return x, gy, y


def gen_block_fixture():
    out = {}
    for kind in ("frozen",):
        for name in G.BLOCKS:
            pre = "%s.%s" % (kind, name)
            for seed in range(200):
                x, gy, y = gen_block(out, kind, name, seed)
                try:   # the host test's precondition: no ReLU input within the fp32 error of zero (else: the next seed)
                    G.block_chain(G.block_layers(out, name), x.detach().double(), gy.double())
                except AssertionError as e:
                    print(pre, "seed", seed, "rejected:", e)
                    for k in [k for k in out if k.startswith(pre + ".")]:
                        del out[k]
                    continue
                print(pre, "seed", seed, tuple(y.shape), float(y.detach().abs().mean()), float(np.abs(out[pre + ".dx"]).mean()),
                      "share of y > 0: %.2f" % float((y > 0).float().mean()))
                break
            assert pre + ".y" in out, pre
    np.savez_compressed(os.path.join(HERE, "resnext_block_golden.npz"), **out)


def gen_bn_block(name, seed=0):
    """One block with norm="BN" in training mode: the known answers and the reference's intermediates, so that every layer can
    be held on its own recorded input and output gradient (tests/grouped_conv_refs.py).  Per conv: weight, the norm's affine pair
    and eps, dweight; `o`, the norm's output in front of the ReLU (conv1, conv2, shortcut; conv3's goes into y), `g`, the
    gradient of that output (conv1, conv2; conv3's and the shortcut's is gy [y > 0]), `dxin`, the gradient of the layer's
    input (conv2, conv3; the block input's is dx).  A layer's input is x or the ReLU of the previous `o`."""
    from detectron2.modeling.backbone.resnet import BottleneckBlock

    cin, cout, cb, stride = G.BLOCKS[name]
    pre = "bn.%s" % name
    g = torch.Generator().manual_seed(sum(map(ord, pre)) + seed)
    blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, num_groups=G.BLOCK_GROUPS, norm="BN")
    blk.train()
    convs = [("conv1", blk.conv1), ("conv2", blk.conv2), ("conv3", blk.conv3)]
    if blk.shortcut is not None:
        convs.append(("shortcut", blk.shortcut))
    out, rec = {}, {}
    for cname, conv in convs:
        n = conv.norm
        c = n.num_features
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / conv.weight[0].numel()) ** 0.5)
            n.weight.copy_(0.5 + torch.rand(c, generator=g))
            n.weight[c // 3] *= -1.0
            n.bias.copy_(0.3 * torch.randn(c, generator=g))
        for key in ("weight", "bias"):
            out["%s.%s.norm.%s" % (pre, cname, key)] = getattr(n, key).detach().numpy().copy()
        out["%s.%s.norm.eps" % (pre, cname)] = np.float64(n.eps)
        out["%s.%s.weight" % (pre, cname)] = conv.weight.detach().numpy().copy()

        def hook(mod, args, output, cname=cname):
            # (the block applies relu_ / += to `output` in place afterwards: a hook registered now sees the gradient of THIS value)
            rec[cname + ".o"] = output.detach().clone()
            output.register_hook(lambda gr, cname=cname: rec.__setitem__(cname + ".g", gr.detach().clone()))
            if args[0].requires_grad and not args[0].is_leaf:
                args[0].register_hook(lambda gr, cname=cname: rec.__setitem__(cname + ".dxin", gr.detach().clone()))
        conv.register_forward_hook(hook)
    x = torch.randn(2, cin, 12, 20, generator=g).requires_grad_(True)
    y = blk(x)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    # what the hooks caught is what their names say
    dz = gy * (y > 0)
    assert torch.equal(rec["conv3.g"], dz) and ("shortcut.g" not in rec or torch.equal(rec["shortcut.g"], dz))
    assert torch.equal(rec["conv2.g"], rec["conv3.dxin"] * (rec["conv2.o"] > 0))
    assert torch.equal(rec["conv1.g"], rec["conv2.dxin"] * (rec["conv1.o"] > 0))
    sc = rec["shortcut.o"] if "shortcut.o" in rec else x.detach()
    assert torch.equal(y.detach(), torch.relu(rec["conv3.o"] + sc))
    out[pre + ".x"], out[pre + ".gy"], out[pre + ".y"] = x.detach().numpy().copy(), gy.numpy().copy(), y.detach().numpy().copy()
    out[pre + ".dx"] = x.grad.numpy().copy()
    for cname, conv in convs:
        out["%s.%s.dweight" % (pre, cname)] = conv.weight.grad.numpy().copy()
    for key in ("conv1.o", "conv2.o", "shortcut.o", "conv1.g", "conv2.g", "conv2.dxin", "conv3.dxin"):
        if key in rec:
            out["%s.%s" % (pre, key)] = rec[key].numpy().copy()
    print(pre, tuple(y.shape), float(y.detach().abs().mean()), "share of y > 0: %.2f" % float((y > 0).float().mean()))
    np.savez_compressed(os.path.join(HERE, "resnext_block_bn_%s_golden.npz" % name), **out)   # (one file per block: the size limit)


if __name__ == "__main__":
    import_reference_light()
    gen_block_fixture()
    for block in G.BLOCKS:
        gen_bn_block(block)
    gen_model_fixture()
