"""Fixtures of BACKBONE.FREEZE_AT / FrozenBN, written from the reference (imported through make_fixtures.py's stand-ins).

  freeze_golden.json       for FREEZE_AT 0..5 x RESNETS.NORM {SyncBN, FrozenBN} on the reduced u2seg_R50_800: the ordered state-dict
                           keys, the names of the trainable parameters and the sizes of the optimizer's parameter groups
                           (names stored once, the lists as index runs: write_compact).
  freeze_block_golden.npz  fp32 CPU known answers of one reference BottleneckBlock with FrozenBN (non-trivial buffers, one negative
                           weight per norm): a projection-shortcut stride-2 block and an identity-shortcut block on a 2x16x12x20
                           input - output, and the gradients w.r.t. the input and the conv weights for a recorded output gradient.

Both files hold data only.  Run: python tests/golden/make_freeze_fixture.py"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as MF  # noqa: E402
from tests import frozen_bn_refs as FR  # noqa: E402  (this repository's tests package: before the reference joins sys.path)

FREEZE_AT = [0, 1, 2, 3, 4, 5]
NORMS = ["SyncBN", "FrozenBN"]
BLOCKS = {   # name -> (in, out, bottleneck, stride)
    "proj": (16, 32, 8, 2),
    "ident": (16, 16, 8, 1),
}


def import_reference_light():
    MF.install_standins()
    sys.path.insert(0, MF.REF)
    sys.modules["detectron2._C"] = types.ModuleType("detectron2._C")   # no compiled op is run


def gen_freeze_fixture():
    os.environ.setdefault("CLUSTER_NUM", "800")
    from detectron2.config import get_cfg
    from detectron2.modeling import build_model
    from detectron2.solver import build_optimizer

    cases = []
    for norm in NORMS:
        for fa in FREEZE_AT:
            cfg = get_cfg()
            cfg.merge_from_file(os.path.join(MF.REF, "configs/COCO-PanopticSegmentation/u2seg_R50_800.yaml"))
            cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHTS", ""] + MF.REDUCED_MODEL_OPTS
                                + ["MODEL.RESNETS.NORM", norm, "MODEL.BACKBONE.FREEZE_AT", fa])
            model = build_model(cfg)
            opt = build_optimizer(cfg, model)
            cases.append({"norm": norm, "freeze_at": fa,
                          "state_dict_keys": list(model.state_dict().keys()),
                          "trainable": [k for k, p in model.named_parameters() if p.requires_grad],
                          "group_sizes": [len(g["params"]) for g in opt.param_groups]})
            print(norm, fa, len(cases[-1]["state_dict_keys"]), len(cases[-1]["trainable"]), cases[-1]["group_sizes"])
    write_compact(cases, os.path.join(HERE, "freeze_golden.json"))


def write_compact(cases, path):
    """Every name once ("names": the longest key list, whose order all others follow), and per case its key list and its
    trainable names as ascending runs [first index, count] into it; tests/test_freeze_host.py expands them again."""
    names = max((c["state_dict_keys"] for c in cases), key=len)
    idx = {k: i for i, k in enumerate(names)}

    def runs(keys):
        ix = [idx[k] for k in keys]
        assert ix == sorted(ix), "a list that does not follow the order of the longest one"
        out = []
        for i in ix:
            if out and out[-1][0] + out[-1][1] == i:
                out[-1][1] += 1
            else:
                out.append([i, 1])
        return out

    rows = [dict(c, state_dict_keys=runs(c["state_dict_keys"]), trainable=runs(c["trainable"])) for c in cases]
    with open(path, "w") as f:
        f.write('{"opts": %s,\n"names": [\n' % json.dumps(MF.REDUCED_MODEL_OPTS))
        for i in range(0, len(names), 6):
            f.write(" " + ", ".join(json.dumps(n) for n in names[i:i + 6]) + (",\n" if i + 6 < len(names) else "\n"))
        f.write('],\n"cases": [\n' + ",\n".join(" " + json.dumps(c) for c in rows) + "\n]}\n")


def gen_block_fixture():
    from detectron2.modeling.backbone.resnet import BottleneckBlock

    out = {}
    for name, seed in [(n, s) for n in BLOCKS for s in range(8)]:
        if name + ".y" in out:
            continue
        cin, cout, cb, stride = BLOCKS[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)) + seed)
        blk = BottleneckBlock(cin, cout, bottleneck_channels=cb, stride=stride, norm="FrozenBN")
        convs = [("conv1", blk.conv1), ("conv2", blk.conv2), ("conv3", blk.conv3)]
        if blk.shortcut is not None:
            convs.append(("shortcut", blk.shortcut))
        for cname, conv in convs:
            n = conv.norm
            c = n.num_features
            n.weight.copy_(0.5 + torch.rand(c, generator=g))
            n.weight[c // 3] *= -1.0
            n.bias.copy_(0.3 * torch.randn(c, generator=g))
            n.running_mean.copy_(0.2 * torch.randn(c, generator=g))
            n.running_var.copy_(0.5 + torch.rand(c, generator=g))
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / conv.weight[0].numel()) ** 0.5)
            conv.weight.requires_grad_(True)
            for key in ("weight", "bias", "running_mean", "running_var"):
                out["%s.%s.norm.%s" % (name, cname, key)] = getattr(n, key).numpy().copy()
            out["%s.%s.norm.eps" % (name, cname)] = np.float64(n.eps)
            out["%s.%s.weight" % (name, cname)] = conv.weight.detach().numpy().copy()
        x = torch.randn(2, cin, 12, 20, generator=g).requires_grad_(True)
        y = blk(x)
        gy = torch.randn(y.shape, generator=g)
        y.backward(gy)
        out[name + ".x"], out[name + ".gy"], out[name + ".y"] = x.detach().numpy().copy(), gy.numpy().copy(), y.detach().numpy().copy()
        out[name + ".dx"] = x.grad.numpy().copy()
        for cname, conv in convs:
            out["%s.%s.dweight" % (name, cname)] = conv.weight.grad.numpy().copy()
        try:   # the host test's precondition: no ReLU input within the fp32 error of zero (else: the next seed)
            FR.block_chain(FR.block_layers(out, name), x.detach().double(), gy.double())
        except AssertionError as e:
            print(name, "seed", seed, "rejected:", e)
            for k in [k for k in out if k.startswith(name + ".")]:
                del out[k]
            continue
        print(name, "seed", seed, tuple(y.shape), float(y.detach().abs().mean()), float(x.grad.abs().mean()))
    assert all(n + ".y" in out for n in BLOCKS)
    np.savez_compressed(os.path.join(HERE, "freeze_block_golden.npz"), **out)


if __name__ == "__main__":
    import_reference_light()
    gen_block_fixture()
    gen_freeze_fixture()
