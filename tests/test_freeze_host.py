"""BACKBONE.FREEZE_AT and FrozenBN on the host: module tree, state-dict keys, trainable names and optimizer groups against the
reference (tests/golden/freeze_golden.json, written by tests/golden/make_freeze_fixture.py), the conversion, what precise BN and
the checkpointer see, and the float64 restatement of the FrozenBN block (tests/frozen_bn_refs.py) against the reference's fp32
known answers (tests/golden/freeze_block_golden.npz)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import frozen_bn_refs as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_DIR = os.path.join(ROOT, "configs", "COCO-PanopticSegmentation")
GOLDEN = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64


def _fixture():
    """freeze_golden.json with every case's key list and trainable names expanded from the [first index, count] runs into
    "names" (make_freeze_fixture.py write_compact)."""
    fx = json.load(open(os.path.join(GOLDEN, "freeze_golden.json")))
    for case in fx["cases"]:
        for key in ("state_dict_keys", "trainable"):
            case[key] = [fx["names"][i] for first, count in case[key] for i in range(first, first + count)]
    return fx


def _cfg(name="u2seg_R50_800.yaml", opts=()):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CFG_DIR, name))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + list(opts))
    return cfg


def _model(norm, freeze_at, opts=None):
    from u2seg_amd.modeling import build_model

    opts = _fixture()["opts"] if opts is None else opts
    cfg = _cfg(opts=list(opts) + ["MODEL.RESNETS.NORM", norm, "MODEL.BACKBONE.FREEZE_AT", freeze_at])
    return cfg, build_model(cfg)


CASES = [(c["norm"], c["freeze_at"]) for c in _fixture()["cases"]]


def test_fixture_covers_all_combinations():
    assert sorted(CASES) == sorted((n, f) for n in ("SyncBN", "FrozenBN") for f in range(6))


@pytest.mark.parametrize("norm,freeze_at", CASES)
def test_keys_trainable_names_and_groups_equal_the_reference(norm, freeze_at):
    from u2seg_amd.solver import build_optimizer

    case = next(c for c in _fixture()["cases"] if (c["norm"], c["freeze_at"]) == (norm, freeze_at))
    cfg, model = _model(norm, freeze_at)
    assert list(model.state_dict().keys()) == case["state_dict_keys"]
    assert [k for k, p in model.named_parameters() if p.requires_grad] == case["trainable"]
    opt = build_optimizer(cfg, model)
    assert [len(m) for m in opt.group_members] == case["group_sizes"]
    # no frozen tensor owns a slot of the gradient arena
    assert all(not hasattr(p, "_u2_grad") for p in model.parameters() if not p.requires_grad)
    assert model.backbone.bottom_up.frozen_prefix == freeze_at


def test_conversion_copies_buffers_eps_and_counter():
    from u2seg_amd.layers.modules import BatchNorm2d, Conv2d, FrozenBatchNorm2d

    bn = BatchNorm2d(6, eps=3e-4)
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([1.0, -2.0, 0.5, 3.0, 1.5, -0.25]))
        bn.bias.copy_(torch.arange(6.0))
        bn.running_mean.copy_(torch.arange(6.0) * 0.1)
        bn.running_var.copy_(1 + torch.arange(6.0))
    bn.count_batch()
    bn.count_batch()    # pending: not in the buffer yet
    bn.num_batches_tracked += 5
    holder = torch.nn.Sequential(Conv2d(3, 6, 1, bias=False, norm=bn))
    out = FrozenBatchNorm2d.convert_frozen_batchnorm(holder)
    assert out is holder
    fz = holder[0].norm
    assert type(fz) is FrozenBatchNorm2d and fz.eps == 3e-4 and fz.num_features == 6
    for key in ("weight", "bias", "running_mean", "running_var"):
        assert torch.equal(getattr(fz, key), getattr(bn, key).detach()), key
        assert not getattr(fz, key).requires_grad
    assert fz.weight.data_ptr() != bn.weight.data_ptr()          # the affine pair is cloned
    assert int(fz.num_batches_tracked) == 7                       # pending count flushed, counter kept
    assert list(fz.state_dict().keys()) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    assert list(fz.parameters()) == []
    s, t = fz.eval_scale_shift()
    s0, t0 = bn.eval_scale_shift()
    assert torch.equal(s, s0) and torch.equal(t, t0)
    # a module born frozen has no counter; a lone BatchNorm2d comes back as the new module
    assert list(FrozenBatchNorm2d(4).state_dict().keys()) == ["weight", "bias", "running_mean", "running_var"]
    assert type(FrozenBatchNorm2d.convert_frozen_batchnorm(BatchNorm2d(4))) is FrozenBatchNorm2d


def test_frozen_blocks_hold_frozen_norms_and_precise_bn_skips_them():
    from u2seg_amd.engine.precise_bn import get_bn_modules, update_bn_stats
    from u2seg_amd.layers.modules import BatchNorm2d, FrozenBatchNorm2d

    _, model = _model("SyncBN", 2)
    model.train()
    bu = model.backbone.bottom_up
    assert all(type(m) is FrozenBatchNorm2d for blk in [bu.stem] + list(bu.res2) for m in blk.modules() if hasattr(m, "running_var"))
    assert all(type(blk.conv1.norm) is BatchNorm2d for blk in bu.res3)
    seen = get_bn_modules(model)
    frozen = {id(m) for blk in [bu.stem] + list(bu.res2) for m in blk.modules()}
    assert seen and not any(id(m) in frozen for m in seen)
    assert len(seen) == sum(isinstance(m, BatchNorm2d) for m in model.modules())
    # nothing in training mode left: a no-op, not an error (no batch is drawn)
    _, all_frozen = _model("FrozenBN", 2, opts=list(_fixture()["opts"]) + ["MODEL.FPN.NORM", ""])
    all_frozen.train()
    assert get_bn_modules(all_frozen) == []

    def no_batches():
        raise AssertionError("precise BN drew a batch for a model without training-mode BatchNorm")
        yield

    update_bn_stats(all_frozen, no_batches(), num_iters=3)


@pytest.mark.parametrize("freeze_at,frozen_stem,frozen_stages", [(6, True, 4), (9, True, 4), (-1, False, 0), (-3, False, 0)])
def test_freeze_at_outside_the_stages_behaves_as_the_reference(freeze_at, frozen_stem, frozen_stages):
    """resnet.py:484-489 compares freeze_at with 1 and the stage numbers 2..5 and nothing else: 6 and more freeze everything, a
    negative value nothing."""
    _, model = _model("SyncBN", freeze_at)
    bu = model.backbone.bottom_up
    assert bu.stem.frozen == frozen_stem
    assert [all(b.frozen for b in st) for st in bu.stages] == [i < frozen_stages for i in range(4)]
    assert bu.frozen_prefix == (1 + frozen_stages if frozen_stem else 0)
    assert any(p.requires_grad for p in bu.parameters()) == (frozen_stages < 4)


def test_checkpoints_cross_between_default_and_finetune_models(tmp_path):
    from u2seg_amd.checkpoint import DetectionCheckpointer
    from u2seg_amd.config import get_cfg
    from u2seg_amd.modeling import build_model
    from u2seg_amd.solver import build_optimizer

    opts = list(_fixture()["opts"])

    def build(name, extra=()):
        cfg = get_cfg()
        cfg.merge_from_file(os.path.join(CFG_DIR, name))
        cfg.merge_from_list(["MODEL.DEVICE", "cpu"] + opts + list(extra))
        return cfg, build_model(cfg)

    _, default = build("u2seg_R50_800.yaml")
    dstate = default.state_dict()
    counters = {k for k in dstate if k.startswith("backbone.bottom_up.") and k.endswith(".norm.num_batches_tracked")}
    # a SyncBN-trained state dict into the same network with FrozenBN and a frozen prefix: nothing missing, the surplus - the
    # batch counters a module born frozen does not carry - reported, not fatal
    _, frozen = build("u2seg_R50_800.yaml", ["MODEL.RESNETS.NORM", "FrozenBN", "MODEL.BACKBONE.FREEZE_AT", 2])
    inc = DetectionCheckpointer(frozen)._load_model({"model": {k: v.clone() for k, v in dstate.items()}})
    assert inc.missing_keys == [] and inc.incorrect_shapes == []
    assert counters and set(inc.unexpected_keys) == counters == set(dstate) - set(frozen.state_dict())
    for k, v in frozen.state_dict().items():
        assert torch.equal(v, dstate[k]), k
    # ... and into the fine-tune config, whose FPN has no norm: its convs carry biases instead, which a SyncBN checkpoint lacks
    cfg_ft, finetune = build("u2seg_R50_800_finetune.yaml")
    fstate = finetune.state_dict()
    inc = DetectionCheckpointer(finetune)._load_model({"model": {k: v.clone() for k, v in dstate.items()}})
    biases = {"backbone.fpn_%s%d.bias" % (kind, lvl) for kind in ("lateral", "output") for lvl in (2, 3, 4, 5)}
    assert set(inc.missing_keys) == biases == set(fstate) - set(dstate) and inc.incorrect_shapes == []
    fpn_norm = {k for k in dstate if k.startswith("backbone.fpn_") and ".norm." in k}
    assert set(inc.unexpected_keys) == counters | fpn_norm == set(dstate) - set(fstate)
    for k, v in finetune.state_dict().items():
        assert k in biases or torch.equal(v, dstate[k]), k
    # the reverse: exactly the entries a frozen model does not carry are missing
    inc = DetectionCheckpointer(default)._load_model({"model": {k: v.clone() for k, v in fstate.items()}})
    assert set(inc.missing_keys) == counters | fpn_norm and set(inc.unexpected_keys) == biases
    # a checkpoint saved from the frozen model resumes into a frozen model, optimizer included
    opt = build_optimizer(cfg_ft, finetune)
    opt.flat_mom.copy_(torch.arange(opt.total, dtype=torch.float32) % 7)
    saver = DetectionCheckpointer(finetune, str(tmp_path), optimizer=opt)
    saver.save("model_0000001", iteration=1)
    _, again = build("u2seg_R50_800_finetune.yaml")
    opt2 = build_optimizer(cfg_ft, again)
    rest = DetectionCheckpointer(again, str(tmp_path), optimizer=opt2).resume_or_load("", resume=True)
    assert rest["iteration"] == 1
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), finetune.state_dict().values()))
    assert torch.equal(opt2.flat_mom, opt.flat_mom) and opt2.total == opt.total


def test_finetune_yaml_loads():
    cfg = _cfg("u2seg_R50_800_finetune.yaml")
    assert cfg.MODEL.RESNETS.NORM == "FrozenBN" and cfg.MODEL.BACKBONE.FREEZE_AT == 2 and cfg.MODEL.FPN.NORM == ""
    assert cfg.TEST.PRECISE_BN.ENABLED is False
    base = _cfg()
    assert cfg.MODEL.ROI_HEADS.NUM_CLASSES == base.MODEL.ROI_HEADS.NUM_CLASSES and cfg.SOLVER.BASE_LR == base.SOLVER.BASE_LR


def test_trainer_bucket_offsets_on_a_frozen_model():
    """engine/trainer.py asks optimizer.offset_of only for tensors that own a slot: the heads form the arena's tail."""
    from u2seg_amd.engine import SimpleTrainer
    from u2seg_amd.solver import build_optimizer

    cfg, model = _model("FrozenBN", 2)
    opt = build_optimizer(cfg, model)
    SimpleTrainer(model, opt)
    back = [opt.offset_of(p) for p in model.backbone.parameters() if p.requires_grad]
    heads = [opt.offset_of(p) for n, m in model.named_children() if n != "backbone" for p in m.parameters() if p.requires_grad]
    assert back and heads and 0 <= min(back) and max(back) < min(heads) and max(heads) < opt.total


@pytest.mark.parametrize("name", ["proj", "ident"])
def test_float64_restatement_reproduces_the_reference_block(name):
    """fp32 (the reference on the CPU) against float64, every element, bound from the term counts carried through the chain
    (tests/frozen_bn_refs.py)."""
    fx = np.load(os.path.join(GOLDEN, "freeze_block_golden.npz"))
    layers = FR.block_layers(fx, name)
    assert ("shortcut" in layers) == (name == "proj")
    assert any(bool((v[1] < 0).any()) for v in layers.values()), "a negative scale is part of the fixture"
    x, gy = torch.from_numpy(fx[name + ".x"]).to(F64), torch.from_numpy(fx[name + ".gy"]).to(F64)
    ref = FR.block_chain(layers, x, gy)
    for key, (val, bound) in ref.items():
        got = torch.from_numpy(fx["%s.%s" % (name, key)]).to(F64)
        assert got.shape == val.shape, key
        err = (got - val).abs()
        print("FROZEN64 %s %s | max |err| / E | %.4g" % (name, key, float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all()), (key, float(err.max()), float(bound.max()))
        assert float(val.abs().max()) > 0
