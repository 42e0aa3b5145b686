"""The solver's options on the host (u2seg_amd/solver/build.py): parameter groups with a bias learning rate against the reference's
own build_optimizer (tests/golden/solver_options_golden.npz, written by tests/golden/make_solver_options_fixture.py), state dicts
with per-group rates, the schedules, and the config keys.  No device."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import solver_option_refs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "solver_options_golden.npz"))


def net_cfg(case):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    for k, v in S.NET_SOLVER.items():
        cfg.SOLVER[k] = v
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    for k, v in S.NET_CASES[case].items():
        cfg.SOLVER.CLIP_GRADIENTS[k] = v
    return cfg


def build(case):
    from u2seg_amd.layers.modules import GroupNorm
    from u2seg_amd.solver import build_lr_scheduler, build_optimizer

    cfg = net_cfg(case)
    net = S.build_net(GroupNorm)
    opt = build_optimizer(cfg, net)
    return cfg, net, opt, build_lr_scheduler(cfg, opt)


# =================================================================================================
# 5. groups and state dicts against the reference's optimizer
@pytest.mark.parametrize("case", sorted(S.NET_CASES))
def test_groups_and_rates_equal_the_reference(golden, case):
    """FlatSGD's groups, torch's numbering and every group entry - lr, initial_lr, nesterov, weight_decay, ... - after three
    scheduler steps equal what the reference's build_optimizer + WarmupCosineLR hold after three steps of its own: the rates to
    1e-15 relative (the schedule multiplies in another order), everything else exactly."""
    from u2seg_amd.solver import FlatSGD

    cfg, net, opt, sched = build(case)
    ref_groups = json.loads(str(golden[case + "/param_groups"]))
    names = {id(p): k for k, p in net.named_parameters()}
    assert [names[id(opt.params[i])] for m in opt.group_members for i in m] == json.loads(str(golden[case + "/numbering"]))
    assert opt.group_lr_class == [0, 1, 0]
    assert opt.clip_mode == {"value": S.VALUE, "l1": S.L1, "inf": S.INF}[case] and opt.nesterov
    for k in range(S.NET_STEPS):
        got = [opt.lr_bias if c else opt.lr for c in opt.group_lr_class]
        assert got == pytest.approx(list(golden[case + "/lrs"][k]), rel=1e-15, abs=0)
        sched.step()
    mine = opt.state_dict()["param_groups"]
    assert len(mine) == len(ref_groups)
    for a, b in zip(mine, ref_groups):
        a, b = dict(a), dict(b)
        assert a.pop("lr") == pytest.approx(b.pop("lr"), rel=1e-15) and a == b, (a, b)
    assert a["nesterov"] is True and mine[1]["initial_lr"] == 0.2 and mine[0]["initial_lr"] == 0.1
    assert sched.state_dict()["base_lrs"] == [0.1, 0.2, 0.1] and sched.state_dict()["last_epoch"] == S.NET_STEPS
    # Nesterov without momentum: torch's error
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum"):
        FlatSGD(S.build_net(torch.nn.GroupNorm), lr=0.1, momentum=0.0, nesterov=True)


def reference_state_dict(golden, case):
    """The state dict the reference's torch.optim.SGD wrote, rebuilt from the fixture (the 75 000-element buffer is kept only at
    big_index(): the rest is filled with zeros)."""
    groups = json.loads(str(golden[case + "/param_groups"]))
    order = json.loads(str(golden[case + "/numbering"]))
    shapes = dict(S.NET_PARAMS)
    state = {}
    for i, name in enumerate(order):
        buf = torch.from_numpy(golden["%s/momentum/%s" % (case, name)])
        if name == "big.weight":
            full = torch.zeros(75000)
            full[S.big_index()] = buf
            buf = full
        state[i] = {"momentum_buffer": buf.view(shapes[name]).clone()}
    return {"state": state, "param_groups": groups}


def test_reference_state_dict_with_per_group_rates_round_trips(golden):
    """A reference state dict whose groups differ in lr loads: groups by position, the bias-class group feeds lr_bias, momentum
    buffers arrive under torch's numbering; what FlatSGD writes back is that dict; torch's own SGD loads it."""
    sd = reference_state_dict(golden, "value")
    assert len({g["lr"] for g in sd["param_groups"]}) == 2
    cfg, net, opt, sched = build("value")
    opt.load_state_dict(copy.deepcopy(sd))
    assert opt.lr == sd["param_groups"][0]["lr"] and opt.lr_bias == sd["param_groups"][1]["lr"]
    assert opt.base_lr == 0.1 and opt.initial_lr_bias == 0.2 and opt.nesterov
    back = opt.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert all(torch.equal(back["state"][i]["momentum_buffer"], sd["state"][i]["momentum_buffer"]) for i in sd["state"])
    names = [k for k, _ in net.named_parameters()]
    off = dict(zip(names, opt.param_offset))
    got = opt.flat_mom[off["fc.bias"]: off["fc.bias"] + 5]
    assert torch.equal(got, torch.from_numpy(golden["value/momentum/fc.bias"]))
    clones = [torch.nn.Parameter(p.detach().clone()) for p in opt.params]
    tsgd = torch.optim.SGD([{"params": [clones[i] for i in m]} for m in opt.group_members], lr=1.0, momentum=0.5)
    tsgd.load_state_dict(back)
    assert [g["lr"] for g in tsgd.param_groups] == [g["lr"] for g in sd["param_groups"]] and tsgd.param_groups[0]["nesterov"]
    # the schedule continues both rates from the file's position
    sched.resume_at(S.NET_STEPS)
    m = 0.5 * (1.0 + math.cos(math.pi * (S.NET_STEPS / S.NET_MAX_ITER)))
    assert opt.lr == 0.1 * m and opt.lr_bias == 0.2 * m


def test_state_dict_with_a_third_rate_is_refused(golden):
    sd = reference_state_dict(golden, "value")
    sd["param_groups"][2]["lr"] = 0.5 * sd["param_groups"][0]["lr"]     # groups 0 and 2 are the base class
    cfg, net, opt, sched = build("value")
    with pytest.raises(ValueError, match=r"param_groups \[\[0\], \[2\]\] hold different 'lr'"):
        opt.load_state_dict(sd)
    # an optimizer built with one rate refuses a file with two, naming the key
    from u2seg_amd.layers.modules import GroupNorm
    from u2seg_amd.solver import FlatSGD

    one = FlatSGD(S.build_net(GroupNorm), lr=0.1, weight_decay=1e-4, weight_decay_norm=0.0, weight_decay_bias=1e-3, clip_value=1.0)
    assert [len(m) for m in one.group_members] == [3, 3, 1]
    with pytest.raises(ValueError, match="BIAS_LR_FACTOR"):
        one.load_state_dict(reference_state_dict(golden, "value"))
    for key, value in (("dampening", 0.5), ("maximize", True)):
        bad = reference_state_dict(golden, "value")
        bad["param_groups"][1][key] = value
        with pytest.raises(ValueError, match=key):
            opt.load_state_dict(bad)


# =================================================================================================
# 6. schedules
class _Opt:
    lr = 0.0


def cosine_cfg(**solver):
    from u2seg_amd.config import get_cfg

    cfg = get_cfg()
    cfg.SOLVER.LR_SCHEDULER_NAME = "WarmupCosineLR"
    for k, v in solver.items():
        cfg.SOLVER[k] = v
    return cfg


@pytest.mark.parametrize("max_iter,warmup", S.COSINE_RUNS)
def test_cosine_equals_the_reference_class_after_warmup(golden, max_iter, warmup):
    """BASE_LR_END 0: every iteration from the end of warm-up to MAX_ITER equals the reference's plain WarmupCosineLR
    (lr_scheduler.py:180-219; the fixture holds what the class itself returned at every iteration) to 1e-12 relative.  The two
    sides differ in the rounding of the cosine's argument, pi (it / M) against (pi it) / M.  Inside the warm-up the plain class
    multiplies the cosine by a factor where the composite interpolates towards sched(warmup_length): another schedule, not
    compared."""
    from u2seg_amd.solver import build_lr_scheduler

    ref = golden["cosine/%d_%d" % (max_iter, warmup)]
    assert ref.shape == (max_iter + 1,) and ref[max_iter // 2] == S.COSINE_BASE_LR * 0.5 * (1.0 + math.cos(math.pi * (max_iter // 2) / max_iter))
    cfg = cosine_cfg(BASE_LR=S.COSINE_BASE_LR, BASE_LR_END=0.0, MAX_ITER=max_iter, WARMUP_ITERS=warmup)
    sched = build_lr_scheduler(cfg, _Opt())
    for it in range(warmup, max_iter + 1):
        assert sched.get_lr(it) == pytest.approx(float(ref[it]), rel=1e-12, abs=0), it


def test_composite_warmup_values_by_hand():
    """Warm-up, `constant`, RESCALE_INTERVAL and BASE_LR_END > 0 against numbers worked out by hand from
    solver/lr_scheduler.py:46-58 and solver/build.py:302-322.  fvcore, whose composite the reference runs, is not available:
    these four are parity unpinned against it.  MAX_ITER 100, WARMUP_ITERS 20 (warmup_length 0.2), WARMUP_FACTOR 0.1,
    BASE_LR 0.5, cos(x) = c(x) below."""
    from u2seg_amd.solver import build_lr_scheduler

    c = lambda where: 0.5 * (1.0 + math.cos(math.pi * where))
    common = dict(BASE_LR=0.5, MAX_ITER=100, WARMUP_ITERS=20, WARMUP_FACTOR=0.1)

    def lr(it, **kw):
        return build_lr_scheduler(cosine_cfg(**dict(common, **kw)), _Opt()).get_lr(it)

    # linear, fixed interval: from 0.1 * sched(0) = 0.1 to sched(0.2); at iteration 5, a = 0.05 / 0.2 = 0.25
    end = c(0.2)
    assert lr(0) == pytest.approx(0.5 * 0.1, rel=1e-15)
    assert lr(5) == pytest.approx(0.5 * (end * 0.25 + 0.1 * 0.75), rel=1e-14)
    assert lr(19) == pytest.approx(0.5 * (end * 0.95 + 0.1 * 0.05), rel=1e-14)
    assert lr(20) == pytest.approx(0.5 * c(0.2), rel=1e-14) and lr(60) == pytest.approx(0.5 * c(0.6), rel=1e-14)
    assert lr(100) == pytest.approx(0.0, abs=1e-17)
    # constant: the start value throughout the warm-up, then the main schedule
    assert lr(0, WARMUP_METHOD="constant") == lr(19, WARMUP_METHOD="constant") == pytest.approx(0.05, rel=1e-15)
    assert lr(20, WARMUP_METHOD="constant") == pytest.approx(0.5 * c(0.2), rel=1e-14)
    # rescaled: the warm-up ends at sched(0) = 1, and the main schedule runs over (where - 0.2) / 0.8
    assert lr(5, RESCALE_INTERVAL=True) == pytest.approx(0.5 * (1.0 * 0.25 + 0.1 * 0.75), rel=1e-14)
    assert lr(20, RESCALE_INTERVAL=True) == pytest.approx(0.5, rel=1e-14)
    assert lr(60, RESCALE_INTERVAL=True) == pytest.approx(0.5 * c(0.5), rel=1e-13)
    assert lr(100, RESCALE_INTERVAL=True) == pytest.approx(0.0, abs=1e-16)
    # BASE_LR_END 0.05: end = 0.1; sched(w) = 0.1 + 0.9 c(w)
    e = lambda where: 0.1 + 0.9 * c(where)
    assert lr(60, BASE_LR_END=0.05) == pytest.approx(0.5 * e(0.6), rel=1e-14)
    assert lr(100, BASE_LR_END=0.05) == pytest.approx(0.05, rel=1e-14)
    assert lr(5, BASE_LR_END=0.05) == pytest.approx(0.5 * (e(0.2) * 0.25 + 0.1 * 0.75), rel=1e-14)
    # multi-step through the same class (constant warm-up is not the shipped path): STEPS (30, 50), GAMMA 0.1
    ms = dict(LR_SCHEDULER_NAME="WarmupMultiStepLR", STEPS=(30, 50), GAMMA=0.1, WARMUP_METHOD="constant")
    assert [lr(it, **ms) for it in (0, 19, 20, 29, 30, 50, 99)] == pytest.approx([0.05, 0.05, 0.5, 0.5, 0.05, 0.005, 0.005], rel=1e-14)
    assert lr(25, **dict(ms, RESCALE_INTERVAL=True)) == pytest.approx(0.5, rel=1e-14)   # (0.25 - 0.2) / 0.8 -> iteration 6
    assert lr(50, **dict(ms, RESCALE_INTERVAL=True)) == pytest.approx(0.05, rel=1e-14)  # (0.5 - 0.2) / 0.8 = 0.375 -> 37
    with pytest.raises(ValueError, match="BASE_LR_END"):
        lr(0, BASE_LR_END=1.0)
    with pytest.raises(ValueError, match="WARMUP_METHOD"):
        lr(0, WARMUP_METHOD="exponential")


ITERS = (0, 1, 999, 1000, 210000, 250000)


def test_multistep_values_and_the_bias_rate_for_the_shipped_config():
    """u2seg_R50_800.yaml: build_lr_scheduler returns the class it always returned; the multiplier class (what a bias rate or
    another warm-up selects) gives the same values - exactly outside the warm-up, within two roundings (4.5e-16 relative) inside
    it, where it multiplies base_lr into the interpolation last and the existing class first.  With BIAS_LR_FACTOR 2 the bias
    rate is initial_lr_bias * multiplier in doubles."""
    from u2seg_amd.config import get_cfg
    from u2seg_amd.solver import WarmupLR, WarmupMultiStepLR, build_lr_scheduler
    from u2seg_amd.solver.build import multistep_schedule

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800.yaml"))
    s = cfg.SOLVER
    old = build_lr_scheduler(cfg, _Opt())
    assert type(old) is WarmupMultiStepLR

    class BiasOpt:
        lr, lr_bias, has_bias_lr, initial_lr_bias, group_lr_class = 0.0, 0.0, True, s.BASE_LR * 2.0, [0, 1]

    opt = BiasOpt()
    new = build_lr_scheduler(cfg, opt)
    assert type(new) is WarmupLR and new.state_dict()["base_lrs"] == [s.BASE_LR, s.BASE_LR * 2.0]
    for it in ITERS:
        exact = it == 0 or it >= s.WARMUP_ITERS
        assert new.get_lr(it) == (old.get_lr(it) if exact else pytest.approx(old.get_lr(it), rel=4.5e-16, abs=0)), it
        new.resume_at(it)
        assert opt.lr == new.get_lr(it) and opt.lr_bias == opt.initial_lr_bias * new.multiplier(it), it
    assert [new.multiplier(it) for it in (1000, 210000, 250000)] == [1.0, s.GAMMA, s.GAMMA ** 2]
    sched = multistep_schedule([210000, 250000], s.GAMMA, s.MAX_ITER)
    assert sched(209999 / s.MAX_ITER) == 1.0 and sched(210000 / s.MAX_ITER) == s.GAMMA


# =================================================================================================
# 7. config
def test_cosine_config_builds_and_unsupported_values_name_their_key():
    from u2seg_amd.config import get_cfg
    from u2seg_amd.layers.modules import GroupNorm
    from u2seg_amd.solver import WarmupLR, build_lr_scheduler, build_optimizer
    from u2seg_amd.solver.build import CLIP_INF, CLIP_L1, CLIP_L2, CLIP_NONE, CLIP_VALUE

    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "COCO-PanopticSegmentation", "u2seg_R50_800_cosine.yaml"))
    s = cfg.SOLVER
    assert s.LR_SCHEDULER_NAME == "WarmupCosineLR" and s.NESTEROV and s.CLIP_GRADIENTS.CLIP_TYPE == "value" and s.BASE_LR == 0.01
    opt = build_optimizer(cfg, S.build_net(GroupNorm))
    sched = build_lr_scheduler(cfg, opt)
    assert type(sched) is WarmupLR and opt.clip_mode == CLIP_VALUE and opt.nesterov and not opt.has_bias_lr
    assert opt.lr == pytest.approx(s.BASE_LR * s.WARMUP_FACTOR, rel=1e-15)
    assert sched.get_lr(s.MAX_ITER) == pytest.approx(s.BASE_LR_END, rel=1e-12)
    assert all(g["nesterov"] for g in opt.state_dict()["param_groups"])

    def with_(*pairs):
        c = cfg.clone() if hasattr(cfg, "clone") else copy.deepcopy(cfg)
        c.merge_from_list(list(pairs))
        return c

    modes = {("norm", 2.0): CLIP_L2, ("norm", 1.0): CLIP_L1, ("norm", float("inf")): CLIP_INF, ("norm", "inf"): CLIP_INF}
    for (ctype, ntype), mode in modes.items():
        c = with_("SOLVER.CLIP_GRADIENTS.CLIP_TYPE", ctype)
        c.SOLVER.CLIP_GRADIENTS.NORM_TYPE = ntype
        assert build_optimizer(c, S.build_net(GroupNorm)).clip_mode == mode
    c = with_("SOLVER.CLIP_GRADIENTS.ENABLED", False)
    assert build_optimizer(c, S.build_net(GroupNorm)).clip_mode == CLIP_NONE
    c = with_("SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.CLIP_GRADIENTS.NORM_TYPE", 3.0)
    with pytest.raises(ValueError, match=r"SOLVER\.CLIP_GRADIENTS\.NORM_TYPE"):
        build_optimizer(c, S.build_net(GroupNorm))
    c = with_("SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model")
    with pytest.raises(ValueError, match=r"SOLVER\.CLIP_GRADIENTS\.CLIP_TYPE"):
        build_optimizer(c, S.build_net(GroupNorm))
    c = with_("SOLVER.LR_SCHEDULER_NAME", "WarmupStepWithFixedGammaLR")
    with pytest.raises(ValueError, match=r"SOLVER\.LR_SCHEDULER_NAME.*fvcore"):
        build_lr_scheduler(c, opt)
    c = with_("SOLVER.MOMENTUM", 0.0)
    with pytest.raises(ValueError, match="Nesterov"):
        build_optimizer(c, S.build_net(GroupNorm))
