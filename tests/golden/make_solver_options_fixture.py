"""Writes tests/golden/solver_options_golden.npz: the REFERENCE's own build_optimizer (detectron2/solver/build.py:119-139: clip-wrapped
torch.optim.SGD over get_default_optimizer_params) on the small module of tests/solver_option_refs.py, for each option set of
NET_CASES on top of NET_SOLVER (BIAS_LR_FACTOR 2, WEIGHT_DECAY_BIAS, Nesterov; clipping by value, by L1 norm, by inf norm), three
steps on the fixed gradients net_grads(k) with the reference's plain WarmupCosineLR (solver/lr_scheduler.py:180-219, no warm-up)
moving both groups' rates every step.  Per case: parameters and momentum buffers after the three steps, the rates of every step,
and the `param_groups` of the optimizer's state_dict() as JSON; and the rates of that scheduler class alone, with warm-up, at
every iteration of the runs COSINE_RUNS.  Of the 75 000-element weight only the elements
solver_option_refs.big_index() names are kept (both ends, both sides of the chunk boundary, every 97th): its norm, and so every
kept element, still depends on all of them.

    python tests/golden/make_solver_options_fixture.py        (needs the reference tree; see make_fixtures.py)

The third-party stand-ins are those of make_fixtures.py, by import."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_fixtures as MF  # noqa: E402  (puts the repository root on sys.path)

from tests import solver_option_refs as S  # noqa: E402


def main():
    MF.install_standins()
    sys.path.insert(0, MF.REF)
    from detectron2.config import get_cfg
    from detectron2.solver import build_optimizer
    from detectron2.solver.lr_scheduler import WarmupCosineLR

    out = {}
    for case, clip in S.NET_CASES.items():
        cfg = get_cfg()
        for k, v in S.NET_SOLVER.items():
            cfg.SOLVER[k] = v
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
        for k, v in clip.items():
            cfg.SOLVER.CLIP_GRADIENTS[k] = v
        net = S.build_net(torch.nn.GroupNorm)
        opt = build_optimizer(cfg, net)
        sched = WarmupCosineLR(opt, cfg.SOLVER.MAX_ITER, warmup_iters=cfg.SOLVER.WARMUP_ITERS)
        lrs = []
        for step in range(S.NET_STEPS):
            lrs.append([g["lr"] for g in opt.param_groups])
            for p, g in zip(net.parameters(), S.net_grads(step)):
                p.grad = g.clone()
            opt.step()
            sched.step()
        sd = opt.state_dict()
        names = {id(p): k for k, p in net.named_parameters()}
        order = [names[id(p)] for g in opt.param_groups for p in g["params"]]
        out[case + "/param_groups"] = np.array(json.dumps(sd["param_groups"]))
        out[case + "/numbering"] = np.array(json.dumps(order))
        out[case + "/lrs"] = np.array(lrs, dtype=np.float64)
        for i, name in enumerate(order):
            out["%s/momentum/%s" % (case, name)] = S.kept(sd["state"][i]["momentum_buffer"]).numpy().copy()
        for name, p in net.named_parameters():
            out["%s/param/%s" % (case, name)] = S.kept(p.detach()).numpy().copy()
        print(case, [len(g["params"]) for g in sd["param_groups"]], lrs[-1])
    # the plain WarmupCosineLR class itself, every iteration: the yardstick of the cosine schedule after warm-up
    for max_iter, warmup in S.COSINE_RUNS:
        p = torch.nn.Parameter(torch.zeros(1))
        sched = WarmupCosineLR(torch.optim.SGD([p], lr=S.COSINE_BASE_LR), max_iter, warmup_iters=warmup)
        lrs = []
        for _ in range(max_iter + 1):
            lrs.append(sched.get_last_lr()[0])
            sched.optimizer.step()
            sched.step()
        out["cosine/%d_%d" % (max_iter, warmup)] = np.array(lrs, dtype=np.float64)
    path = os.path.join(HERE, "solver_options_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
