"""Generates tests/golden/usl_select_golden.npz by running the reference's own get_selection_with_reg_imagenet
(u2seg/Instance_Clustering/shared/utils/nn_utils_imagenet.py:105-218) and its kNN (shared/utils/nn_utils.py:204-227) on
the CPU.  Runs only where the reference is checked out; the output is committed and the tests read nothing else.

    python tests/golden/make_usl_select_fixture.py --reference PATH_TO_REFERENCE_ROOT

Stand-ins: pykeops' LazyTensor becomes a dense fp32 tensor whose Kmin / Kmin_argKmin take the first K of a stable sort
(ties: smaller index), `.cuda()` is the identity, torchvision and the reference's config / USL-T helpers are empty modules.

Data: 1 200 rows of 12 clusters in D = 32 (cluster id = generating component), neighbors_dist = the mean of the
reference kNN's 20 smallest distances.  Cases (JSON "cases", per case "<name>/labels", "<name>/nd", "<name>/picks"):
  shipped        iters 2, w 0.05, momentum 0, H 8, alpha 1, exclude True: round 2 differs from round 1 in >= 2 clusters
  iters3         iters 3, momentum 0.5, alpha 0.5
  dup_keep       exclude False; row "<name>/dup"[0] (another cluster) is a copy of round 1's pick "<name>/dup"[1]
  truncate       final_sample_num 8 < num_centroids 12
  empty_last     cluster 11 empty (its rows moved to 10), final 11
  empty_mid      cluster 5 empty (its rows moved to 4), exclude True: the reference raises AssertionError
  empty_mid_keep the same labels, exclude False
  collision      iters 1: two rows of one cluster with different nd and equal fp32 1 / nd lead it; the earlier one wins
  h_eq_s         H = S' = 12
Every visited cluster's best score leads its second by >= 1e-4 relative in every round (checked with the float64 oracle
of tests/usl_select_oracle.py, which must also reproduce every case), except at the planted collision."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.usl_select_oracle import get_selection_with_reg64, score_leads  # noqa: E402

N_PER, K_CL, D = 100, 12, 32
LEAD = 1e-4


class LazyTensor:
    """Dense stand-in for pykeops.torch.LazyTensor over the few operations the reference uses."""

    def __init__(self, t):
        self.t = t

    def __sub__(self, other):
        return LazyTensor(self.t - (other.t if isinstance(other, LazyTensor) else other))

    def __pow__(self, p):
        return LazyTensor(self.t ** p)

    def sum(self, dim):
        return LazyTensor(self.t.sum(dim))

    def Kmin(self, K, dim):
        assert dim == 1 and K <= self.t.shape[1]
        return torch.sort(self.t, dim=1, stable=True).values[:, :K].contiguous()

    def Kmin_argKmin(self, K, dim, backend=None):
        assert dim == 1 and K <= self.t.shape[1]
        s = torch.sort(self.t, dim=1, stable=True)
        return s.values[:, :K].contiguous(), s.indices[:, :K].contiguous()


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference(ref_root):
    utils = os.path.join(ref_root, "u2seg", "Instance_Clustering", "shared", "utils")
    _module("pykeops")
    _module("pykeops.torch", LazyTensor=LazyTensor)
    _module("tqdm", tqdm=lambda it, *a, **k: it)
    tv = _module("torchvision")
    tv.datasets = _module("torchvision.datasets", ImageFolder=type("ImageFolder", (), {}))
    tv.transforms = _module("torchvision.transforms")
    if importlib.util.find_spec("pandas") is None:
        _module("pandas")
    pkg = _module("refusl")
    pkg.__path__ = [utils]
    import logging

    _module("refusl.config_utils", cfg=types.SimpleNamespace(), logger=logging.getLogger("refusl"))
    _module("refusl.uslt_utils", LocalGlobalDataset=object)
    mods = {}
    for name in ("nn_utils", "nn_utils_imagenet"):
        spec = importlib.util.spec_from_file_location("refusl." + name, os.path.join(utils, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["refusl." + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    torch.Tensor.cuda = lambda self, *a, **k: self
    return mods["nn_utils"], mods["nn_utils_imagenet"]


def make_data(seed, sep, sigma):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(K_CL, D, generator=g) * sep
    labels = torch.arange(K_CL).repeat_interleave(N_PER)
    x = centers[labels] + torch.randn(K_CL * N_PER, D, generator=g) * sigma * (0.5 + torch.rand(K_CL * N_PER, 1, generator=g))
    perm = torch.randperm(K_CL * N_PER, generator=g)
    return x[perm].float().contiguous(), labels[perm].contiguous()


def nd_of(nnu, x):
    _, d_knn = nnu.kNN(x, x, K=20)
    return d_knn.mean(dim=1)


def run_ref(nui, x, nd, labels, p):
    try:
        return nui.get_selection_with_reg_imagenet(
            x, nd, labels, p["num_centroids"], iters=p["iters"], final_sample_num=p["final_sample_num"], w=p["w"],
            momentum=p["momentum"], horizon_num=p["horizon_num"], alpha=p["alpha"],
            exclude_same_cluster=p["exclude_same_cluster"]).astype(np.int64), False
    except AssertionError:
        return np.zeros(0, dtype=np.int64), True


def check_case(name, x, nd, labels, p, picks, raises, skip_cluster=None):
    kw = {k: p[k] for k in ("iters", "final_sample_num", "w", "momentum", "horizon_num", "alpha", "exclude_same_cluster")}
    try:
        got, regs = get_selection_with_reg64(x, nd, labels, p["num_centroids"], return_regs=True, **kw)
    except AssertionError:
        assert raises, name + ": the oracle raised, the reference did not"
        return True
    assert not raises and got == picks.tolist(), (name, got, picks.tolist())
    for reg in [torch.zeros(len(nd), dtype=torch.float64)] + regs:
        leads = score_leads(nd, reg.float(), labels, p["num_centroids"], p["final_sample_num"], p["w"])
        vis = [c for c in range(p["num_centroids"]) if (labels == c).any()][:p["final_sample_num"]]
        for c, lead in zip(vis, leads):
            if c != skip_cluster and lead < LEAD:
                return False
    return True


def plant_collision(nd, labels, c):
    """Two rows a < b of cluster c: nd[b] < nd[a], fp32 1 / nd equal, both well ahead of the rest of the cluster."""
    rows = torch.where(labels == c)[0]
    a, b = int(rows[0]), int(rows[1])
    lo = float(nd[rows].min()) * 0.9
    e = int(np.floor(np.log2(lo)))
    v = np.float32(2.0 ** e * 1.9)  # upper part of a binade: neighbouring floats can share a correctly rounded reciprocal
    if v >= lo:
        v = np.float32(2.0 ** (e - 1) * 1.9)
    one = np.float32(1)
    for _ in range(100000):
        u = np.nextafter(v, np.float32(np.inf))
        if one / v == one / u:
            break
        v = np.nextafter(v, np.float32(0))
    else:
        raise SystemExit("no reciprocal collision found")
    nd = nd.clone()
    nd[a], nd[b] = float(u), float(v)
    return nd, a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    nnu, nui = load_reference(args.reference)
    base = dict(num_centroids=K_CL, iters=2, final_sample_num=K_CL, w=0.05, momentum=0.0, horizon_num=8, alpha=1.0,
                exclude_same_cluster=True)
    for seed in range(200):
        x, labels = make_data(seed, sep=1.0, sigma=0.5)
        nd = nd_of(nnu, x)
        out, cases, ok = {}, [], True

        def add(name, lab, ndv, p, skip=None, xv=None, extra=None):
            xv = x if xv is None else xv
            picks, raises = run_ref(nui, xv, ndv, lab, p)
            if not check_case(name, xv, ndv, lab, p, picks, raises, skip):
                return None
            out[name + "/labels"] = lab.numpy().astype(np.int64)
            out[name + "/nd"] = ndv.numpy().astype(np.float32)
            out[name + "/picks"] = picks
            cases.append(dict(p, name=name, raises=raises, **(extra or {})))
            return picks, raises

        r = add("shipped", labels, nd, base)
        round1, _ = run_ref(nui, x, nd, labels, dict(base, iters=1))
        if r is None or (r[0] != round1).sum() < 2:
            continue
        ok = add("iters3", labels, nd, dict(base, iters=3, momentum=0.5, alpha=0.5)) is not None
        # a copy of round 1's pick of cluster 0 in another cluster's row
        p0 = int(round1[0])
        r_dup = int(torch.where(labels == 1)[0][-1])
        xd = x.clone()
        xd[r_dup] = x[p0]
        ndd = nd_of(nnu, xd)
        res = add("dup_keep", labels, ndd, dict(base, exclude_same_cluster=False), xv=xd, extra=dict(dup=[r_dup, p0]))
        ok = ok and res is not None
        if ok:
            out["dup_keep/x"] = xd.numpy()
        ok = ok and add("truncate", labels, nd, dict(base, final_sample_num=8, horizon_num=6)) is not None
        lab_last = torch.where(labels == 11, torch.tensor(10), labels)
        ok = ok and add("empty_last", lab_last, nd, dict(base, final_sample_num=11)) is not None
        lab_mid = torch.where(labels == 5, torch.tensor(4), labels)
        res = add("empty_mid", lab_mid, nd, dict(base, final_sample_num=11))
        ok = ok and res is not None and res[1]
        res = add("empty_mid_keep", lab_mid, nd, dict(base, final_sample_num=11, exclude_same_cluster=False))
        ok = ok and res is not None and not res[1]
        ndc, a, b = plant_collision(nd, labels, 3)
        res = add("collision", labels, ndc, dict(base, iters=1), skip=3, extra=dict(collision=[a, b]))
        ok = ok and res is not None and int(res[0][3]) == a
        ok = ok and add("h_eq_s", labels, nd, dict(base, horizon_num=K_CL)) is not None
        if ok:
            break
    else:
        raise SystemExit("no seed satisfied every case")
    out["x"] = x.numpy()
    out["cases"] = np.array(json.dumps({"seed": seed, "cases": cases}))
    path = os.path.join(HERE, "usl_select_golden.npz")
    np.savez_compressed(path, **out)
    print("seed %d: wrote %s (%d bytes), cases %s" % (seed, path, os.path.getsize(path), [c["name"] for c in cases]))


if __name__ == "__main__":
    main()
