"""USL's regularised selection on the GPU (u2seg_amd/csrc/usl.hip, u2seg_amd/cluster/select.py): the reference's
recorded picks (tests/golden/usl_select_golden.npz), the regularizer against the float64 oracle (tests/usl_select_oracle.py)
on ragged shapes and at full size, and the stage-1 tool end to end."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import float64_refs as R
from tests.usl_select_oracle import horizon_dists, regularizer64, select_loop

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "usl_select_golden.npz")
CASES = ["shipped", "iters3", "dup_keep", "truncate", "empty_last", "empty_mid", "empty_mid_keep", "collision", "h_eq_s"]


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_match_reference(H, name):
    from u2seg_amd.cluster.select import get_selection_with_reg_imagenet

    z = np.load(GOLDEN)
    c = next(c for c in json.loads(str(z["cases"]))["cases"] if c["name"] == name)
    x = torch.from_numpy(z[name + "/x"] if name + "/x" in z.files else z["x"])
    nd, labels = torch.from_numpy(z[name + "/nd"]), torch.from_numpy(z[name + "/labels"])
    kw = {k: c[k] for k in ("iters", "final_sample_num", "w", "momentum", "horizon_num", "alpha", "exclude_same_cluster")}
    if c["raises"]:
        with pytest.raises(AssertionError):
            get_selection_with_reg_imagenet(x, nd, labels, c["num_centroids"], **kw)
        return
    got = get_selection_with_reg_imagenet(x, nd, labels, c["num_centroids"], **kw)
    assert got.dtype == np.int64
    assert got.tolist() == z[name + "/picks"].tolist()


def clustered(n, d, k, seed, unit=False):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    centers = torch.randn(k, d, device=DEV, generator=g)
    lab = torch.randint(0, k, (n,), device=DEV, generator=g)
    x = centers[lab] + 0.6 * torch.randn(n, d, device=DEV, generator=g)
    if unit:
        x = torch.nn.functional.normalize(x, dim=1)
    return x.contiguous(), lab


def check_reg(x, y, labels, reg_in, got, h, alpha, momentum, exclude):
    # the derived per-row bound of float64_refs.usl_reg_ref on the scalars the kernel received (select.py rounds momentum and
    # 1 - momentum to fp32), for every row: none may be undecidable, which is a matter of the reference alone
    m32, omm32 = R.fp32_value(float(momentum)), R.fp32_value(float(1 - momentum))
    ref = R.usl_reg_ref(x, y, labels, reg_in, h, alpha, m32, omm32, exclude)
    assert int((~ref[2]).sum()) == 0, "%d rows are undecidable: the case does not test what it is there for" % int((~ref[2]).sum())
    over = ~R.usl_reg_within(got, ref)
    assert not bool(over.any()), (int(over.sum()), torch.where(over)[0][:8].tolist())
    # and the flat tolerance these tests started with, against the reference's own scalars
    want = regularizer64(x, y, labels, reg_in, h, alpha, momentum, exclude)
    rel = (got.double() - want).abs() / want.abs().clamp_min(1e-30)
    bad = torch.where(rel > RTOL)[0]
    if bad.numel() and h < y.shape[0]:
        # a row may miss only where its H-th and (H+1)-th float64 distances are a near-tie (the knn_lists_agree rule)
        v, _ = horizon_dists(x[bad], y, h + 1)
        tie = (v[:, h] - v[:, h - 1]) <= RTOL * v[:, h]
        bad = bad[~tie]
    assert bad.numel() == 0, (bad[:8].tolist(), rel[bad[:8]].tolist())


# (N, S, D, H, exclude, alpha, momentum): every value of the issue's lists appears at least once
RAGGED = [
    (1, 37, 16, 20, True, 1.0, 0.0),
    (127, 64, 384, 64, False, 0.5, 0.3),
    (3011, 300, 768, 32, True, 1.0, 0.3),
    (3011, 801, 384, 64, False, 1.0, 0.0),
    (127, 801, 768, 1, True, 0.5, 0.0),
    (3011, 20, 16, 20, False, 0.5, 0.3),
    (127, 300, 16, 32, False, 1.0, 0.0),
    (1, 1, 768, 1, False, 1.0, 0.3),
    (3011, 37, 768, 20, True, 0.5, 0.3),
]


@pytest.mark.parametrize("n,s,d,h,exclude,alpha,momentum", RAGGED)
def test_regularizer_ragged(H, n, s, d, h, exclude, alpha, momentum):
    from u2seg_amd.cluster.select import selection_regularizer

    x, lab = clustered(n + s, d, 7, seed=n * 31 + s * 7 + d + h)
    # the selected rows are rows of the data set at positions 0..S-1 with label = position (their own distance is masked
    # in the exclude mode); the other rows get labels in [0, S + 3), so some match no position at all
    g = torch.Generator(device=DEV)
    g.manual_seed(h)
    labels = torch.randint(0, s + 3, (n + s,), device=DEV, generator=g)
    labels[:s] = torch.arange(s, device=DEV)
    if not exclude and n > 2:
        x[s + 1] = x[0]  # a duplicate of a selected row: its zero distance is masked to 1e10
    y = x[:s].clone()
    reg_in = torch.rand(n + s, device=DEV, generator=g) * 3 if momentum else torch.zeros(n + s, device=DEV)
    got = selection_regularizer(x, y, labels, reg_in, h, alpha=alpha, momentum=momentum, exclude_same_cluster=exclude)
    assert got.dtype == torch.float32 and got.shape == (n + s,) and torch.isfinite(got).all()
    check_reg(x, y, labels, reg_in, got, h, alpha, momentum, exclude)
    with pytest.raises(ValueError):
        selection_regularizer(x, y[: h - 1], labels, reg_in, h) if h > 1 else selection_regularizer(x, y[:0], labels, reg_in, h)


def test_regularizer_duplicates(H):
    from u2seg_amd.cluster.select import selection_regularizer

    x, _ = clustered(500, 64, 5, seed=3)
    y = x[:40].clone()
    labels = torch.arange(500, device=DEV) % 40
    x[100] = x[7]  # row 100 (label 20) duplicates selected row 7
    reg0 = torch.zeros(500, device=DEV)
    # exclude False: every zero becomes 1e10, including the selected rows' own distances
    got = selection_regularizer(x, y, labels, reg0, 16, momentum=0.0, exclude_same_cluster=False)
    check_reg(x, y, labels, reg0, got, 16, 1.0, 0.0, False)
    # exclude True: rows 0..39 mask their own position; row 100's zero distance to position 7 stays: the reference raises
    labels[:40] = torch.arange(40, device=DEV)
    with pytest.raises(AssertionError):
        selection_regularizer(x, y, labels, reg0, 16, momentum=0.0, exclude_same_cluster=True)
    labels[100] = 7
    got = selection_regularizer(x, y, labels, reg0, 16, momentum=0.0, exclude_same_cluster=True)
    check_reg(x, y, labels, reg0, got, 16, 1.0, 0.0, True)
    # the empty set of rows
    assert selection_regularizer(x[:0], y, labels[:0], reg0[:0], 16).shape == (0,)


def test_full_size_selection(H):
    from u2seg_amd.cluster.select import get_selection_with_reg_imagenet, selection_regularizer

    n, s, d, h, w = 1_000_000, 800, 768, 32, 0.05
    x, _ = clustered(n, d, s, seed=11, unit=True)
    centers = torch.nn.functional.normalize(x[:s].clone(), dim=1)
    labels = torch.empty(n, dtype=torch.long, device=DEV)
    for i0 in range(0, n, 65536):
        labels[i0:i0 + 65536] = (x[i0:i0 + 65536] @ centers.T).argmax(1)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    nd = 0.5 + torch.rand(n, device=DEV, generator=g)
    kw = dict(final_sample_num=s, w=w, momentum=0.0, horizon_num=h, alpha=1.0, exclude_same_cluster=True)
    picks1 = get_selection_with_reg_imagenet(x, nd, labels, s, iters=1, **kw)
    k_used = int(torch.unique(labels).numel())
    assert len(picks1) == s == k_used
    assert picks1.tolist() == select_loop(nd, torch.zeros(n, device=DEV), labels, s, s, w)
    sel = torch.from_numpy(picks1).to(DEV)
    reg = selection_regularizer(x, x[sel], labels, torch.zeros(n, device=DEV), h, alpha=1.0, momentum=0.0,
                                exclude_same_cluster=True)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:2000].to(DEV)
    check_reg(x[rows], x[sel], labels[rows], torch.zeros(2000, device=DEV), reg[rows], h, 1.0, 0.0, True)
    picks2 = get_selection_with_reg_imagenet(x, nd, labels, s, iters=2, **kw)
    assert picks2.tolist() == select_loop(nd, reg, labels, s, s, w)
    assert (picks2 != picks1).any()


def test_cluster_instances_selection_end_to_end(H, tmp_path):
    from PIL import Image

    from u2seg_amd.cluster.knn import partitioned_kNN
    from u2seg_amd.cluster.select import get_selection_with_reg_imagenet

    npz = np.load(os.path.join(os.path.dirname(GOLDEN), "dino_golden.npz"))
    with open(os.path.join(os.path.dirname(GOLDEN), "dino_golden.json")) as f:
        meta = json.load(f)
    sc = float(npz["param_scale"])
    sd = {k: torch.from_numpy(npz["sd/" + k].astype(np.float32) / sc) for k in meta["tiny"]["keys"]}
    root = tmp_path / "crops" / "train"
    rng = np.random.default_rng(9)
    names = []
    for c in range(3):
        dd = root / ("cls%d" % c)
        dd.mkdir(parents=True)
        for i in range(20 + c):
            w, h = int(rng.integers(32, 80)), int(rng.integers(32, 80))
            arr = np.clip(rng.integers(0, 256, 3) + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
            fn = "%03d.png" % i
            Image.fromarray(arr, "RGB").save(str(dd / fn))
            names.append("cls%d/%s" % (c, fn))
    wpath = str(tmp_path / "tiny.pth")
    torch.save(sd, wpath)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("cluster_instances", os.path.join(repo, "tools", "cluster_instances.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["--crops", str(tmp_path / "crops"), "--weights", wpath, "--num-centroids", "4", "--niter", "20", "--knn-k", "5",
              "--batch", "8", "--workers", "0", "--size", "32"]
    plain = tmp_path / "plain"
    out = mod.run(mod.parse_args(common + ["--out", str(plain)]))
    assert len(out) == 4
    assert sorted(os.listdir(plain)) == sorted(["memory_feats_list.npy", "cluster_labels_4_0.npy", "centroids_4_0.npy",
                                                 "cluster_labels_decode.json"])
    sel_dir = tmp_path / "sel"
    feats, labels, _, _ = mod.run(mod.parse_args(common + ["--out", str(sel_dir), "--num-selected", "3", "--reg-horizon", "2",
                                                           "--reg-w", "0.5", "--reg-keep-same-cluster"]))
    got = np.load(sel_dir / "selected_indices_3_0.npy")
    saved = torch.from_numpy(np.load(sel_dir / "memory_feats_list.npy")).to(DEV)
    d_knns, _ = partitioned_kNN(saved, K=5)
    want = get_selection_with_reg_imagenet(saved, d_knns.mean(dim=1), labels, 4, iters=2, final_sample_num=3, w=0.5,
                                           momentum=0.0, horizon_num=2, alpha=1.0, exclude_same_cluster=False)
    assert got.dtype == np.int64 and got.tolist() == want.tolist()
    keys = sorted(names)  # dataset order is the sorted order here
    p = 0.2 * 3 / 2911
    sel_csv = sel_dir / ("train_%sp_gen_imagenet_usl_dino_0.2_index.csv" % p)
    rem_csv = sel_dir / ("train_%sp_gen_imagenet_usl_dino_0.2_index.csv" % (100 - p))
    assert open(sel_csv).read() == "Index,ImageID\n" + "".join("%d,%s\n" % (i, keys[i]) for i in sorted(got.tolist()))
    rem = [i for i in range(len(keys)) if i not in set(got.tolist())]
    assert open(rem_csv).read() == "Index,ImageID\n" + "".join("%d,%s\n" % (i, keys[i]) for i in rem)
    assert set(os.listdir(sel_dir)) == set(os.listdir(plain)) | {"selected_indices_3_0.npy", sel_csv.name, rem_csv.name}
