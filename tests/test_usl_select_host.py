"""USL's regularised selection without a GPU: the float64 oracle against the reference's recorded picks
(tests/golden/usl_select_golden.npz, make_usl_select_fixture.py), the file names and CSV bytes of the reference's
save_data, and the argument checks that run before any device work."""
import json
import os

import numpy as np
import pytest
import torch

from tests.usl_select_oracle import get_selection_with_reg64
from u2seg_amd.cluster import select

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "usl_select_golden.npz")


def load_cases():
    z = np.load(GOLDEN)
    meta = json.loads(str(z["cases"]))
    return z, meta["cases"]


def case_inputs(z, c):
    x = torch.from_numpy(z[c["name"] + "/x"] if c["name"] + "/x" in z.files else z["x"])
    return x, torch.from_numpy(z[c["name"] + "/nd"]), torch.from_numpy(z[c["name"] + "/labels"])


KW = ("iters", "final_sample_num", "w", "momentum", "horizon_num", "alpha", "exclude_same_cluster")


def test_fixture_covers_the_issue_cases():
    z, cases = load_cases()
    names = [c["name"] for c in cases]
    assert names == ["shipped", "iters3", "dup_keep", "truncate", "empty_last", "empty_mid", "empty_mid_keep", "collision",
                     "h_eq_s"]
    by = {c["name"]: c for c in cases}
    assert by["empty_mid"]["raises"] and not any(c["raises"] for c in cases if c["name"] != "empty_mid")
    r, p = by["dup_keep"]["dup"]
    xd = z["dup_keep/x"]
    labels = z["dup_keep/labels"]
    assert np.array_equal(xd[r], xd[p]) and labels[r] != labels[p]
    a, b = by["collision"]["collision"]
    nd = z["collision/nd"]
    assert a < b and nd[b] < nd[a] and np.float32(1) / nd[a] == np.float32(1) / nd[b]
    assert int(z["collision/picks"][3]) == a
    assert by["h_eq_s"]["horizon_num"] == by["h_eq_s"]["final_sample_num"]


@pytest.mark.parametrize("name", ["shipped", "iters3", "dup_keep", "truncate", "empty_last", "empty_mid", "empty_mid_keep",
                                  "collision", "h_eq_s"])
def test_oracle_reproduces_reference(name):
    z, cases = load_cases()
    c = next(c for c in cases if c["name"] == name)
    x, nd, labels = case_inputs(z, c)
    kw = {k: c[k] for k in KW}
    if c["raises"]:
        with pytest.raises(AssertionError):
            get_selection_with_reg64(x, nd, labels, c["num_centroids"], **kw)
        return
    picks = get_selection_with_reg64(x, nd, labels, c["num_centroids"], **kw)
    assert picks == z[name + "/picks"].tolist()


@pytest.mark.parametrize("s,seed,first,second", [
    (300, 0, "train_0.020611473720371008p_gen_imagenet_usl_dino_0.2_index.csv",
     "train_99.97938852627964p_gen_imagenet_usl_dino_0.2_index.csv"),
    (800, 1, "train_0.05496392992098935p_gen_imagenet_usl_dino_0.2_seed1_index.csv",
     "train_99.94503607007901p_gen_imagenet_usl_dino_0.2_seed1_index.csv"),
    (2911, 0, "train_0.2p_gen_imagenet_usl_dino_0.2_index.csv", "train_99.8p_gen_imagenet_usl_dino_0.2_index.csv"),
    (12820, 1, "train_1p_gen_imagenet_usl_dino_0.2_seed1_index.csv", "train_99p_gen_imagenet_usl_dino_0.2_seed1_index.csv"),
])
def test_sample_info_and_csv_names(s, seed, first, second):
    k, p = select.get_sample_info_imagenet(s)
    assert k == {12820: 12900}.get(s, s)
    assert select.split_csv_names(p, "imagenet_usl_dino_0.2", seed) == (first, second)


def test_csv_bytes_match_pandas(tmp_path):
    pd = pytest.importorskip("pandas")
    ids = ["n01/a.jpg", "n01/b,c.jpg", 'n02/say "hi".png', "n02/ünïcødé_日本.jpg", "n03/plain.JPEG", "n03/x y.jpg"]
    sel = np.array([4, 1, 3])
    a, b = select.save_split_csvs(str(tmp_path), sel, ids, 0.5, "run")
    assert os.path.basename(a) == "train_0.5p_gen_run_index.csv" and os.path.basename(b) == "train_99.5p_gen_run_index.csv"
    for path, rows in ((a, np.sort(sel)), (b, np.array([0, 2, 5]))):
        want = tmp_path / "want.csv"
        pd.DataFrame(data=[[int(i), ids[i]] for i in rows], columns=["Index", "ImageID"]).to_csv(str(want), index=False)
        assert open(path, "rb").read() == open(want, "rb").read()


def test_remainder_is_sorted_complement(tmp_path):
    ids = ["c/%d.jpg" % i for i in range(10)]
    a, b = select.save_split_csvs(str(tmp_path), np.array([7, 2, 5]), ids, 0.3, "r", seed=2)
    assert b.endswith("train_99.7p_gen_r_seed2_index.csv")
    lines = open(b).read().splitlines()
    assert lines[0] == "Index,ImageID"
    assert [int(l.split(",")[0]) for l in lines[1:]] == [0, 1, 3, 4, 6, 8, 9]
    assert open(a).read() == "Index,ImageID\n2,c/2.jpg\n5,c/5.jpg\n7,c/7.jpg\n"


@pytest.mark.parametrize("h", [0, 65, 256, -1, 2.0])
def test_horizon_out_of_range_raises_without_gpu(h):
    x = torch.zeros(4, 16)
    with pytest.raises(ValueError):
        select.get_selection_with_reg_imagenet(x, torch.ones(4), torch.zeros(4, dtype=torch.long), 1, iters=2,
                                               final_sample_num=1, horizon_num=h)
    with pytest.raises(ValueError):
        select.selection_regularizer(x, x[:1], torch.zeros(4, dtype=torch.long), torch.zeros(4), h)


def test_final_sample_num_none_raises_without_gpu():
    x = torch.zeros(4, 16)
    with pytest.raises(AssertionError):
        select.get_selection_with_reg_imagenet(x, torch.ones(4), torch.zeros(4, dtype=torch.long), 1, iters=2,
                                               horizon_num=1)


def test_horizon_above_selected_rows_raises_without_gpu():
    x = torch.zeros(4, 16)
    with pytest.raises(ValueError):
        select.selection_regularizer(x, x[:2], torch.zeros(4, dtype=torch.long), torch.zeros(4), 3)


def test_get_selection_saves_and_loads(tmp_path):
    fn = lambda *a, **k: np.array([3, 1], dtype=np.int64)  # noqa: E731
    got = select.get_selection(fn, final_sample_num=2, seed=0, run_dir=str(tmp_path))
    assert np.array_equal(np.load(tmp_path / "selected_indices_2_0.npy"), got)
    again = select.get_selection(None, final_sample_num=2, seed=0, recompute=False, run_dir=str(tmp_path))
    assert np.array_equal(again, got)
    select.get_selection(fn, final_sample_num=2, run_dir=str(tmp_path))
    assert os.path.exists(tmp_path / "selected_indices_2.npy")
