"""Polygon ground truth on the GPU (u2seg_amd/csrc/polygon.hip through u2seg_amd/evaluation/mask_ops.py) against the host
definition u2seg_amd/data/polygon.py: plane bits, padding bits and areas, then the intersections, the synchronisation budget
and the evaluator.  Everything is integers: every comparison is ==."""
import math

import numpy as np
import pytest
import torch

from tests import polygon_cases as PC
from u2seg_amd.data import polygon, rle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.evaluation import mask_ops

    _hip.load()
    return mask_ops


def ann(polys):
    return {"id": 0, "segmentation": polys}


def check_planes(M, anns_per_image, sizes):
    """One call of planes_from_annotations for the batch; every plane (bits and padding) and every area == the definition.
    Returns the masks per image, in annotation order."""
    planes, descs, info = M.planes_from_annotations(anns_per_image, sizes, torch.device(DEV))
    host = planes.cpu().numpy()
    area = info["area"].copy()
    area[info["poly_rows"]] = info["poly_area"].cpu().numpy()
    out = []
    for i, ((h, w), anns) in enumerate(zip(sizes, anns_per_image)):
        d, order = descs[i], info["order"][i]
        assert d.n == len(anns) and sorted(order) == list(range(len(anns)))
        nw = d.n * w * M.words_per_column(h)
        got, padding = M.unpack_planes(host[d.plane_offset : d.plane_offset + nw], d.n, h, w)
        assert not padding.any(), i
        masks = np.zeros((len(anns), h, w), dtype=np.uint8)
        for j, k in enumerate(order):
            want = M.gt_mask(anns[k], h, w)
            assert np.array_equal(got[j], want), (i, k, int(got[j].sum()), int(want.sum()))
            assert int(area[d.first + j]) == int(want.sum()), (i, k)
            masks[k] = want
        out.append(masks)
    return out


def test_known_answers_in_one_ragged_batch(M):
    cases = PC.known_answers()
    masks = check_planes(M, [[ann(c["polygons"])] for c in cases], [(c["h"], c["w"]) for c in cases])
    for c, m in zip(cases, masks):
        assert int(m.sum()) == c["area"], c["name"]
        if c["counts"] is not None:
            assert np.array_equal(m[0], rle.decode({"size": [c["h"], c["w"]], "counts": c["counts"]})), c["name"]


def test_small_sizes_and_the_image_border(M):
    """Sizes around the word length, polygons wholly outside each side, and polygons whose lower edge lies on y = h: in the last
    column the toggle at position x h + h is dropped, in an inner column it is carried into bit 0 of the next column."""
    rs = np.random.RandomState(3)
    anns, sizes = [], []
    for h, w in ((1, 1), (1, 7), (7, 1), (63, 5), (64, 5), (65, 5), (128, 3), (37, 21)):
        per = [ann([[-3, -3, w + 3, -3, w + 3, h + 3, -3, h + 3]]),                      # covers the image
               ann([[-9, 1, -2, 1, -2, h - .5, -9, h - .5]]),                            # left of it
               ann([[w + 1, 0, w + 6, 0, w + 6, h, w + 1, h]]),                          # right of it
               ann([[0, -8, w, -8, w, -1.5, 0, -1.5]]),                                  # above
               ann([[0, h + 1.5, w, h + 1.5, w, h + 9, 0, h + 9]]),                      # below
               ann([[w - 1, h - 1, w, h - 1, w, h, w - 1, h]]),                          # the last pixel: touches y = h in the last column
               ann([[0, 0, .6 * w, 0, .6 * w, h, 0, h]]),                                # touches y = h in inner columns
               ann([[.3, h - .4, w - .3, h + 2, w * .5, .2]]),
               ann([PC.blob_polygon(rs, h, w, 9)]),
               ann([])]                                                                  # no polygon at all: an empty mask
        anns.append(per)
        sizes.append((h, w))
    masks = check_planes(M, anns, sizes)
    for (h, w), m in zip(sizes, masks):
        assert m[0].all() and not m[1:5].any() and not m[9].any()
        assert m[5].sum() == 1 and m[5][h - 1, w - 1] == 1


def test_more_vertices_than_a_work_group(M):
    """A circle of radius 40 with 3 000 vertices in 100 x 100: 12 tiles of edges, most edges shorter than a grid step."""
    t = np.arange(3000) * (2 * math.pi / 3000)
    xy = np.stack([50.2 + 40 * np.cos(t), 49.7 + 40 * np.sin(t)], axis=1).reshape(-1).tolist()
    m = check_planes(M, [[ann([xy])]], [(100, 100)])[0][0]
    assert abs(int(m.sum()) - math.pi * 1600) < 40 and m[50, 50] and not m[5, 5]


def test_one_long_edge_among_many_short_ones_at_full_size(M):
    """800 x 1333 (21-word columns): an edge of 1 300 px, then 200 edges of under 1 px back along a wavy line."""
    xs = 1310 - np.arange(201) * 0.6
    ys = 420 + np.sin(np.arange(201) * 0.5)
    xy = [10.3, 390.6, 1310.0, 402.2] + np.stack([xs, ys], axis=1).reshape(-1).tolist() + [700.5, 799.9, 10.3, 640.0]
    assert max(math.hypot(a - c, b - d) for a, b, c, d in zip(xs[:-1], ys[:-1], xs[1:], ys[1:])) < 1
    m = check_planes(M, [[ann([xy])]], [(800, 1333)])[0][0]
    assert m.sum() > 100000 and m[799, 700]


def test_union_of_overlapping_polygons(M):
    rs = np.random.RandomState(4)
    h, w = 70, 90
    polys = [PC.blob_polygon(rs, h, w, 12) for _ in range(4)] + [[5, 5, 60, 5, 60, 50, 5, 50]]
    polys[1] = polys[0]  # the same ring twice as two polygons: union, not parity
    m = check_planes(M, [[ann(polys), ann(polys[:1]), ann(polys[::-1])]], [(h, w)])[0]
    single = [polygon.polygon_to_mask(p, h, w) for p in polys]
    assert np.array_equal(m[0], np.bitwise_or.reduce(single)) and m[0].sum() < sum(s.sum() for s in single)
    assert np.array_equal(m[0], m[2])


def mixed_batch(rs):
    """6 images: no annotation, RLE only, polygons only, mixed in interleaved order (twice, one at the full size), polygons."""
    sizes = [(33, 45), (65, 67), (129, 40), (200, 300), (480, 640), (64, 64)]
    kinds = ["", "RRR", "PPPP", "PRPRRP", "RPPRP", "PP"]
    anns = []
    for (h, w), kind in zip(sizes, kinds):
        per = []
        for k, c in enumerate(kind):
            if c == "R":
                yy, xx = np.mgrid[0:h, 0:w]
                cx, cy = rs.uniform(0, w), rs.uniform(0, h)
                seg = rle.encode(((xx - cx) / (w / 3.0)) ** 2 + ((yy - cy) / (h / 3.0)) ** 2 <= 1)
                if k % 2:
                    seg = {"size": [h, w], "counts": rle.counts_of(seg)}  # a crowd region as COCO stores it
            else:
                seg = [PC.blob_polygon(rs, h, w, rs.randint(3, 60)) for _ in range(rs.randint(1, 4))]
            per.append({"id": 100 * len(anns) + k, "iscrowd": int(c == "R" and k % 2), "segmentation": seg})
        anns.append(per)
    return sizes, anns


def test_mixed_batch_intersections_and_sync_budget(M):
    rs = np.random.RandomState(6)
    sizes, anns = mixed_batch(rs)
    gt_masks = check_planes(M, anns, sizes)
    dets = [rs.rand(rs.randint(1, 6), h, w) < 0.5 for h, w in sizes]
    dets[2] = np.zeros((0,) + sizes[2], dtype=bool)
    tensors = [torch.from_numpy(d).to(DEV) for d in dets]
    before = dict(M.counters)
    out = M.mask_batch(tensors, gt=anns)
    used = {k: M.counters[k] - before[k] for k in before}
    for res, d, g in zip(out, dets, gt_masks):
        want = (d[:, None] & g[None].astype(bool)).sum(axis=(2, 3), dtype=np.int64)
        assert res["inter"].dtype == np.int64 and np.array_equal(res["inter"], want)
        assert np.array_equal(res["area_gt"], g.sum(axis=(1, 2))) and np.array_equal(res["area"], d.sum(axis=(1, 2)))
    # the same batch with every ground truth as RLE, through the parent's route: equal counts, equal budget
    counts = [[rle.counts_of(rle.encode(m)) for m in g] for g in gt_masks]
    before = dict(M.counters)
    ref = M.mask_batch(tensors, counts)
    assert used == {k: M.counters[k] - before[k] for k in before} == {"host_syncs": 2, "d2h_transfers": 2}
    for a, b in zip(out, ref):
        assert a["rles"] == b["rles"] and np.array_equal(a["inter"], b["inter"])
    host = M.mask_batch_any([t.cpu() for t in tensors], gt=anns)
    for a, b in zip(out, host):
        assert np.array_equal(a["inter"], b["inter"]) and np.array_equal(a["area_gt"], b["area_gt"])
    one = M.mask_pair_counts(tensors[3], anns[3], *sizes[3], polygons=True)
    assert np.array_equal(one[0], out[3]["inter"]) and np.array_equal(one[2], out[3]["area_gt"])


def test_launcher_checks_its_arguments(M):
    from u2seg_amd import _hip

    pm = (M._PolyMask * 1)()
    pm[0].H, pm[0].W, pm[0].num_polys = 8, 8, 2
    planes = torch.zeros(8, dtype=torch.int64, device=DEV)
    xy = torch.zeros(8, dtype=torch.float64, device=DEV)
    offs = torch.tensor([0, 2, 4], dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="status -1"):  # two polygons need 8 scratch words
        _hip.call("u2_mask_planes_from_polygons", xy, offs, pm, 1, planes, None, None, 0)
    pm[0].H = -1
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_mask_planes_from_polygons", xy, offs, pm, 1, planes, None, planes, 8)
    pm[0].H, pm[0].W = 1 << 16, 1 << 15
    with pytest.raises(RuntimeError, match="status -1"):
        _hip.call("u2_mask_planes_from_polygons", xy, offs, pm, 1, planes, None, planes, 8)
    with pytest.raises(ValueError, match="within"):
        M.planes_from_annotations([[ann([[0, 0, 1e9, 0, 5, 5]])]], [(8, 8)], torch.device(DEV))


def test_evaluator_device_equals_host(M, tmp_path, monkeypatch):
    """COCOEvaluator(gt_polygons="rasterize") fed device Instances == the same Instances on the host."""
    from tests.test_polygon_host import same_with_nans, tiny_polygon_dataset
    from u2seg_amd.evaluation import COCOEvaluator

    inputs, outputs = tiny_polygon_dataset(tmp_path, monkeypatch, names=("tiny_poly_gpu", "tiny_poly_gpu_as_rle"))
    results = {}
    for where in ("host", "device"):
        ev = COCOEvaluator("tiny_poly_gpu", output_dir="out_" + where, mode="eval", tasks=("bbox", "segm"), gt_polygons="rasterize")
        outs = outputs if where == "host" else [{"instances": o["instances"].to(DEV)} for o in outputs]
        for k in range(0, len(inputs), 2):
            ev.process(inputs[k : k + 2], outs[k : k + 2])
        results[where] = (ev._predictions, ev.evaluate())
    (pa, ra), (pb, rb) = results["host"], results["device"]
    for a, b in zip(pa, pb):
        assert a["image_id"] == b["image_id"] and a["instances"] == b["instances"]
        for key in ("inter", "area_dt", "area_gt"):
            assert np.array_equal(a["segm_pairs"][key], b["segm_pairs"][key]), key
    assert ra["segm"]["AP"] > 0
    same_with_nans(ra["bbox"], rb["bbox"])
    same_with_nans(ra["segm"], rb["segm"])
    assert set(ra) == set(rb) == {"bbox", "segm"}
