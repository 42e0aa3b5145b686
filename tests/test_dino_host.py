"""Host side of the DINO feature extractor (u2seg_amd/cluster/dino.py, u2seg_amd/data/crops.py), on the CPU: state-dict names
and shapes, strict loading, positional-embedding interpolation and the fp32 restatement of the reference forward against the
reference's own outputs (tests/golden/dino_golden.*, written by make_dino_fixture.py), the ImageFolder order, the Resize /
CenterCrop sizes and the JSON key form."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from u2seg_amd.cluster import dino
from u2seg_amd.data import crops


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "dino_golden.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, "dino_golden.npz"))


def tiny_model(meta, npz):
    t = meta["tiny"]
    m = dino.DinoViT(img_size=t["img_size"], patch_size=t["patch_size"], embed_dim=t["embed_dim"], depth=t["depth"],
                     num_heads=t["num_heads"], mlp_ratio=4, qkv_bias=True,
                     norm_layer=lambda d: torch.nn.LayerNorm(d, eps=t["eps"]))
    s = float(npz["param_scale"])
    sd = {k: torch.from_numpy(npz["sd/" + k].astype(np.float32) / s) for k in t["keys"]}
    m.load_state_dict(sd, strict=True)
    return m.eval(), sd


def test_vit_base8_names_and_shapes(golden):
    meta, _ = golden
    got = {k: list(v.shape) for k, v in dino.vit_base(patch_size=8).state_dict().items()}
    assert got == meta["vit_base8"]
    assert list(got.keys()) == list(meta["vit_base8"].keys())


def test_tiny_names_match_reference(golden):
    meta, npz = golden
    m, _ = tiny_model(meta, npz)
    assert list(m.state_dict().keys()) == meta["tiny"]["keys"]


def test_strict_loading(golden, tmp_path):
    meta, npz = golden
    _, sd = tiny_model(meta, npz)
    path = str(tmp_path / "tiny.pth")
    torch.save(sd, path)
    m = dino.load_dino_weights(path)  # architecture from the checkpoint
    assert (m.embed_dim, len(m.blocks), m.num_heads, m.patch_embed.patch_size) == (128, 2, 2, 8)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    bad = dict(sd)
    bad["head.weight"] = torch.zeros(4, 128)
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        dino.load_dino_weights(path)
    missing = dict(sd)
    del missing["norm.bias"]
    torch.save(missing, path)
    with pytest.raises(RuntimeError, match="Missing key"):
        dino.load_dino_weights(path, model=dino.build_from_state_dict(sd))


def test_pos_embed_interpolation(golden):
    meta, npz = golden
    m, _ = tiny_model(meta, npz)
    p = meta["tiny"]["patch_size"]
    for h, w in meta["tiny"]["sizes"]:
        got = m.interpolate_pos_encoding((h // p) * (w // p), h, w)
        ref = torch.from_numpy(npz["pos_%dx%d" % (h, w)])
        assert got.shape == ref.shape
        torch.testing.assert_close(got, ref, rtol=0, atol=1e-6)
        assert m.interpolate_pos_encoding((h // p) * (w // p), h, w) is got  # cached
    # the checkpoint's own grid is returned unchanged
    n = m.pos_embed.shape[1] - 1
    assert torch.equal(m.interpolate_pos_encoding(n, 32, 32), m.pos_embed.detach())


def test_reference_restatement_matches_reference(golden):
    """dino.reference_forward (the yardstick of the GPU tests) equals the reference's fp32 forward on the CPU."""
    meta, npz = golden
    m, _ = tiny_model(meta, npz)
    xs = float(npz["input_scale"])
    for h, w in meta["tiny"]["sizes"]:
        x = torch.from_numpy(npz["x_%dx%d" % (h, w)].astype(np.float32) / xs)
        ref = torch.from_numpy(npz["y_%dx%d" % (h, w)])
        got = dino.reference_forward(m, x)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


def _save(path, size, mode="RGB", seed=0):
    rng = np.random.default_rng(seed)
    w, h = size
    if mode == "L":
        Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L").save(path)
    else:
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(path)


def test_image_folder_order(tmp_path):
    root = tmp_path / "train"
    (root / "b_cls" / "sub").mkdir(parents=True)
    (root / "a_cls").mkdir(parents=True)
    (root / "B_upper").mkdir()
    _save(root / "a_cls" / "z.png", (20, 30))
    _save(root / "a_cls" / "A.PNG", (30, 20))
    _save(root / "a_cls" / "m.JPEG", (17, 17))
    (root / "a_cls" / "notes.txt").write_text("not an image")
    _save(root / "b_cls" / "x.bmp", (9, 40), mode="L")
    _save(root / "b_cls" / "sub" / "c.png", (41, 9))
    _save(root / "B_upper" / "q.Tif", (12, 12))
    ds = crops.CropFolder(str(root), size=8)
    assert ds.classes == ["B_upper", "a_cls", "b_cls"]
    rel = [os.path.relpath(p, str(root)) for p, _ in ds.samples]
    assert rel == ["B_upper/q.Tif", "a_cls/A.PNG", "a_cls/m.JPEG", "a_cls/z.png", "b_cls/x.bmp", "b_cls/sub/c.png"]
    assert ds.targets == [0, 1, 1, 1, 2, 2]
    assert ds.keys() == ["B_upper/q.Tif", "a_cls/A.PNG", "a_cls/m.JPEG", "a_cls/z.png", "b_cls/x.bmp", "sub/c.png"]
    img, t = ds[4]
    assert img.dtype == torch.uint8 and tuple(img.shape) == (8, 8, 3) and t == 2
    # grayscale converts to RGB: the three channels are equal
    assert torch.equal(img[..., 0], img[..., 1]) and torch.equal(img[..., 1], img[..., 2])
    batch = next(iter(crops.crop_loader(ds, batch_size=4, workers=0)))
    assert tuple(batch[0].shape) == (4, 8, 8, 3) and batch[1].tolist() == [0, 1, 1, 1]


@pytest.mark.parametrize("w,h,exp", [
    (640, 480, (640, 480)),     # already the target size: unchanged
    (500, 375, (640, 480)),     # landscape: short side 480, long int(480 * 500 / 375) = 640
    (375, 500, (480, 640)),     # portrait
    (333, 517, (480, 745)),     # int(480 * 517 / 333) = 745.22 -> 745
    (517, 333, (745, 480)),
    (1001, 999, (480, 480)),    # int(480 * 1001 / 999) = 480.96 -> 480
    (100, 100, (480, 480)),
])
def test_resize_size(w, h, exp):
    assert crops.resize_size(w, h, 480) == exp


def test_center_crop_box():
    assert crops.center_crop_box(745, 480, 480) == (132, 0, 612, 480)    # round(132.5) = 132 (half to even)
    assert crops.center_crop_box(480, 747, 480) == (0, 134, 480, 614)    # round(133.5) = 134
    assert crops.center_crop_box(480, 480, 480) == (0, 0, 480, 480)


def test_load_crop_matches_pil_steps(tmp_path):
    path = str(tmp_path / "p.png")
    _save(path, (37, 53), seed=3)
    got = crops.load_crop(path, size=24)
    img = Image.open(path).convert("RGB").resize((24, int(24 * 53 / 37)), Image.BILINEAR)
    top = int(round((img.size[1] - 24) / 2.0))
    ref = np.asarray(img.crop((0, top, 24, top + 24)))
    assert got.shape == (24, 24, 3) and np.array_equal(got, ref)


def test_json_key_form():
    assert crops.sample_key("/data/crops/train/person/123.jpg") == "person/123.jpg"
    assert crops.sample_key("rel/cls/a.png") == "cls/a.png"
