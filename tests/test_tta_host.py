"""Test-time augmentation on the host (u2seg_amd/modeling/test_time_augmentation.py): the mapper's views
and their order, the host definition of the device views against PIL, the float32 box maps, the descriptors the kernels are
given, and the configuration.  CPU only.

The merge itself (fast_rcnn_inference_single_image) ends in the HIP NMS kernel and cannot run without a GPU: its hand-made
cases are in tests/test_gpu_tta.py."""
import inspect

import numpy as np
import pytest
import torch
from torch import nn

from tests import tta_cases as C
from u2seg_amd.config import get_cfg
from u2seg_amd.data import device_mapper as dm
from u2seg_amd.data import transforms as T
from u2seg_amd.modeling import DatasetMapperTTA, GeneralizedRCNN, GeneralizedRCNNWithTTA, PanopticFPN
from u2seg_amd.modeling.test_time_augmentation import apply_box_f32, mean_in_view_order, view_descriptor


@pytest.mark.parametrize("pre_resize", [True, False])
def test_mapper_views_order_shapes_and_transforms(pre_resize):
    """6 views, size-major, the unflipped in front of the flipped; shapes by ResizeShortestEdge.get_output_shape (down-scaling,
    identity, and 80 -> 67 x 100 where MAX_SIZE binds); the transforms start at the ORIGINAL image when the input was resized."""
    inp = C.image_input(pre_resize)
    views = C.mapper()(inp)
    assert len(views) == 6
    want = []
    for s in C.MIN_SIZES:
        want += [T.ResizeShortestEdge.get_output_shape(54, 81, s, C.MAX_SIZE)] * 2
    assert want == C.VIEW_SHAPES
    src = inp["image"].permute(1, 2, 0).numpy()
    for k, (v, hw) in enumerate(zip(views, want)):
        assert tuple(v["image"].shape) == (3,) + hw and v["image"].dtype == torch.uint8
        assert (v["height"], v["width"]) == (inp["height"], inp["width"])
        kinds = [type(t) for t in v["transforms"].transforms]
        assert kinds == ([T.ResizeTransform] if pre_resize else []) + [T.ResizeTransform] + ([T.HFlipTransform] if k % 2 else [])
        first = v["transforms"].transforms[0]
        assert (first.h, first.w) == (inp["height"], inp["width"])
        plain = T.ResizeTransform(54, 81, hw[0], hw[1]).apply_image(src)
        assert np.array_equal(v["image"].numpy().transpose(1, 2, 0), plain[:, ::-1] if k % 2 else plain)
    assert torch.equal(inp["image"], C.image_input(pre_resize)["image"])   # the input is left alone
    # the geometry the device path takes from the mapper, without pixels
    tf = C.mapper().view_transforms((54, 81), (inp["height"], inp["width"]))
    for a, b in zip(tf, views):
        assert [type(t) for t in a.transforms] == [type(t) for t in b["transforms"].transforms]
        for s, t in zip(a.transforms, b["transforms"].transforms):
            assert vars(s) == vars(t)


def test_host_definition_of_the_device_views_equals_pil():
    """device_mapper.host_image over build_tables(h, w, H, W, hflip) - the host definition of u2_aug_resize_bilinear_u8 - equals
    the mapper's PIL view bit for bit: down-scaling, identity, up-scaling, each unflipped and flipped."""
    inp = C.image_input()
    src = inp["image"].permute(1, 2, 0).numpy()
    for k, v in enumerate(C.mapper()(inp)):
        H, W = v["image"].shape[1:]
        got = dm.host_image(src, dm.build_tables(54, 81, H, W, hflip=bool(k % 2)))
        assert np.array_equal(got, v["image"].numpy()), k


def test_box_maps_are_float32_and_not_exact():
    """apply_box_f32: float32 in, float32 out; it differs from a float64 evaluation of the same chain (the dtype matters);
    forward after inverse returns within a few ulp - NOT the same bits: four multiplications and, in a flipped view, two
    subtractions, each rounded once, so |difference| <= 8 * 2^-24 * (the largest coordinate met on the way, at most twice the
    largest image edge here) - and a flipped view swaps x0 and x1."""
    rs = np.random.RandomState(0)
    differs = False
    for im, tfm in C.box_views():
        h, w = C.BOX_CLIP[im]
        boxes = C.random_boxes(rs, 64, h, w, special=False)
        fwd = apply_box_f32(tfm, boxes)
        assert fwd.dtype == np.float32 and fwd.shape == boxes.shape
        wide = T.TransformList(tfm.transforms).apply_box(boxes.astype(np.float64))
        assert np.allclose(fwd, wide, rtol=1e-6, atol=1e-4)
        differs |= bool((fwd != wide.astype(np.float32)).any())
        back = apply_box_f32(tfm, fwd, inverse=True)
        scale = 2.0 * max(h, w, *C.view_size(tfm))
        assert np.abs(back.astype(np.float64) - boxes).max() <= 8 * 2.0 ** -24 * scale
        assert (fwd[:, 0] <= fwd[:, 2]).all() and (fwd[:, 1] <= fwd[:, 3]).all()
        if any(isinstance(t, T.HFlipTransform) for t in tfm.transforms):
            unflipped = apply_box_f32(T.TransformList(tfm.transforms[:-1]), boxes)
            vw = np.float32(C.view_size(tfm)[1])
            assert np.array_equal(fwd[:, 0], vw - unflipped[:, 2]) and np.array_equal(fwd[:, 2], vw - unflipped[:, 0])
            assert np.array_equal(fwd[:, [1, 3]], unflipped[:, [1, 3]])
    assert differs, "the float32 chain equals the float64 one everywhere: the case no longer guards the dtype"
    with pytest.raises(AssertionError):
        apply_box_f32(C.box_views()[0][1], np.zeros((1, 4), dtype=np.float64))


def _chain_like_the_kernels(desc, flip, boxes, inverse):
    """The step order of csrc/tta.hip in numpy float32, from a view descriptor."""
    b = boxes.copy()

    def corners(x0, x1, y0, y1):   # every step ends in the bounding box of the mapped corners
        b[:, 0], b[:, 2] = np.minimum(x0, x1), np.maximum(x0, x1)
        b[:, 1], b[:, 3] = np.minimum(y0, y1), np.maximum(y0, y1)

    def do_flip():
        corners(desc[4] - b[:, 0], desc[4] - b[:, 2], b[:, 1], b[:, 3])

    if inverse and flip:
        do_flip()
    for sx, sy in ((desc[0], desc[1]), (desc[2], desc[3])):
        corners(b[:, 0] * sx, b[:, 2] * sx, b[:, 1] * sy, b[:, 3] * sy)
    if not inverse and flip:
        do_flip()
    return b


@pytest.mark.parametrize("inverse", [False, True])
def test_view_descriptors_restate_the_transform_chain(inverse):
    """view_descriptor: two float32 scale pairs (1.0 where a step is absent), the flip and the view width; the kernels' order
    of steps over them gives apply_box_f32 bit for bit, in both directions."""
    rs = np.random.RandomState(1)
    for im, tfm in C.box_views():
        desc, flip = view_descriptor(tfm, inverse=inverse)
        assert desc.dtype == np.float32 and desc.shape == (5,)
        assert flip == int(any(isinstance(t, T.HFlipTransform) for t in tfm.transforms))
        resizes = [t for t in tfm.transforms if isinstance(t, T.ResizeTransform)]
        if len(resizes) == 1:
            assert desc[2] == 1.0 and desc[3] == 1.0
        if flip:
            assert desc[4] == C.view_size(tfm)[1]
        h, w = C.view_size(tfm) if inverse else C.BOX_CLIP[im]
        boxes = C.random_boxes(rs, 257, h, w)   # with a NaN and an inf row
        assert np.array_equal(_chain_like_the_kernels(desc, flip, boxes, inverse), apply_box_f32(tfm, boxes, inverse=inverse),
                              equal_nan=True)
    with pytest.raises(NotImplementedError):
        view_descriptor(T.TransformList([T.HFlipTransform(10), T.ResizeTransform(5, 10, 10, 20)]))


def test_mean_in_view_order_is_the_sequential_sum():
    for images in C.REDUCE_CASES:
        probs, _ = C.reduce_case(images, 7)
        for views in probs:
            want = C.reduce_expected([views], [[0] * len(views)])
            got = mean_in_view_order(views)
            assert torch.equal(got, want)
            exact = C.reduce_exact_mean([views], [[0] * len(views)])
            if got.numel():
                assert float((got.double() - exact).abs().max()) <= len(views) * 2.0 ** -24


def _blank_rcnn(cls=GeneralizedRCNN):
    model = cls.__new__(cls)
    nn.Module.__init__(model)
    return model


def test_config_reaches_the_mapper_and_the_wrapper_refuses_what_it_cannot_do():
    cfg = get_cfg()
    cfg.merge_from_list(["TEST.AUG.MIN_SIZES", (32, 54, 80), "TEST.AUG.MAX_SIZE", 100, "TEST.AUG.FLIP", False])
    m = DatasetMapperTTA(cfg)
    assert (list(m.min_sizes), m.max_size, m.flip) == ([32, 54, 80], 100, False)
    assert len(m(C.image_input())) == 3
    d = DatasetMapperTTA(get_cfg())
    assert len(d.min_sizes) == 9 and d.max_size == 4000 and d.flip is True   # the reference's defaults: 18 views
    for cls in (GeneralizedRCNN, PanopticFPN):
        w = GeneralizedRCNNWithTTA(cfg, _blank_rcnn(cls))
        assert w.batch_size == 3 and w.impl == "device" and w.keep_features and isinstance(w.tta_mapper, DatasetMapperTTA)
        assert w.tta_mapper.flip is False
    assert GeneralizedRCNNWithTTA(cfg, _blank_rcnn(), impl="host", batch_size=2).batch_size == 2
    with pytest.raises(ValueError):
        GeneralizedRCNNWithTTA(cfg, _blank_rcnn(), impl="eager")
    with pytest.raises(AssertionError):
        GeneralizedRCNNWithTTA(cfg, nn.Linear(1, 1))
    for key in ("MODEL.KEYPOINT_ON", "MODEL.LOAD_PROPOSALS"):
        bad = get_cfg()
        bad.merge_from_list([key, True])
        with pytest.raises(AssertionError):
            GeneralizedRCNNWithTTA(bad, _blank_rcnn())
    with pytest.raises(NotImplementedError):   # the device views are DatasetMapperTTA's
        GeneralizedRCNNWithTTA(cfg, _blank_rcnn(), tta_mapper=lambda d: [d])
    GeneralizedRCNNWithTTA(cfg, _blank_rcnn(), tta_mapper=lambda d: [d], impl="host")


def test_inference_signature_is_the_reference_s():
    """GeneralizedRCNN.inference(batched_inputs, detected_instances=None, do_postprocess=True); PanopticFPN keeps its own."""
    p = list(inspect.signature(GeneralizedRCNN.inference).parameters.values())
    assert [q.name for q in p] == ["self", "batched_inputs", "detected_instances", "do_postprocess"]
    assert p[2].default is None and p[3].default is True
    assert [q for q in inspect.signature(PanopticFPN.inference).parameters] == ["self", "batched_inputs", "do_postprocess"]
    model = _blank_rcnn()
    model.eval()
    with pytest.raises(TypeError):   # the old second positional argument is not silently taken for instances
        model.inference([], False)


def test_device_path_has_no_host_fallback():
    cfg = get_cfg()
    model = _blank_rcnn()
    model.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    model.eval()
    w = GeneralizedRCNNWithTTA(cfg, model, impl="device")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        w([C.image_input()])
