"""Test-time augmentation for instance inference (detectron2/modeling/test_time_augmentation.py:29-307).

`DatasetMapperTTA` turns one input into its resized (and flipped) views, `GeneralizedRCNNWithTTA` detects on every view, maps
the boxes back, merges them with one NMS, asks every view for the masks of the merged boxes and averages those.

The wrapper has two implementations of the same definition:

  impl="host"    the reference's lines restated from existing pieces: PIL views (data/transforms.py), boxes mapped with numpy
                 in float32 with a device <-> host round trip per view, a dense [N, K + 1] score matrix for
                 fast_rcnn_inference_single_image, one image at a time.  This is the definition and the yardstick.
  impl="device"  all views of an image from one call of u2_aug_resize_bilinear_u8 (V descriptors on one source), the box
                 maps and the mask mean in csrc/tta.hip for all images of the call in one launch each, the merge without the
                 dense matrix, and the FPN maps of the detection pass kept for the mask pass (keep_features).

Both give the same bits (tests/test_gpu_tta.py).  Two things are pinned down that the reference leaves open:

  * box coordinates are float32 all the way: fvcore's apply_box keeps the dtype of the array it is given, so every resize step
    is x * fl32(new_w * 1.0 / w) and every flip fl32(width) - x, rounded to float32 once per step (`apply_box_f32`);
  * the mask mean is a sequential float32 sum in view order and one division by float(V) (`mean_in_view_order`); torch.mean
    leaves the order open, either order is within V * 2^-24 of the exact mean for probabilities in [0, 1].

Keypoints and semantic / panoptic outputs are not augmented (the reference's wrapper returns instances only)."""
import copy
from contextlib import contextmanager

import numpy as np
import torch
from torch import nn

from ..config import configurable
from ..data import transforms as T
from ..structures import Boxes, Instances
from .batched import _PinnedRing, device_upload
from .inference import detector_postprocess, detector_postprocess_batch, fast_rcnn_inference_single_image
from .panoptic_fpn import GeneralizedRCNN

__all__ = ["DatasetMapperTTA", "GeneralizedRCNNWithTTA", "apply_box_f32", "mean_in_view_order"]

MERGE_SCORE_THRESH = 1e-8  # test_time_augmentation.py:275
_BOX_CORNERS = np.array([0, 1, 2, 1, 0, 3, 2, 3])


# ---- the float32 box maps (host definition) -----------------------------------------------------------------------------------
def _inverse(t):
    """Transform.inverse() of the transforms a view is made of (transform.py:156-160; a flip is its own inverse)."""
    if isinstance(t, T.ResizeTransform):
        return T.ResizeTransform(t.new_h, t.new_w, t.h, t.w, t.interp)
    if isinstance(t, (T.HFlipTransform, T.NoOpTransform)):
        return t
    raise NotImplementedError("test-time augmentation maps boxes through resizes and horizontal flips, not %s" % type(t).__name__)


def _steps(transforms, inverse=False):
    """The members of a TransformList in the order they are applied (inverse: the inverses, last first)."""
    members = list(transforms.transforms if isinstance(transforms, T.TransformList) else [transforms])
    return [_inverse(t) for t in reversed(members)] if inverse else members


def apply_box_f32(transforms, boxes, inverse=False):
    """TransformList.apply_box (inverse: TransformList.inverse().apply_box) on a float32 array, as fvcore computes it: every
    member maps the four corners of the box it is given and takes their bounding box; the coordinates stay float32, so a resize
    multiplies by the float32 rounding of its float64 scale and a flip subtracts from float32(width).

    Not exact: forward after inverse returns a box within a few ulp of the one that went in, not the same bits."""
    boxes = np.asarray(boxes)
    assert boxes.dtype == np.float32, "the reference maps the float32 boxes the model predicted (got %s)" % boxes.dtype
    boxes = boxes.reshape(-1, 4)
    for t in _steps(transforms, inverse):
        c = boxes[:, _BOX_CORNERS].reshape(-1, 2).copy()
        if isinstance(t, T.ResizeTransform):
            c[:, 0] = c[:, 0] * np.float32(t.new_w * 1.0 / t.w)
            c[:, 1] = c[:, 1] * np.float32(t.new_h * 1.0 / t.h)
        elif isinstance(t, T.HFlipTransform):
            c[:, 0] = np.float32(t.width) - c[:, 0]
        elif not isinstance(t, T.NoOpTransform):
            raise NotImplementedError("test-time augmentation maps boxes through resizes and horizontal flips, not %s"
                                      % type(t).__name__)
        c = c.reshape(-1, 4, 2)
        boxes = np.concatenate([c.min(axis=1), c.max(axis=1)], axis=1)
    return boxes


def view_descriptor(transforms, inverse=False):
    """A view's transforms as the kernels of csrc/tta.hip take them: ((s1x, s1y, s2x, s2y, width) float32, flip).  Forward: the
    scales in order, then the flip; inverse: the flip, then the inverse scales (1.0 where a step is absent)."""
    scales, flip, width = [], 0, 0.0
    steps = _steps(transforms, inverse)
    for k, t in enumerate(steps):
        if isinstance(t, T.ResizeTransform):
            scales.append((np.float32(t.new_w * 1.0 / t.w), np.float32(t.new_h * 1.0 / t.h)))
        elif isinstance(t, T.HFlipTransform):
            if flip or k != (0 if inverse else len(steps) - 1):
                raise NotImplementedError("the device maps take one horizontal flip, behind the resizes of the view")
            flip, width = 1, float(t.width)
    if len(scales) > 2:
        raise NotImplementedError("the device maps take at most two resizes per view (input and view)")
    scales += [(np.float32(1.0), np.float32(1.0))] * (2 - len(scales))
    return np.array([scales[0][0], scales[0][1], scales[1][0], scales[1][1], width], dtype=np.float32), flip


def mean_in_view_order(masks):
    """The mean of a list of float32 tensors as a sequential sum in list order and one division by float(V)."""
    acc = masks[0]
    for m in masks[1:]:
        acc = acc + m
    # a one-element tensor, not a Python number: for a host scalar torch's device kernel multiplies by the reciprocal
    return acc / torch.full((1,), float(len(masks)), dtype=acc.dtype, device=acc.device)


# ---- the mapper -----------------------------------------------------------------------------------------------------------------
class DatasetMapperTTA:
    """A callable from one input dict (standard model input format) to the list of its augmented versions:
    len(min_sizes) * (2 if flip else 1) dicts, size-major, the unflipped view in front of the flipped one.  Every dict carries
    "transforms", the TransformList from the ORIGINAL image (height x width of the dict) to the view."""

    @configurable
    def __init__(self, min_sizes, max_size, flip):
        self.min_sizes, self.max_size, self.flip = list(min_sizes), max_size, flip

    @classmethod
    def from_config(cls, cfg):
        return {"min_sizes": cfg.TEST.AUG.MIN_SIZES, "max_size": cfg.TEST.AUG.MAX_SIZE, "flip": cfg.TEST.AUG.FLIP}

    def view_transforms(self, shape, orig_shape):
        """The TransformLists of all views of an input of `shape` (h, w) whose original image has `orig_shape`; no pixels."""
        h, w = shape
        pre = T.ResizeTransform(orig_shape[0], orig_shape[1], h, w) if tuple(shape) != tuple(orig_shape) else T.NoOpTransform()
        out = []
        for min_size in self.min_sizes:
            newh, neww = T.ResizeShortestEdge.get_output_shape(h, w, min_size, self.max_size)
            resize = T.ResizeTransform(h, w, newh, neww)
            out.append(T.TransformList([pre, resize]))
            if self.flip:
                out.append(T.TransformList([pre, resize, T.HFlipTransform(neww)]))
        return out

    def __call__(self, dataset_dict):
        numpy_image = dataset_dict["image"].permute(1, 2, 0).cpu().numpy()
        shape = numpy_image.shape
        orig_shape = (dataset_dict["height"], dataset_dict["width"])
        pre_tfm = T.ResizeTransform(orig_shape[0], orig_shape[1], shape[0], shape[1]) if shape[:2] != orig_shape else T.NoOpTransform()
        aug_candidates = []
        for min_size in self.min_sizes:
            resize = T.ResizeShortestEdge(min_size, self.max_size)
            aug_candidates.append([resize])
            if self.flip:
                aug_candidates.append([resize, T.RandomFlip(prob=1.0)])
        ret = []
        for aug in aug_candidates:
            aug_input = T.AugInput(np.copy(numpy_image))
            tfms = T.AugmentationList(aug)(aug_input)
            dic = copy.copy(dataset_dict)
            dic["transforms"] = T.TransformList([pre_tfm, tfms])
            dic["image"] = torch.from_numpy(np.ascontiguousarray(aug_input.image.transpose(2, 0, 1)))
            ret.append(dic)
        return ret


# ---- views on the device ----------------------------------------------------------------------------------------------------------
_OUT_ALIGN = 256
_view_plans = {}


def _view_plan(shape, geometry):
    """The tables of all views of a source of `shape`, packed for u2_aug_resize_bilinear_u8: (int32 array, descriptors, output
    bytes).  geometry: ((H, W, hflip), ...).  The source pixels follow the tables in the block (src_offset of every view)."""
    from ..data import device_mapper as dm

    key = (tuple(shape), tuple(geometry))
    plan = _view_plans.get(key)
    if plan is not None:
        return plan
    h, w = shape
    parts, bases, metas, cursor = [], [], [], 0
    for H, W, hflip in geometry:
        tables = dm.build_tables(h, w, H, W, hflip=bool(hflip))
        flat, where = dm.pack_tables(tables, [])
        rows = np.concatenate([tables["by_bounds"][:, 0], tables["by_bounds"][:, 0] + tables["by_bounds"][:, 1]])
        metas.append((tables, where, int(rows.min()), int(rows.max() - rows.min())))
        parts.append(flat)
        bases.append(cursor)
        cursor += flat.size
    flat = np.concatenate(parts).astype(np.int32, copy=False)
    descs = (dm._AugImage * len(geometry))()
    out_bytes = 0
    for a, (H, W, _), base, (tables, where, row0, nrows) in zip(descs, geometry, bases, metas):
        a.h, a.w, a.H, a.W = h, w, H, W
        a.kx, a.ky = int(tables["bx_coef"].shape[1]), int(tables["by_coef"].shape[1])
        a.x_identity, a.y_identity, a.row0, a.nrows = int(tables["x_identity"]), int(tables["y_identity"]), row0, nrows
        a.num_masks = a.first_mask = 0
        a.src_offset, a.lab_offset = 4 * flat.size, -1
        for k in dm._TABLE_ORDER + ("mask_offs",):
            setattr(a, k, base + int(where[k]))
        a.ends_base = base
        a.img_out_offset, a.lab_out_offset, a.mask_out_offset = out_bytes, 0, 0
        out_bytes += (3 * H * W + _OUT_ALIGN - 1) // _OUT_ALIGN * _OUT_ALIGN
    if len(_view_plans) >= 64:
        _view_plans.pop(next(iter(_view_plans)))
    plan = _view_plans[key] = (torch.from_numpy(flat), descs, out_bytes)
    return plan


def device_views(image, geometry):
    """The views of one CHW uint8 image, made on the device by ONE call of u2_aug_resize_bilinear_u8: V descriptors that share
    one source.  geometry: ((H, W, hflip), ...).  Returns the list of CHW uint8 views (of one allocation); each equals PIL's
    bilinear resize of the image, flipped where asked, bit for bit.  The launcher reads the tables from their host copy only:
    the pixels may already be on the device and never come back."""
    from .. import _hip

    if not image.is_cuda:
        raise RuntimeError("the device views of test-time augmentation are made by a HIP kernel: they need a GPU (no host fallback)")
    assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[0] == 3, (image.dtype, tuple(image.shape))
    dev = image.device
    h, w = int(image.shape[1]), int(image.shape[2])
    tables, descs, out_bytes = _view_plan((h, w), tuple((int(a), int(b), int(bool(c))) for a, b, c in geometry))
    tbytes, n = 4 * tables.numel(), len(geometry)
    nbytes = tbytes + 3 * h * w
    block = torch.empty((nbytes + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    block[:tbytes].view(torch.int32).copy_(_PinnedRing.get(dev).upload(tables))
    block[tbytes:nbytes].view(h, w, 3).copy_(image.permute(1, 2, 0))  # the kernel reads HWC
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    need = int(_hip.call_nostream("u2_aug_resize_bilinear_scratch_bytes", descs, n))
    if need < 0:
        raise RuntimeError("u2_aug_resize_bilinear_scratch_bytes failed with status %d" % need)
    scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _hip.call("u2_aug_resize_bilinear_u8", block, nbytes, tables.data_ptr(), out, out_bytes, scratch, need, descs, n)
    return [out[a.img_out_offset:a.img_out_offset + 3 * a.H * a.W].view(3, a.H, a.W) for a in descs]


# ---- the three kernels of csrc/tta.hip ------------------------------------------------------------------------------------------------
def tta_boxes_to_original(boxes, scores, row_view, view_desc, view_flip, view_image, image_clip, score_thresh=MERGE_SCORE_THRESH):
    """u2_tta_boxes_to_original: boxes [N, 4] fp32 of all views (row i from view row_view[i]) -> (boxes in the original image,
    clipped; candidate flags uint8 [N])."""
    from .. import _hip

    n = int(boxes.shape[0])
    out = torch.empty((n, 4), dtype=torch.float32, device=boxes.device)
    cand = torch.empty(n, dtype=torch.uint8, device=boxes.device)
    _hip.call("u2_tta_boxes_to_original", boxes, scores, row_view, view_desc, view_flip, view_image, image_clip, out, cand, n,
              int(view_flip.shape[0]), int(image_clip.shape[0]), float(score_thresh))
    return out, cand


def tta_boxes_to_views(boxes, image_rows, view_desc, view_flip, view_image, view_out_row, total_rows, max_rows):
    """u2_tta_boxes_to_views: the boxes of every image (rows image_rows[i] .. image_rows[i + 1]) in each of its views; view v
    fills rows view_out_row[v] .. of the [total_rows, 4] result."""
    from .. import _hip

    out = torch.empty((total_rows, 4), dtype=torch.float32, device=boxes.device)
    _hip.call("u2_tta_boxes_to_views", boxes, image_rows, view_desc, view_flip, view_image, view_out_row, out, int(max_rows),
              int(view_flip.shape[0]), int(image_rows.shape[0]) - 1)
    return out


def tta_reduce_masks(view_probs, view_flip, image_views, image_rows, rows_per_image, views_per_image, side):
    """u2_tta_reduce_masks: view_probs[v] fp32 [R_i, 1, P, P] of every view (image-major, view order) -> [sum R_i, 1, P, P]: the
    mean over the views of each image, flipped views mirrored, summed in view order."""
    from .. import _hip

    dev = view_flip.device
    total = sum(rows_per_image)
    out = torch.empty((total, 1, side, side), dtype=torch.float32, device=dev)
    if total == 0:
        return out
    for p in view_probs:
        assert p.dtype == torch.float32 and p.is_contiguous() and p.is_cuda
    ptrs = device_upload([p.data_ptr() for p in view_probs], torch.int64, dev)
    live = [v for r, v in zip(rows_per_image, views_per_image) if r]
    _hip.call("u2_tta_reduce_masks", ptrs, view_flip, image_views, image_rows, out, max(rows_per_image), min(live),
              len(rows_per_image), int(side))
    return out


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
class GeneralizedRCNNWithTTA(nn.Module):
    """A GeneralizedRCNN with test-time augmentation; called like GeneralizedRCNN.forward in eval mode, returns
    [{"instances": Instances}] at height x width of every input."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3, impl="device", keep_features=True):
        super().__init__()
        if isinstance(model, nn.parallel.DistributedDataParallel):
            model = model.module
        assert isinstance(model, GeneralizedRCNN), "TTA is only supported on GeneralizedRCNN. Got a model of type {}".format(type(model))
        self.cfg = cfg.clone()
        assert not self.cfg.MODEL.KEYPOINT_ON, "TTA for keypoint is not supported yet"
        assert not self.cfg.MODEL.LOAD_PROPOSALS, "TTA for pre-computed proposals is not supported yet"
        if impl not in ("device", "host"):
            raise ValueError("impl must be 'device' or 'host', got %r" % (impl,))
        self.model = model
        self.tta_mapper = DatasetMapperTTA(cfg) if tta_mapper is None else tta_mapper
        if impl == "device" and not isinstance(self.tta_mapper, DatasetMapperTTA):
            raise NotImplementedError("impl='device' builds the views of DatasetMapperTTA on the device; use impl='host' with a "
                                      "custom tta_mapper")
        self.batch_size, self.impl, self.keep_features = batch_size, impl, bool(keep_features)
        self.stage_hook = None  # optional callable(name) called at the stage boundaries of the device path (tools/bench_tta.py)

    @contextmanager
    def _turn_off_roi_heads(self, attrs):
        roi_heads = self.model.roi_heads
        old = {a: getattr(roi_heads, a) for a in attrs if hasattr(roi_heads, a)}
        for a in old:
            setattr(roi_heads, a, False)
        try:
            yield
        finally:
            for a, v in old.items():
                setattr(roi_heads, a, v)

    def _mask_side(self):
        return 2 * self.model.roi_heads.mask_pooler.output_size

    def _read(self, dataset_dict):
        ret = copy.copy(dataset_dict)
        if "image" not in ret:
            from ..data import detection_utils as utils

            image = utils.read_image(ret.pop("file_name"), self.model.input_format)
            ret["image"] = torch.from_numpy(np.ascontiguousarray(image.transpose(2, 0, 1)))
        if "height" not in ret and "width" not in ret:
            ret["height"], ret["width"] = int(ret["image"].shape[1]), int(ret["image"].shape[2])
        return ret

    def forward(self, batched_inputs):
        assert not self.model.training, "test-time augmentation runs a model in eval mode"
        inputs = [self._read(x) for x in batched_inputs]
        with torch.no_grad():
            if self.impl == "host":
                return [self._inference_one_image(x) for x in inputs]
            return self._inference_device(inputs)

    # ---- host path: test_time_augmentation.py:162-307 ---------------------------------------------------------------------------
    def _batch_inference(self, batched_inputs, detected_instances=None):
        if detected_instances is None:
            detected_instances = [None] * len(batched_inputs)
        outputs, inputs, instances = [], [], []
        for idx, (inp, inst) in enumerate(zip(batched_inputs, detected_instances)):
            inputs.append(inp)
            instances.append(inst)
            if len(inputs) == self.batch_size or idx == len(batched_inputs) - 1:
                outputs.extend(GeneralizedRCNN.inference(self.model, inputs, instances if instances[0] is not None else None,
                                                         do_postprocess=False))
                inputs, instances = [], []
        return outputs

    def _inference_one_image(self, inp):
        orig_shape = (inp["height"], inp["width"])
        augmented_inputs = self.tta_mapper(inp)
        tfms = [x.pop("transforms") for x in augmented_inputs]
        with self._turn_off_roi_heads(["mask_on", "keypoint_on"]):
            all_boxes, all_scores, all_classes = self._get_augmented_boxes(augmented_inputs, tfms)
        merged = self._merge_detections(all_boxes, all_scores, all_classes, orig_shape)
        if not self.cfg.MODEL.MASK_ON:
            return {"instances": merged}
        if len(merged) == 0:  # no box to ask the views about
            side = self._mask_side()
            merged.pred_masks = torch.zeros((0, 1, side, side), dtype=torch.float32, device=all_boxes.device)
        else:
            augmented_instances = self._rescale_detected_boxes(augmented_inputs, merged, tfms)
            outputs = self._batch_inference(augmented_inputs, augmented_instances)
            del augmented_inputs, augmented_instances
            merged.pred_masks = self._reduce_pred_masks(outputs, tfms)
        return {"instances": detector_postprocess(merged, *orig_shape)}

    def _get_augmented_boxes(self, augmented_inputs, tfms):
        outputs = self._batch_inference(augmented_inputs)
        all_boxes, all_scores, all_classes = [], [], []
        for output, tfm in zip(outputs, tfms):
            pred_boxes = output.pred_boxes.tensor
            original = apply_box_f32(tfm, pred_boxes.cpu().numpy(), inverse=True)
            all_boxes.append(torch.from_numpy(original).to(pred_boxes.device))
            all_scores.append(output.scores)
            all_classes.append(output.pred_classes)
        return torch.cat(all_boxes, dim=0), torch.cat(all_scores), torch.cat(all_classes)

    def _merge_detections(self, all_boxes, all_scores, all_classes, shape_hw):
        num_boxes, num_classes = len(all_boxes), self.cfg.MODEL.ROI_HEADS.NUM_CLASSES
        # + 1: fast_rcnn_inference expects the background scores as well; one indexed store for the reference's loop over rows
        all_scores_2d = torch.zeros(num_boxes, num_classes + 1, device=all_boxes.device)
        all_scores_2d[torch.arange(num_boxes, device=all_boxes.device), all_classes] = all_scores
        merged, _ = fast_rcnn_inference_single_image(all_boxes, all_scores_2d, shape_hw, MERGE_SCORE_THRESH,
                                                     self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, self.cfg.TEST.DETECTIONS_PER_IMAGE)
        return merged

    def _rescale_detected_boxes(self, augmented_inputs, merged, tfms):
        out = []
        for inp, tfm in zip(augmented_inputs, tfms):
            pred_boxes = torch.from_numpy(apply_box_f32(tfm, merged.pred_boxes.tensor.cpu().numpy()))
            out.append(Instances(tuple(inp["image"].shape[1:3]), pred_boxes=Boxes(pred_boxes), pred_classes=merged.pred_classes,
                                 scores=merged.scores))
        return out

    @staticmethod
    def _reduce_pred_masks(outputs, tfms):
        masks = []
        for output, tfm in zip(outputs, tfms):
            flipped = any(isinstance(t, T.HFlipTransform) for t in tfm.transforms)
            masks.append(output.pred_masks.flip(dims=[3]) if flipped else output.pred_masks)
        return mean_in_view_order(masks)

    # ---- device path --------------------------------------------------------------------------------------------------------------
    def _stage(self, name):
        if self.stage_hook is not None:
            self.stage_hook(name)

    def _inference_device(self, inputs):
        model, dev = self.model, self.model.device
        if dev.type != "cuda":
            raise RuntimeError("impl='device' runs HIP kernels: it needs a GPU (impl='host' is the definition on any device)")
        nimg = len(inputs)
        if nimg == 0:
            return []
        orig_shapes = [(x["height"], x["width"]) for x in inputs]
        # 1. views: one resize launch per image
        self._stage("views")
        view_inputs, view_tfms, views_per_image = [], [], []
        for x, orig in zip(inputs, orig_shapes):
            image = x["image"].to(dev)
            shape = (int(image.shape[1]), int(image.shape[2]))
            tfms = self.tta_mapper.view_transforms(shape, orig)
            geometry = []
            for t in tfms:
                resize = [s for s in t.transforms if isinstance(s, T.ResizeTransform)][-1]
                geometry.append((resize.new_h, resize.new_w, any(isinstance(s, T.HFlipTransform) for s in t.transforms)))
            rest = {k: v for k, v in x.items() if k != "image"}
            view_inputs.append([dict(rest, image=v) for v in device_views(image, geometry)])
            view_tfms.append(tfms)
            views_per_image.append(len(tfms))
        # 2. detection pass: the views of an image in batches of batch_size, mask head off; the FPN maps are kept
        self._stage("detect")
        kept, detections = [], []
        with self._turn_off_roi_heads(["mask_on", "keypoint_on"]):
            for views in view_inputs:
                for b0 in range(0, len(views), self.batch_size):
                    features, image_sizes, _ = GeneralizedRCNN._backbone_features(model, views[b0:b0 + self.batch_size])
                    detections.extend(model._detect_from_features(features, image_sizes))
                    kept.append((features, image_sizes) if self.keep_features else None)
        # 3. boxes back into the original images and the merge, all images at once
        self._stage("merge")
        flat_tfms = [t for tfms in view_tfms for t in tfms]
        inv = [view_descriptor(t, inverse=True) for t in flat_tfms]
        fwd = [view_descriptor(t) for t in flat_tfms]
        view_flip = device_upload([f for _, f in fwd], torch.int32, dev)
        view_image = device_upload([i for i, v in enumerate(views_per_image) for _ in range(v)], torch.int32, dev)
        inv_desc = device_upload(np.stack([d for d, _ in inv]).tolist(), torch.float32, dev)
        fwd_desc = device_upload(np.stack([d for d, _ in fwd]).tolist(), torch.float32, dev)
        clip = device_upload([[float(w), float(h)] for h, w in orig_shapes], torch.float32, dev)
        merged = self._merge_device(detections, views_per_image, inv_desc, view_flip, view_image, clip, orig_shapes)
        if not self.cfg.MODEL.MASK_ON:
            return [{"instances": m} for m in merged]
        # 4. mask pass: the merged boxes in every view, on the kept maps
        self._stage("masks")
        rows = [len(m) for m in merged]
        side = self._mask_side()
        if sum(rows):
            offs = np.concatenate([[0], np.cumsum(rows)])
            image_rows = device_upload(offs.tolist(), torch.int32, dev)
            view_out_row, cursor = [], 0
            for r, v in zip(rows, views_per_image):
                view_out_row += [cursor + k * r for k in range(v)]
                cursor += v * r
            all_boxes = torch.cat([m.pred_boxes.tensor for m in merged])
            in_views = tta_boxes_to_views(all_boxes, image_rows, fwd_desc, view_flip, view_image,
                                          device_upload(view_out_row, torch.int64, dev), cursor, max(rows))
            view_probs, v, batch = [], 0, 0
            for i, views in enumerate(view_inputs):
                for b0 in range(0, len(views), self.batch_size):
                    group = views[b0:b0 + self.batch_size]
                    if rows[i]:
                        given = []
                        for k, inp in enumerate(group):
                            o = view_out_row[v + b0 + k]
                            given.append(Instances(tuple(inp["image"].shape[1:3]), pred_boxes=Boxes(in_views[o:o + rows[i]]),
                                                   pred_classes=merged[i].pred_classes, scores=merged[i].scores))
                        if kept[batch] is not None:
                            features, image_sizes = kept[batch]
                            kept[batch] = None  # the maps of this batch are not needed again
                        else:
                            features, image_sizes, _ = GeneralizedRCNN._backbone_features(model, group)
                        out = model._detect_from_features(features, image_sizes, given)
                        view_probs.extend(o.pred_masks.contiguous() for o in out)
                    batch += 1
                v += len(views)
            del kept
            # 5. mean over the views, then rescale + paste, all images at once
            self._stage("reduce")
            if any(r == 0 for r in rows):  # the views of images without boxes made no masks: their pointers are never read
                it = iter(view_probs)
                filler = view_probs[0]
                view_probs = [next(it) if rows[i] else filler for i, n in enumerate(views_per_image) for _ in range(n)]
            image_views = device_upload(np.concatenate([[0], np.cumsum(views_per_image)]).tolist(), torch.int32, dev)
            mean = tta_reduce_masks(view_probs, view_flip, image_views, image_rows, rows, views_per_image, side)
            for m, part in zip(merged, mean.split(rows)):
                m.pred_masks = part
        else:
            self._stage("reduce")
            for m in merged:
                m.pred_masks = torch.zeros((0, 1, side, side), dtype=torch.float32, device=dev)
        out = [{"instances": r} for r in detector_postprocess_batch(merged, orig_shapes)]
        self._stage("end")
        return out

    def _merge_device(self, detections, views_per_image, inv_desc, view_flip, view_image, clip, orig_shapes):
        """fast_rcnn_inference_single_image over the union of every image's views without the dense score matrix: candidate
        flags from the kernel, a stable descending sort per image (ties keep the view-major detection order, as the reference's
        sort of the candidate list does), F.batched_nms per class, top DETECTIONS_PER_IMAGE.  One host synchronisation."""
        from ..layers import functional as F

        dev = clip.device
        nimg = len(views_per_image)
        counts_v = [len(d) for d in detections]
        n_img, v = [], 0
        for nv in views_per_image:
            n_img.append(sum(counts_v[v:v + nv]))
            v += nv
        total = sum(n_img)
        empty = lambda: torch.zeros(0, dtype=torch.float32, device=dev)  # noqa: E731
        if total == 0:
            return [Instances(s, pred_boxes=Boxes(torch.zeros((0, 4), dtype=torch.float32, device=dev)), scores=empty(),
                              pred_classes=torch.zeros(0, dtype=torch.int64, device=dev)) for s in orig_shapes]
        boxes = torch.cat([d.pred_boxes.tensor for d in detections]).float().contiguous()
        scores = torch.cat([d.scores for d in detections]).float().contiguous()
        classes = torch.cat([d.pred_classes for d in detections])
        row_view = device_upload(np.repeat(np.arange(len(counts_v)), counts_v).tolist(), torch.int32, dev)
        mapped, cand = tta_boxes_to_original(boxes, scores, row_view, inv_desc, view_flip, view_image, clip)
        nmax = max(n_img)
        row_img = np.repeat(np.arange(nimg), n_img)
        row_pos = np.concatenate([np.arange(n) for n in n_img])
        slot = device_upload((row_img * nmax + row_pos).tolist(), torch.int64, dev)
        cand = cand.bool()
        neg = torch.full((nimg * nmax,), float("-inf"), dtype=torch.float32, device=dev)
        neg[slot] = torch.where(cand, scores, float("-inf"))
        row_of = torch.zeros(nimg * nmax, dtype=torch.int64, device=dev)
        row_of[slot] = torch.arange(total, device=dev)
        order = torch.sort(neg.view(nimg, nmax), dim=1, descending=True, stable=True)[1]   # candidates first, ties in row order
        src = torch.gather(row_of.view(nimg, nmax), 1, order)                                # [B, nmax] rows of the union
        ncand = torch.zeros(nimg, dtype=torch.int32, device=dev)
        ncand.index_add_(0, device_upload(row_img.tolist(), torch.int64, dev), cand.to(torch.int32))
        live = torch.arange(nmax, device=dev)[None] < ncand[:, None]
        pb = torch.where(live[..., None], mapped[src], torch.zeros((), dtype=torch.float32, device=dev))
        pg = torch.where(live, classes[src].to(torch.int32), torch.zeros((), dtype=torch.int32, device=dev))
        topk = self.cfg.TEST.DETECTIONS_PER_IMAGE
        max_keep = nmax if topk < 0 else min(nmax, topk)
        keep, nkeep = F.batched_nms(pb, pg, ncand, self.cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, max_keep)
        nk = nkeep.tolist()  # the one host synchronisation of the merge
        kept_live = torch.arange(keep.shape[1], device=dev)[None] < nkeep[:, None]
        sel = torch.gather(src, 1, keep.long())[kept_live]  # image-major, kept order
        g_boxes, g_scores, g_classes = mapped[sel], scores[sel], classes[sel]
        out = []
        for shape, b, s, c in zip(orig_shapes, g_boxes.split(nk), g_scores.split(nk), g_classes.split(nk)):
            out.append(Instances(shape, pred_boxes=Boxes(b), scores=s, pred_classes=c))
        return out
