"""Test-time augmentation of the semantic and panoptic outputs of a PanopticFPN.

`GeneralizedRCNNWithTTA` (modeling/test_time_augmentation.py) returns instances only, as the reference's
wrapper does.  `PanopticFPNWithTTA` adds what that wrapper does not return: the mean over the views of the semantic logits and
the panoptic merge of its arg-max with the augmented instances.  Keypoints are not augmented.

The module test_time_augmentation.py is left as it is: the subclass reaches the FPN maps of the detection pass by standing in
front of `model._detect_from_features` for the length of a call (`_watch_view_features`), the way the parent switches the mask
head off for the detection pass."""
import ctypes
from contextlib import contextmanager

import torch

from ..data import transforms as T
from .batched import device_upload
from .inference import combine_semantic_and_instance_outputs_batch, sem_seg_postprocess
from .panoptic_fpn import GeneralizedRCNN, PanopticFPN
from .test_time_augmentation import GeneralizedRCNNWithTTA, mean_in_view_order

__all__ = ["PanopticFPNWithTTA", "tta_accumulate_sem_seg"]


def tta_accumulate_sem_seg(view_logits, windows, flips, acc, first, divisor=0, argmax=None):
    """u2_tta_accumulate_sem_seg (csrc/tta.hip): adds the terms of some views of one image, in list order, to the running sum
    `acc` (fp32 [C, H, W], contiguous).  view_logits[k]: fp32 [C, >= h, >= w] device tensor of any channel and row stride (a
    slice of the head's padded batch), read in its window windows[k] = (h, w); flips[k]: mirror the term along x.  first: the
    sum starts here (acc is not read); divisor > 0: this is the last call, the sum is divided by float(divisor) and `argmax`
    (optional int64 [H, W]) is written."""
    from .. import _hip

    n = len(view_logits)
    c, h, w = (int(d) for d in acc.shape)
    assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.is_cuda, (acc.dtype, acc.is_contiguous(), acc.device)
    flat = []
    for t, (vh, vw), f in zip(view_logits, windows, flips):
        assert t.dtype == torch.float32 and t.is_cuda and t.dim() == 3 and t.shape[0] == c and t.stride(2) == 1, (t.dtype, t.shape)
        assert vh <= t.shape[1] and vw <= t.shape[2], ((vh, vw), tuple(t.shape))
        flat += [int(vh), int(vw), t.stride(1), t.stride(0), int(bool(f))]
    if argmax is not None:
        assert argmax.dtype == torch.int64 and argmax.is_contiguous() and tuple(argmax.shape) == (h, w)
    ptrs = device_upload([t.data_ptr() for t in view_logits], torch.int64, acc.device) if n else None
    _hip.call("u2_tta_accumulate_sem_seg", ptrs, (ctypes.c_longlong * max(len(flat), 1))(*flat), n, acc, int(bool(first)),
              int(divisor), argmax, c, h, w)


def _flipped(tfm):
    return any(isinstance(t, T.HFlipTransform) for t in tfm.transforms)


class PanopticFPNWithTTA(GeneralizedRCNNWithTTA):
    """A PanopticFPN with test-time augmentation; called like PanopticFPN.forward in eval mode, returns
    [{"instances", "sem_seg", "panoptic_seg"}] at height x width of every input.

    instances     what GeneralizedRCNNWithTTA with the same arguments returns.
    sem_seg       float32 [C, H, W]: the mean over the views of the views' LOGITS.  View v contributes
                  sem_seg_postprocess(logits_v, view_size_v, H, W), mirrored along x when the view was flipped; the views are
                  summed by mean_in_view_order.  The logits of a view come from model.sem_seg_head on the FPN maps of the view
                  batches of the detection pass (views of one image, batch_size at a time: the padded batch shape is part of
                  what the head sees, so both implementations group alike).
                  Logits, not probabilities, are averaged: the result stays in the units of the plain model's "sem_seg", of
                  which every consumer takes the arg-max, and every step is float32 arithmetic that a kernel repeats bit for
                  bit - a softmax is not.
    panoptic_seg  combine_semantic_and_instance_outputs_batch on the augmented instances and the arg-max of the mean logits
                  (first maximum), with the model's own combine_* thresholds.

    impl="host" writes this out from existing pieces, one image at a time; impl="device" runs the head on the maps the
    detection pass computes anyway and reduces the views with u2_tta_accumulate_sem_seg, one call per view batch, so that only
    batch_size views' logits are alive at a time; all on the current stream."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=3, impl="device", keep_features=True):
        super().__init__(cfg, model, tta_mapper, batch_size, impl, keep_features)
        assert isinstance(self.model, PanopticFPN), "PanopticFPNWithTTA wraps a PanopticFPN. Got a model of type {}".format(
            type(self.model))
        assert self.cfg.MODEL.MASK_ON, "the panoptic merge takes the instances' masks: MODEL.MASK_ON must be True"
        if impl == "device" and self.model.sem_seg_head.num_classes > 64:
            raise NotImplementedError("impl='device' keeps a pixel's class sums in registers: at most 64 classes (got %d); use "
                                      "impl='host'" % self.model.sem_seg_head.num_classes)

    def _combine(self, instances, argmaxes):
        model = self.model
        mask_res = 2 * model.roi_heads.mask_pooler.output_size if getattr(model.roi_heads, "mask_on", False) else 0
        return combine_semantic_and_instance_outputs_batch(instances, argmaxes, model.combine_overlap_thresh,
                                                           model.combine_stuff_area_thresh, model.combine_instances_score_thresh,
                                                           mask_res)

    # ---- host path ------------------------------------------------------------------------------------------------------------------
    def _inference_one_image(self, inp):
        out = super()._inference_one_image(inp)
        out["sem_seg"] = self._mean_logits_host(inp)
        out["panoptic_seg"] = self._combine([out["instances"]], [out["sem_seg"].argmax(dim=0)])[0]
        return out

    def _mean_logits_host(self, inp):
        height, width = inp["height"], inp["width"]
        views = self.tta_mapper(inp)
        tfms = [v.pop("transforms") for v in views]
        terms = []
        for b0 in range(0, len(views), self.batch_size):
            features, image_sizes, _ = GeneralizedRCNN._backbone_features(self.model, views[b0:b0 + self.batch_size])
            logits, _ = self.model.sem_seg_head(features, None)
            for k, size in enumerate(image_sizes):
                term = sem_seg_postprocess(logits[k], size, height, width)
                terms.append(term.flip(dims=[2]) if _flipped(tfms[b0 + k]) else term)
        return mean_in_view_order(terms)

    # ---- device path ----------------------------------------------------------------------------------------------------------------
    def _view_batches(self, inputs):
        """The view batches of the parent's detection pass in its order: (image, first view, the image's TransformLists, the
        image's output size) per call of _backbone_features."""
        out = []
        for i, x in enumerate(inputs):
            orig = (x["height"], x["width"])
            tfms = self.tta_mapper.view_transforms((int(x["image"].shape[1]), int(x["image"].shape[2])), orig)
            out += [(i, b0, tfms, orig) for b0 in range(0, len(tfms), self.batch_size)]
        return out

    def _accumulate_batch(self, sem, batch, features, image_sizes):
        """The semantic head on the maps of one view batch, and its views added to the image's running sum."""
        image, first_view, tfms, orig_shape = batch
        logits, _ = self.model.sem_seg_head(features, None)  # [B, C, padded H, padded W] on the current stream
        n = len(image_sizes)
        assert first_view + n <= len(tfms), "the detection pass does not batch the views as planned"
        if image not in sem:
            sem[image] = (torch.empty((logits.shape[1],) + tuple(orig_shape), dtype=torch.float32, device=logits.device),
                          torch.empty(tuple(orig_shape), dtype=torch.int64, device=logits.device))
        acc, argmax = sem[image]
        last = first_view + n == len(tfms)
        tta_accumulate_sem_seg([logits[k] for k in range(n)], image_sizes, [_flipped(t) for t in tfms[first_view:first_view + n]],
                               acc, first_view == 0, len(tfms) if last else 0, argmax if last else None)
        # the logits go back to the allocator here; the kernel that reads them is ahead of any reuse on this stream

    @contextmanager
    def _watch_view_features(self, batches, sem):
        """For the length of a call, every detection-pass call of model._detect_from_features (no given instances) first hands
        its FPN maps to the semantic head; the calls of the mask pass go through as they are."""
        model = self.model
        plain = model._detect_from_features
        todo = iter(batches)

        def detect(features, image_sizes, detected_instances=None):
            if detected_instances is None:
                self._accumulate_batch(sem, next(todo), features, image_sizes)
            return plain(features, image_sizes, detected_instances)

        model._detect_from_features = detect
        try:
            yield
        finally:
            del model._detect_from_features  # the class's method again

    def _inference_device(self, inputs):
        sem = {}
        with self._watch_view_features(self._view_batches(inputs), sem):
            out = super()._inference_device(inputs)
        if out:
            assert len(sem) == len(out), "not every image went through the semantic head"
            self._stage("panoptic")
            merged = self._combine([o["instances"] for o in out], [sem[i][1] for i in range(len(out))])
            for i, (o, panoptic) in enumerate(zip(out, merged)):
                o["sem_seg"], o["panoptic_seg"] = sem[i][0], panoptic
            self._stage("end")
        return out
