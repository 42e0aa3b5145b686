"""Semantic / panoptic test-time augmentation on the host: the float64 definition of the mean of the
views' logits against a literal torch restatement, and the --tta-outputs flag.  CPU only."""
import numpy as np
import pytest
import torch

from tests import tta_panoptic_cases as P
from u2seg_amd.engine import default_argument_parser
from u2seg_amd.modeling.test_time_augmentation import mean_in_view_order


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_float64_definition_agrees_with_the_torch_restatement(name):
    """mean_logits_f64 against F.interpolate(bilinear, align_corners=False) of every view's window, Tensor.flip where the view
    was flipped, mean_in_view_order - all float32 on the CPU - within (V + 8) * 2^-24 * max |logit|."""
    c, H, W, views = P.CASES[name]
    blocks, windows, flips = P.make_views(name, seed=11)
    terms = []
    for block, (h, w), flipped in zip(blocks, windows, flips):
        window = torch.from_numpy(block)[:, :h, :w]
        term = torch.nn.functional.interpolate(window[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        terms.append(term.flip(dims=[2]) if flipped else term)
    got = mean_in_view_order(terms)
    assert got.dtype == torch.float32 and tuple(got.shape) == (c, H, W)
    want = P.mean_logits_f64(blocks, windows, flips, H, W)
    assert want.dtype == np.float64 and want.shape == (c, H, W) and np.isfinite(want).all()
    magnitude = max(float(np.abs(b[:, :h, :w]).max()) for b, (h, w) in zip(blocks, windows))
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print("%s: max error %.3e, bound %.3e" % (name, err, P.bound(len(views), magnitude)))
    assert err <= P.bound(len(views), magnitude)


def test_definition_of_a_flipped_identity_view_and_the_view_order():
    """By hand: an identity view and its mirrored twin average to the symmetrised map; one view is its own mean."""
    v = np.arange(12, dtype=np.float32).reshape(1, 3, 4)
    assert np.array_equal(P.mean_logits_f64([v], [(3, 4)], [False], 3, 4), v.astype(np.float64))
    both = P.mean_logits_f64([v, v], [(3, 4)] * 2, [False, True], 3, 4)
    assert np.array_equal(both, (v.astype(np.float64) + v[:, :, ::-1]) / 2.0)
    # a 1 x 1 source is constant over the output; the padding of a block is never read
    block = np.full((2, 4, 6), np.nan, dtype=np.float32)
    block[:, 0, 0] = [3.0, -5.0]
    out = P.mean_logits_f64([block], [(1, 1)], [True], 5, 7)
    assert np.array_equal(out, np.broadcast_to(np.array([3.0, -5.0])[:, None, None], (2, 5, 7)))


def test_parser_takes_tta_outputs():
    p = default_argument_parser()
    assert p.parse_args([]).tta_outputs == "instances"
    assert p.parse_args(["--tta-outputs", "instances"]).tta_outputs == "instances"
    assert p.parse_args(["--tta-outputs", "panoptic"]).tta_outputs == "panoptic"
    with pytest.raises(SystemExit):
        p.parse_args(["--tta-outputs", "semantic"])
