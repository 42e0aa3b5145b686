"""The layout of u2seg_amd/layers: layers.functional stays the one name the package calls the layers by, the stream state lives in
layers.streams alone, and the parts of streams.py that need no GPU - the stream-K rule, the inline weight gradient, the
branch-piece queue - behave as their callers assume."""
import pytest
import torch

from u2seg_amd import _hip
from u2seg_amd.layers import functional as F
from u2seg_amd.layers import losses, select, streams, weights

MOVED = {
    streams: ["set_stream_overlap", "aux_stream", "join_aux_stream", "streamk_region", "queue_branch_pieces", "issue_branch_piece",
              "flush_branch_pieces", "clear_branch_pieces", "join_all_streams", "producer_streams", "join_wgrad_stream"],
    weights: ["BF16", "ceil32", "zeros_f32", "release_library_scratch", "weight_fwd_layout", "weight_dgrad_layout",
              "weight_fc_dgrad_layout", "grad_slot", "_weight_layout"],
    losses: ["sem_seg_loss", "softmax_cross_entropy", "box_reg_l1_loss", "sigmoid_cross_entropy", "BOX_REG_LOSS_KINDS",
             "box_reg_loss", "mask_predict_bce_loss", "count_labels_i8", "mask_predict_prob", "rpn_losses"],
    select: ["assign_levels", "mask_crop", "iou_match", "sem_seg_upsample", "topk_rows", "topk_rows_multi", "apply_deltas",
             "rpn_decode", "batched_nms", "_topk_rows_sorted", "_TOPK_MAX_K"],
}
KEPT = ["set_deterministic_stats", "conv2d", "conv2d_add_", "linear", "stem_conv", "batch_norm_act", "affine_act",
        "group_norm_act", "max_pool_3x3_s2", "STEM_TAIL_FUSE", "stem_tail_ok", "batch_norm_relu_max_pool", "affine_relu_max_pool",
        "fpn_upsample_add", "bilinear_up2", "fan_out", "RoiGradTap", "roi_grad_tap", "FUSED_BWD_MIN_PIXELS", "LAZY_BN_APPLY",
        "ROI_SUM_FOLD", "TAIL_BWD_FUSE", "set_tail_bwd_fuse", "reset_deferred_gradients", "assert_no_deferred_gradients",
        "ROI_ORDER_MIN", "ROI_ALIGN_BWD_ATOMIC", "roi_align", "_roi_group", "_roi_gather", "_Conv2dFn", "_StemConvFn",
        "_fixed_order_stats", "_DET_STATS"]
STREAM_STATE = ["_WGRAD_SIDE", "_AUX_ENABLED", "_SK_REGION", "_side_streams", "_aux_streams", "_deferred_pieces", "_branch_pieces"]


def test_functional_keeps_its_surface_and_owns_no_stream_state():
    for module, names in MOVED.items():
        for name in names:
            assert hasattr(F, name), name
            assert getattr(F, name) is getattr(module, name), name
    for name in KEPT:
        assert hasattr(F, name), name
        assert not any(hasattr(module, name) for module in MOVED), name   # defined here, and only here
    for name in STREAM_STATE:
        assert not hasattr(F, name), name
    for name in STREAM_STATE[:5] + ["_branch_pieces"]:
        assert hasattr(streams, name), name


@pytest.fixture
def clean_rule(monkeypatch):
    for name in ("U2_AUX_STREAM", "U2_STREAMK_EVERYWHERE", "U2_CONV_VARIANT"):
        monkeypatch.delenv(name, raising=False)
    assert streams._SK_REGION[0] == 0
    try:
        streams.set_stream_overlap(True)
        yield monkeypatch
    finally:
        streams.set_stream_overlap(True)
        assert streams._SK_REGION[0] == 0


def test_streamk_rule_table(clean_rule):
    forbid, rule = _hip.K.CV_STREAMK_FORBID, streams._conv_variant
    assert forbid and streams._NO_STREAMK == forbid
    assert rule() == forbid
    with streams.streamk_region():
        assert rule() == 0
        with streams.streamk_region():
            assert rule() == 0
        assert rule() == 0   # the inner exit leaves the outer region open
    assert rule() == forbid
    with pytest.raises(KeyError):
        with streams.streamk_region():
            with streams.streamk_region():
                raise KeyError("inside")
    assert rule() == forbid and streams._SK_REGION[0] == 0

    streams.set_stream_overlap(False)
    assert rule() == 0
    streams.set_stream_overlap(True)
    assert rule() == forbid

    for name, value in (("U2_AUX_STREAM", "0"), ("U2_STREAMK_EVERYWHERE", "1"), ("U2_CONV_VARIANT", "0"),
                        ("U2_CONV_VARIANT", "4097"), ("U2_CONV_VARIANT", "")):
        clean_rule.setenv(name, value)
        assert rule() == 0, (name, value)
        clean_rule.delenv(name)
        assert rule() == forbid, name
    clean_rule.setenv("U2_AUX_STREAM", "1")
    clean_rule.setenv("U2_STREAMK_EVERYWHERE", "0")
    assert rule() == forbid

    # torch.distributed reporting two ranks
    clean_rule.setattr(streams, "_world", lambda: 2)
    assert rule() == forbid
    with streams.streamk_region():
        assert rule() == forbid   # the gradient exchange's stream competes inside the backbone as well
    streams.set_stream_overlap(False)
    assert rule() == forbid
    streams.set_stream_overlap(True)
    clean_rule.setenv("U2_AUX_STREAM", "0")
    assert rule() == forbid
    clean_rule.delenv("U2_AUX_STREAM")
    # the two switches that hand the dispatch to the caller are read first and still win
    clean_rule.setenv("U2_STREAMK_EVERYWHERE", "1")
    assert rule() == 0
    clean_rule.delenv("U2_STREAMK_EVERYWHERE")
    clean_rule.setenv("U2_CONV_VARIANT", "0")
    assert rule() == 0
    clean_rule.delenv("U2_CONV_VARIANT")
    assert rule() == forbid
    clean_rule.setattr(streams, "_world", lambda: 1)
    assert rule() == forbid
    with streams.streamk_region():
        assert rule() == 0


def test_weight_gradient_runs_inline_without_the_side_stream(monkeypatch):
    def no_cuda(*a, **k):
        raise AssertionError("the inline path must not touch the CUDA API")

    monkeypatch.setattr(streams, "_WGRAD_SIDE", False)
    for name in ("current_stream", "stream", "Stream"):
        monkeypatch.setattr(torch.cuda, name, no_cuda)
    monkeypatch.setattr(streams, "_side_stream", no_cuda)
    calls, before = [], (dict(streams._side_dirty), dict(streams._side_streams))
    streams._run_wgrad(torch.device("cpu"), (), lambda: calls.append(1))
    assert calls == [1]
    assert (streams._side_dirty, streams._side_streams) == before


def test_branch_piece_queue():
    log = []
    piece = lambda k: (lambda: log.append(k))
    try:
        streams.issue_branch_piece()   # nothing queued: a no-op
        streams.flush_branch_pieces()
        assert log == []
        streams.queue_branch_pieces([piece(0), piece(1), piece(2)])
        streams.queue_branch_pieces([piece(3), piece(4)])
        streams.issue_branch_piece()
        assert log == [0]
        streams.issue_branch_piece(2)
        assert log == [0, 1, 2] and len(streams._branch_pieces) == 2
        streams.issue_branch_piece(5)   # more than are queued: stops at the empty queue
        assert log == [0, 1, 2, 3, 4] and not streams._branch_pieces
        streams.queue_branch_pieces([piece(5), piece(6)])
        streams.flush_branch_pieces()
        assert log == [0, 1, 2, 3, 4, 5, 6] and not streams._branch_pieces
        streams.queue_branch_pieces([piece(7), piece(8)])
        streams.clear_branch_pieces()   # dropped, not called
        assert not streams._branch_pieces
        streams.flush_branch_pieces()
        assert log == [0, 1, 2, 3, 4, 5, 6]
        assert F.queue_branch_pieces is streams.queue_branch_pieces and F.clear_branch_pieces is streams.clear_branch_pieces
    finally:
        streams.clear_branch_pieces()
