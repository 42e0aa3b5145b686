"""The backward reduce of a residual block's tail folded into the next block's conv1 data gradient (u2_conv_dgrad_tail, the TAIL
epilogue of conv_stream.hip; U2_TAIL_BWD_FUSE in layers/functional.py).

1. The kernel against the composition it replaces - u2_conv_igemm (forced onto the streaming kernel, same variant bits) followed
   by u2_norm_bwd_reduce with dout2, dz_out and the bit mask: dz must be bit-identical, each column sum within d u sum|term| of
   the float64 sum of the same bf16 terms, d being the longest chain of fp32 additions of the new epilogue (tail_depth, from the
   launch geometry as reduce_depth of tests/test_gpu_norm_full_size.py does for the reduce pass).
2. Through autograd: a stage of three bottleneck blocks at 2 x 13 x 21, 64 -> 256, from identical state with the switch on and
   off.  The residual-path gradients dz of the two fused tails are compared bit for bit with the two launches evaluated on the
   SAME operands - the fused run's own: conv1's incoming gradient, the posted residual gradient, the tail's saved tensors.
   Between the two RUNS only the last block's dz (a function of the stage's output gradient alone) is bit-equal: every tail's
   inputs come through the next block's dx, which depends on that block's two sums, and the order of their fp32 additions
   differs not only between the fused and the two-launch form but between any two runs (atomics; with both runs on two
   launches as well).  Measured: dz of block 0 differs between the runs in 306 of 139 776 elements, by one bf16 step; dz of
   block 1 was bit-equal in one process and not in another.  The run-to-run comparison is therefore made under the bound
   derived below, and its figures are printed.  Each fused tail's dx / dz /
   dgamma / dbeta meet the float64 closed form under check_backward's bounds in both runs (the depth being the new epilogue's
   when the switch is on).  The stage input gradient and every parameter gradient of the two runs are compared with each other
   as a guard against a dropped or doubled gradient (an error of order 1): the runs differ only in the order of the fp32
   additions behind the sums, which moves isolated elements of the bf16 gradients downstream across a rounding midpoint, one
   bf16 step (2^-8 to 2^-7 of the value) each.  A bf16 tensor may therefore differ by a step at its largest magnitude plus the
   propagated difference before the rounding, itself below a step: 2^-6 max-normalised.  An fp32 parameter gradient is a sum of
   products of such elements; if every one of them were a step off it would move by 2^-7 sum|terms|: 2^-7 max-normalised.
   The fused run makes two u2_norm_bwd_reduce calls fewer (a silent fall-back would pass every numeric check); no deferred state
   is left behind.
"""
import pytest
import torch

from tests.conv_variants import K
from tests.test_gpu_norm_full_size import DEV, EPS, MOM, NormRef, U, check_backward, gen, randn_bf, reduce_depth

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
FORCED_TINY = K.CV_STREAM_FORCE | K.CV_TINY_GRID   # conv_stream.hip: lift the size rule, 8 work-groups per channel block only
# (TM pixels per tile, waves along the pixels, waves per work-group) of the three tail instantiations, by reduction width C
TAIL_CFG = {64: (128, 1, 4), 128: (64, 1, 4), 256: (64, 2, 8)}


def tail_depth(c, n, m, tiny):
    """Longest chain of fp32 additions behind one column sum of the TAIL epilogue (launch_stream_cfg / conv_stream_kernel):
    a lane's running sum over the NF rows it holds of a tile, the 16-row transposing sum (4), one addition per tile of the
    work-group into the lane's total, the work-group flush over its waves, one atomicAdd per work-group of the channel block."""
    tm, psw, nwv = TAIL_CFG[c]
    nf = tm // psw // 16
    tiles_n = n // ((nwv // psw) * 64)
    grid = 8 * tiles_n if tiny else 256 * (2 if nwv == 4 else 1)
    nwalk = (grid // 8) // tiles_n
    per_xcd = -(-(-(-m // tm)) // 8)
    my_tiles = -(-per_xcd // nwalk)
    return nf + 4 + my_tiles + nwv + 8 * nwalk


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


MAPS = {40: (1, 5, 8), 546: (2, 13, 21), 1024: (1, 32, 32)}


def tail_case(H, c, n, m, mask_mode, seed):
    """Operands of one launch: the bits come from u2_bn_act_fused, so their layout is the product's."""
    g = gen(seed)
    y = randn_bf((m, n), g)
    sig = 0.5 + 1.5 * torch.rand(n, generator=g, device=DEV)
    off = torch.where(torch.arange(n, device=DEV) % 3 == 0, 0.0, 3.0) * sig * torch.where(torch.arange(n, device=DEV) % 2 == 0, 1.0, -1.0)
    y = (y * sig.to(BF16) + off.to(BF16)).contiguous()      # non-zero channel means
    yd = y.to(F64)
    stats = torch.stack([yd.sum(0), (yd * yd).sum(0)]).float().contiguous()
    gamma = (1 + 0.2 * torch.randn(n, generator=g, device=DEV)).contiguous()
    beta = (0.1 * torch.randn(n, generator=g, device=DEV)).contiguous()
    rm, rv = torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    mean, invstd, scale, shift = (torch.empty(n, device=DEV) for _ in range(4))
    res = randn_bf((m, n), g)
    if mask_mode == "zeros":
        res = torch.full((m, n), -1e4, dtype=BF16, device=DEV)
    elif mask_mode == "ones":
        res = torch.full((m, n), 1e4, dtype=BF16, device=DEV)
    out = torch.empty_like(y)
    bits = torch.empty((m, n // 8), dtype=torch.uint8, device=DEV)
    H.call("u2_bn_act_fused", y, stats, float(m), None, gamma, beta, rm, rv, MOM, EPS, mean, invstd, scale, shift, res, out, m, n, n,
           1, bits)
    dy = randn_bf((m, c), g)
    wt = (0.1 * torch.randn((n, c), generator=g, device=DEV)).to(BF16).contiguous()
    g2 = randn_bf((m, n), g)
    return y, bits, mean, invstd, out, dy, wt, g2


@pytest.mark.parametrize("m", [40, 546, 1024])
@pytest.mark.parametrize("c,n", [(64, 256), (128, 512), (256, 1024)])
def test_tail_kernel_against_two_launches(H, c, n, m):
    b, h, w = MAPS[m]
    d = tail_depth(c, n, m, tiny=True)
    for k, mask_mode in enumerate(("random", "zeros", "ones")):
        y, bits, mean, invstd, out, dy, wt, g2 = tail_case(H, c, n, m, mask_mode, seed=1000 * k + c + m)
        if mask_mode != "random":
            assert int(bits.max()) == int(bits.min()) == (0 if mask_mode == "zeros" else 255)
        # the two launches
        g1 = torch.empty((m, n), dtype=BF16, device=DEV)
        H.call("u2_conv_igemm", dy, wt, g1, None, None, b, h, w, c, c, h, w, n, n, 1, 1, 0, 0, 1, 1, 0, 0, FORCED_TINY)
        assert K.K_STREAM <= H.call_nostream("u2_conv_last_kernel") < K.K_STREAM + 100, "the data gradient did not run on the streaming kernel"
        dz_ref = torch.empty_like(g1)
        sums_ref = torch.zeros((2, n), device=DEV)
        H.call("u2_norm_bwd_reduce", g1, bits, y, mean, invstd, sums_ref, 1, m, n, n, 1, None, None, g2, dz_ref, None, 1)
        # the one launch
        dz = torch.full((m, n), 7.0, dtype=BF16, device=DEV)
        sums = torch.zeros((2, n), device=DEV)
        rc = H.call_status("u2_conv_dgrad_tail", dy, wt, g2, y, bits, mean, invstd, dz, sums, b, h, w, c, c, n, n, FORCED_TINY)
        assert rc == 0, "u2_conv_dgrad_tail declined a served shape"
        assert H.call_nostream("u2_conv_last_kernel") == K.K_STREAM + K.K_STREAM_TAIL + c // 32 * 10
        torch.cuda.synchronize()
        assert torch.equal(dz, dz_ref), "%s: dz differs from the two-launch path in %d elements" % (mask_mode, int((dz != dz_ref).sum()))
        if mask_mode == "zeros":
            assert int((dz.view(torch.int16) != 0).sum()) == 0
        # the float64 sums of the same bf16 terms
        dzd = dz.to(F64)
        t1 = dzd * (y.to(F64) - mean.to(F64)) * invstd.to(F64)
        for q, terms in enumerate((dzd, t1)):
            ref, bound = terms.sum(0), d * U * terms.abs().sum(0)
            for name, got in (("fused", sums[q]), ("two launches", sums_ref[q])):
                err = (got.to(F64) - ref).abs()
                dd = d if name == "fused" else reduce_depth(1, m, n)
                bnd = bound * dd / d
                i = int((err - bnd).argmax())
                print("tail %dx%d m=%d %s sum %d (%s): worst err / bound = %.3g" % (c, n, m, mask_mode, q, name,
                                                                                    float((err / (bnd + 1e-300)).max())))
                assert bool((err <= bnd).all()), "%s sum %d column %d: got %r ref %r bound %r" % (
                    name, q, i, float(got[i]), float(ref[i]), float(bnd[i]))


@pytest.mark.parametrize("c,n", [(512, 2048), (64, 252)])
def test_tail_kernel_declines_unserved_shapes(H, c, n):
    m = 64
    npad = (n + 7) // 8 * 8
    g = gen(c + n)
    dy, wt = randn_bf((m, c), g), randn_bf((n, c), g)
    g2, y = randn_bf((m, npad), g), randn_bf((m, npad), g)
    bits = torch.zeros((m, npad // 8), dtype=torch.uint8, device=DEV)
    mean, invstd = torch.zeros(npad, device=DEV), torch.ones(npad, device=DEV)
    dz = torch.full((m, npad), 7.0, dtype=BF16, device=DEV)
    sums = torch.zeros((2, npad), device=DEV)
    rc = H.call_status("u2_conv_dgrad_tail", dy, wt, g2, y, bits, mean, invstd, dz, sums, 1, 8, 8, c, c, n, n, FORCED_TINY)
    torch.cuda.synchronize()
    assert rc == 1, "an unserved shape must answer 'not served'"
    assert bool((dz == 7.0).all()) and not bool(sums.any()), "a declined launch wrote to its outputs"


# -------------------------------------------------------------------------------------------------
def run_stage(F, H, monkeypatch, fuse, state):
    """One forward / backward pass of a three-block stage from `state` (parameters, input, output gradient); returns the
    captured tensors.  batch_norm_act is wrapped to reach the tails' tensors, _hip.call to count the reduce launches."""
    from u2seg_amd.modeling.backbone import BottleneckBlock, ResNet

    F.set_tail_bwd_fuse(fuse)
    torch.manual_seed(0)
    blocks = ResNet.make_stage(BottleneckBlock, 3, in_channels=64, out_channels=256, stride_per_block=[1, 1, 1],
                               bottleneck_channels=64, norm="BN")
    stage = torch.nn.Sequential(*blocks).to(DEV).train()
    if "params" in state:
        stage.load_state_dict(state["params"])
    else:
        with torch.no_grad():
            for name, p in stage.named_parameters():
                if name.endswith("norm.weight"):
                    p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen(len(name)), device=DEV))
                elif name.endswith("norm.bias"):
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen(len(name) + 1), device=DEV))
        state["params"] = {k: v.clone() for k, v in stage.state_dict().items()}
        state["x"] = randn_bf((2, 13, 21, 64), gen(5))
        state["dout"] = randn_bf((2, 13, 21, 256), gen(6))
    tails, calls, norms = [], [], []
    real_bn, real_call = F.batch_norm_act, H.call

    def bn(y, stats, gamma, beta, rm, rv, residual=None, relu=False, *a, **k):
        out = real_bn(y, stats, gamma, beta, rm, rv, residual, relu, *a, **k)
        rec = {"y": y, "out": out, "gamma": gamma, "beta": beta, "res": residual}
        norms.append(rec)   # in call order: block 0 conv1, conv2, shortcut, conv3; blocks 1, 2 conv1, conv2, conv3
        y.register_hook(lambda g, rec=rec: rec.__setitem__("dx", g.clone()))
        if residual is not None:
            saved = out.grad_fn.saved_tensors   # (y, bits, gamma, mean, invstd, ...)
            rec["bits"], rec["mean"], rec["invstd"] = saved[1], saved[3], saved[4]
            tails.append(rec)
            residual.register_hook(lambda g, rec=rec: rec.__setitem__("dz", g.clone()))   # this tail's dz, as it leaves
            out.register_hook(lambda g, rec=rec: rec.__setitem__("g1", g))
        return out

    def call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(F, "batch_norm_act", bn)
    monkeypatch.setattr(H, "call", call)
    x = state["x"].clone().requires_grad_(True)
    out = stage(x)
    F.reset_deferred_gradients()
    out.backward(state["dout"])   # (the stage output's second handle receives nothing)
    torch.cuda.synchronize()
    F.assert_no_deferred_gradients()
    monkeypatch.setattr(F, "batch_norm_act", real_bn)
    monkeypatch.setattr(H, "call", real_call)
    grads = {k: p.grad.clone() for k, p in stage.named_parameters()}
    return {"tails": tails, "norms": norms, "calls": calls, "dx": x.grad.clone(), "grads": grads, "stage": stage}


def two_launches(F, H, run, k):
    """(g1, dz) of the tail of block k by u2_conv_igemm + u2_norm_bwd_reduce on the operands that run met: the gradient arriving at
    the conv1 output of block k + 1, that layer's data-gradient filter, the next tail's dz, the tail's saved tensors."""
    t = run["tails"][k]
    dy = run["norms"][4 + 3 * k]["dx"].contiguous()      # conv1 of block k + 1
    conv1 = run["stage"][k + 1].conv1
    b, h, w, c = dy.shape
    n = t["y"].shape[3]
    wd = F.weight_dgrad_layout(conv1.weight, n, c, conv1.weight)
    g1, dz = torch.empty_like(t["y"]), torch.empty_like(t["y"])
    H.call("u2_conv_igemm", dy, wd, g1, None, None, b, h, w, c, c, h, w, n, n, 1, 1, 0, 0, 1, 1, 0, 0, FORCED_TINY)
    sums = torch.zeros((2, n), device=DEV)
    H.call("u2_norm_bwd_reduce", g1, t["bits"], t["y"], t["mean"], t["invstd"], sums, 1, b * h * w, n, n, 1, None, None,
           run["tails"][k + 1]["dz"].contiguous(), dz, None, 1)
    return g1, dz


def max_rel(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def test_stage_backward_fused_against_two_launches(H, monkeypatch):
    from u2seg_amd.layers import functional as F

    monkeypatch.setenv("U2_CONV_VARIANT", str(FORCED_TINY))   # every served 1x1 launch on the streaming kernel, both runs
    was = F.TAIL_BWD_FUSE
    state = {}
    try:
        off = run_stage(F, H, monkeypatch, False, state)
        on = run_stage(F, H, monkeypatch, True, state)
    finally:
        F.set_tail_bwd_fuse(was)
    n_off, n_on = off["calls"].count("u2_norm_bwd_reduce"), on["calls"].count("u2_norm_bwd_reduce")
    print("u2_norm_bwd_reduce calls: %d with two launches, %d fused" % (n_off, n_on))
    assert n_on == n_off - 2, "the fused path was not taken for both tails (a silent fall-back)"
    assert len(off["tails"]) == len(on["tails"]) == 3
    m, c = 2 * 13 * 21, 256
    d_new = tail_depth(64, 256, m, tiny=True)
    # the residual-path gradients of the fused tails (blocks 0 and 1), captured as they leave the tails: against the two launches
    # on the same operands bit for bit (below), between the runs under the bf16 bound of the module's docstring
    assert torch.equal(on["tails"][2]["dz"], off["tails"][2]["dz"])
    for k in (0, 1):
        a, b = on["tails"][k]["dz"], off["tails"][k]["dz"]
        print("dz of block %d, fused run against two-launch run: %d of %d elements differ, max-normalised %.3g" % (
            k, int((a != b).sum()), a.numel(), max_rel(a, b)))
        assert max_rel(a, b) <= 2.0 ** -6
    g1s = {}
    for run, name in ((off, "two launches"), (on, "fused")):
        for k in (0, 1):
            g1s[(name, k)], dz2 = two_launches(F, H, run, k)
            assert torch.equal(run["tails"][k]["dz"], dz2), "%s: dz of the tail of block %d is not the two launches' on the same operands" % (name, k)
    for run, name in ((off, "two launches"), (on, "fused")):
        for k in (0, 1):
            t, t_off = run["tails"][k], off["tails"][k]
            assert torch.equal(t["y"], t_off["y"]) and torch.equal(t["out"], t_off["out"])
            # the statistics behind mean / invstd come from the conv3 epilogue (conv_stream forward, the same chain as the tail's)
            ref = NormRef(t["y"].detach().view(1, m, c), t["gamma"], t["beta"], 1, d_new * U)
            # g1 as u2_conv_igemm forms it from this run's operands (the fused run never stores it); g2 is the next tail's dz
            if run is off:
                assert torch.equal(g1s[(name, k)], t["g1"])
            douts = [g1s[(name, k)].view(1, m, c), run["tails"][k + 1]["dz"].view(1, m, c)]
            gamma, beta = torch.nn.Parameter(t["gamma"].detach()), torch.nn.Parameter(t["beta"].detach())
            gamma.grad, beta.grad = run["grads"]["%d.conv3.norm.weight" % k], run["grads"]["%d.conv3.norm.bias" % k]
            depth = d_new if run is on else reduce_depth(1, m, c)
            check_backward(ref, "block %d tail (%s)" % (k, name), douts, t["out"].detach().view(1, m, c), True,
                           t["dx"].view(1, m, c), gamma, beta, depth, t["dz"].view(1, m, c))
    r = max_rel(on["dx"], off["dx"])
    print("stage input gradient, fused against two launches: %.3g" % r)
    assert r <= 2.0 ** -6
    worst = max((max_rel(g, off["grads"][k]), k) for k, g in on["grads"].items())
    print("parameter gradients, fused against two launches: worst %.3g (%s)" % worst)
    assert worst[0] <= 2.0 ** -7, worst


def test_misrouted_placeholder_raises(H, monkeypatch):
    """A tail gradient formed by conv1 whose placeholder meets a further consumer of the block output must fail loudly."""
    from u2seg_amd.layers import functional as F
    from u2seg_amd.modeling.backbone import BottleneckBlock, ResNet

    monkeypatch.setenv("U2_CONV_VARIANT", str(FORCED_TINY))
    was = F.TAIL_BWD_FUSE
    F.set_tail_bwd_fuse(True)
    try:
        torch.manual_seed(0)
        blocks = ResNet.make_stage(BottleneckBlock, 2, in_channels=64, out_channels=256, stride_per_block=[1, 1],
                                   bottleneck_channels=64, norm="BN")
        b0, b1 = (b.to(DEV).train() for b in blocks)
        x = randn_bf((2, 13, 21, 64), gen(7)).requires_grad_(True)
        mid = b0(x)
        out = b1(mid)
        extra = mid.float().sum()   # a third consumer on the first handle: autograd sums its gradient with the placeholder
        F.reset_deferred_gradients()
        with pytest.raises(RuntimeError, match="U2_TAIL_BWD_FUSE"):
            torch.autograd.backward([out, extra], [randn_bf(out.shape, gen(8)), torch.ones((), device=DEV)])
        F.reset_deferred_gradients(strict=False)
    finally:
        F.set_tail_bwd_fuse(was)
