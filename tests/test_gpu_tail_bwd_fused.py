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
3. Past the LDS ring's end.  The shapes of 1 and 2 leave a work-group at most two tiles against a ring of five stages, so the
   kernel never refills a ring slot there.  TAIL_CASES adds, per shape: 59 tiles on the 8-work-group grid (8 or 7 per walker),
   3 331 / 1 667 / 419 tiles on the production grid (64 / 32 / 8 walkers per XCD and channel block, 7 or 6 tiles each, taken
   nwalk apart), 546 pixels on the production grid (most walkers idle) and 5 595 pixels (two tiles 8 apart); each with random
   inputs as in 1 and with exact inputs - small integers, so that dz must equal its float64 definition bit for bit and sum dz
   the integer - and a dy that is a column window of a wider buffer.  Every case asserts its regime from the launch geometry
   restated in tests/float64_refs.py (stream_geometry; checked on hand-worked values by tests/test_float64_refs_host.py) and
   the kernel code.  Through autograd at production dispatch: two blocks 1024 -> 1024 at 8 x 50 x 84, no variant word.
   Measured on the MI355X, worst err / bound of the column sums: 0.068 (8-work-group grid), 0.011 (production grid), 0 with exact
   inputs, 1.9e-3 in the stage; 0.04 s for the three mask modes of the 426 331-pixel case.
"""
import time

import pytest
import torch

from tests.conv_variants import K
from tests.float64_refs import TWO24, bf16_round, exact_amp, stream_geometry, tail_depth, walker_tiles
from tests.test_gpu_norm_full_size import CHUNK, DEV, EPS, MOM, NormRef, U, check_backward, gen, randn_bf, reduce_depth

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F64 = torch.float64
FORCED = K.CV_STREAM_FORCE                         # conv_stream.hip: lift the size rule, the production grid
FORCED_TINY = K.CV_STREAM_FORCE | K.CV_TINY_GRID   # ... and 8 work-groups per channel block only


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip

    _hip.load()
    return _hip


MAPS = {40: (1, 5, 8), 546: (2, 13, 21), 1024: (1, 32, 32)}
SHAPES = [(64, 256), (128, 512), (256, 1024)]
# Pixel counts past the ring's end (5 stages in all three instantiations), TP = 8 xcnt + 3 tiles less 37 pixels: XCDs 0-2 own one
# tile more than XCDs 3-7, the last tile is ragged.  8-work-group grid: 59 tiles, a walker owns 8 or 7.  Production grid
# (nwalk = 64 / 32 / 8 walkers per XCD and channel block): 3 331 / 1 667 / 419 tiles, a walker owns 7 or 6.
STEADY_TINY = {64: 59 * 128 - 37, 128: 59 * 64 - 37, 256: 59 * 64 - 37}
STEADY_PROD = {64: 3331 * 128 - 37, 128: 1667 * 64 - 37, 256: 419 * 64 - 37}
# (C, N, pixels, tiny grid, input mode, columns of the dy buffer beyond C, regime)
#   prologue: no walker owns as many tiles as the ring has stages (the cases this file began with, ids unchanged)
#   steady:   every walker owns ring + 1 tiles or more, some ring + 2: ring slots are refilled while companion loads are in
#             flight, tail_epilogue runs with step_issued, the counted waits are the deep ones, the slot index wraps
#   idle:     production grid on a small map: most walkers own nothing and return at once
#   strided:  production grid, walkers 0-2 of every XCD own two tiles nwalk apart, the others one
TAIL_CASES = [(c, n, m, True, "random", 0, "prologue") for m in (40, 546, 1024) for c, n in SHAPES]
for _mode in ("exact", "random"):
    for _c, _n in SHAPES:
        TAIL_CASES += [(_c, _n, STEADY_TINY[_c], True, _mode, 0, "steady"), (_c, _n, STEADY_PROD[_c], False, _mode, 0, "steady"),
                       (_c, _n, 546, False, _mode, 0, "idle")]
    TAIL_CASES.append((256, 1024, 88 * 64 - 37, False, _mode, 0, "strided"))
TAIL_CASES += [(c, n, STEADY_TINY[c], True, "exact", 8, "steady") for c, n in SHAPES]


def tail_case_id(case):
    c, n, m, tiny, mode, pad, regime = case
    if regime == "prologue":
        return "%d-%d-%d" % (c, n, m)
    return "%d-%d-%d-%s-%s%s" % (c, n, m, "tiny" if tiny else "prod", mode, "-ld%d" % (c + pad) if pad else "")


def assert_regime(geo, m, regime):
    """The launch geometry (float64_refs.stream_geometry, itself checked on the host) puts the case where it claims to be."""
    counts, ring = walker_tiles(geo), geo["ring"]
    if regime == "steady":
        assert counts[-1] >= ring + 2 and counts[0] >= ring + 1, (counts, ring)
        assert len(set(geo["xcnt"])) == 2 and m % geo["TM"] != 0
    elif regime == "idle":
        assert counts == [1] and sum(t == 0 for row in geo["my_tiles"] for t in row) > 4 * geo["nwalk"]
    elif regime == "strided":
        assert counts == [1, 2] and geo["nwalk"] == 8
    else:
        assert counts[-1] < ring


def row_chunks(m, n):
    rc = max(1, CHUNK // n)
    return [slice(r0, min(m, r0 + rc)) for r0 in range(0, m, rc)]


def relu_bits(H, m, n, mask_mode, g):
    """A conv3 output y with non-zero channel means, its batch statistics and the ReLU bits of relu(bn(y) + res): the bits come
    from u2_bn_act_fused, so their layout is the product's."""
    y = randn_bf((m, n), g)
    sig = 0.5 + 1.5 * torch.rand(n, generator=g, device=DEV)
    off = torch.where(torch.arange(n, device=DEV) % 3 == 0, 0.0, 3.0) * sig * torch.where(torch.arange(n, device=DEV) % 2 == 0, 1.0, -1.0)
    y = (y * sig.to(BF16) + off.to(BF16)).contiguous()      # non-zero channel means
    s1, s2 = torch.zeros(n, dtype=F64, device=DEV), torch.zeros(n, dtype=F64, device=DEV)
    for rs in row_chunks(m, n):
        yd = y[rs].to(F64)
        s1 += yd.sum(0)
        s2 += (yd * yd).sum(0)
    stats = torch.stack([s1, s2]).float().contiguous()
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
    if mask_mode != "random":
        assert int(bits.max()) == int(bits.min()) == (0 if mask_mode == "zeros" else 255)
    return y, bits, mean, invstd, out


def tail_case(H, c, n, m, mask_mode, seed):
    """Operands of one launch, random mode: N(0, 1) gradients, filters of 0.1 N(0, 1), the statistics of the y behind the bits."""
    g = gen(seed)
    y, bits, mean, invstd, out = relu_bits(H, m, n, mask_mode, g)
    dy = randn_bf((m, c), g)
    wt = (0.1 * torch.randn((n, c), generator=g, device=DEV)).to(BF16).contiguous()
    g2 = randn_bf((m, n), g)
    return y, bits, mean, invstd, out, dy, wt, g2


def dev_ints(shape, amp, g):
    """float64_refs.ints drawn on the device (the largest case has 10^8 elements per tensor): integers uniform in {-amp .. amp}."""
    return torch.randint(-amp, amp + 1, shape, generator=g, device=DEV)


def exact_tail_case(H, c, n, m, mask_mode, seed):
    """Operands of one launch, exact mode: integer dy and filters of float64_refs.exact_amp's amplitude (g1 = dy wt^T has a
    standard deviation of 512 or more: a good share lies past 256, where bf16 no longer holds every integer), integer g2
    (|.| <= 64) and y (|.| <= 8), integer means (|.| <= 4), invstd in {1, 1/2, 1/4, 1/8}.  Every product and partial sum of the
    data gradient is an integer below C a^2 < 2^24, g1 + g2 is an integer, dz (y - mean) invstd an integer / 8 below 2^24: all of
    them fp32 numbers, so the kernel's dz and every TERM of its sums are exact, in whatever order they are formed."""
    g = gen(seed)
    bits = relu_bits(H, m, n, mask_mode, g)[1]
    a = exact_amp(c)
    assert c * a * a < TWO24
    dy, wt = dev_ints((m, c), a, g).to(BF16), dev_ints((n, c), a, g).to(BF16)
    g2, y = dev_ints((m, n), 64, g).to(BF16), dev_ints((m, n), 8, g).to(BF16)
    mean = dev_ints((n,), 4, g).float()
    invstd = torch.ldexp(torch.ones(n, device=DEV), -torch.randint(0, 4, (n,), generator=g, device=DEV)).float()
    return y, bits, mean, invstd, dy, wt, g2


def exact_dz(dy, wt, g2, bits):
    """The float64 definition dz = mask ? bf16(bf16(dy wt^T) + g2) : +0 as a bf16 tensor, and the share of |dy wt^T| > 256.
    Bit k of byte j of a row of `bits` belongs to channel 8 j + k."""
    m, n = g2.shape
    dz = torch.empty((m, n), dtype=BF16, device=DEV)
    wd = wt.to(F64).t().contiguous()
    shifts = torch.arange(8, device=DEV, dtype=torch.uint8)
    big = 0
    for rs in row_chunks(m, 2 * n):
        g1 = dy[rs].to(F64) @ wd
        big += int((g1.abs() > 256).sum())
        s = bf16_round(bf16_round(g1) + g2[rs].to(F64))
        mask = ((bits[rs].unsqueeze(2) >> shifts) & 1).reshape(-1, n).bool()
        dz[rs] = torch.where(mask, s, torch.zeros_like(s)).to(BF16)
    return dz, big / float(m * n)


def float64_sums(dz, y, mean, invstd):
    """The float64 column sums of the two reduce terms over the stored bf16 dz, and of their magnitudes: ([2, n], [2, n])."""
    m, n = dz.shape
    ref, mag = torch.zeros((2, n), dtype=F64, device=DEV), torch.zeros((2, n), dtype=F64, device=DEV)
    for rs in row_chunks(m, 2 * n):
        dzd = dz[rs].to(F64)
        t1 = dzd * (y[rs].to(F64) - mean.to(F64)) * invstd.to(F64)
        for q, terms in enumerate((dzd, t1)):
            ref[q] += terms.sum(0)
            mag[q] += terms.abs().sum(0)
    return ref, mag


def check_sums(label, got, ref, mag, depth):
    """|got - ref| <= depth u sum|term| for every column of both sums; prints the worst err / bound."""
    worst = 0.0
    for q in range(2):
        err, bnd = (got[q].to(F64) - ref[q]).abs(), depth * U * mag[q]
        i = int((err - bnd).argmax())
        ratio = float((err / (bnd + 1e-300)).max())
        worst = max(worst, ratio)
        print("tail %s sum %d: worst err / bound = %.3g" % (label, q, ratio))
        assert bool((err <= bnd).all()), "%s sum %d column %d: got %r ref %r bound %r" % (
            label, q, i, float(got[q][i]), float(ref[q][i]), float(bnd[i]))
    return worst


@pytest.mark.parametrize("case", TAIL_CASES, ids=[tail_case_id(case) for case in TAIL_CASES])
def test_tail_kernel_against_two_launches(H, case):
    """random mode: dz bit-identical to u2_conv_igemm (same variant word, streaming kernel) + u2_norm_bwd_reduce, both sums
    within tail_depth u sum|term| of the float64 sums of the same bf16 terms.  exact mode: dz bit-identical to the float64
    definition (no other kernel involved), column sum 0 equal wherever sum|dz| < 2^24 (every column on the 8-work-group grid:
    asserted), both sums under the same bound.  Three mask modes each.  With columns beyond C in the dy buffer (in_ld = C + 8:
    dy is a column window) the bytes outside the window hold 3e4, which must not reach dz."""
    c, n, m, tiny, mode, pad, regime = case
    b, h, w = MAPS[m] if regime == "prologue" else (1, 1, m)
    variant = FORCED_TINY if tiny else FORCED
    geo = stream_geometry(c, n, m, tiny, tail=True)
    assert_regime(geo, m, regime)
    d = tail_depth(c, n, m, tiny)
    code = K.K_STREAM + K.K_STREAM_TAIL + c // 32 * 10
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, mask_mode in enumerate(("random", "zeros", "ones")):
        label = "%dx%d m=%d %s %s %s" % (c, n, m, "tiny" if tiny else "prod", mode, mask_mode)
        seed = 1000 * k + c + m
        if mode == "exact":
            y, bits, mean, invstd, dy, wt, g2 = exact_tail_case(H, c, n, m, mask_mode, seed)
        else:
            y, bits, mean, invstd, out, dy, wt, g2 = tail_case(H, c, n, m, mask_mode, seed)
        if pad:
            wide = torch.full((m, c + pad), 3e4, dtype=BF16, device=DEV)
            wide[:, pad:] = dy
            dy_arg = wide[:, pad:]     # the window's first element; rows c + pad elements apart
        else:
            dy_arg = dy
        if mode == "exact":
            dz_ref, big = exact_dz(dy, wt, g2, bits)
            assert big > 0.25, "the data gradient hardly leaves bf16's integer range: %g" % big
            sums_ref = None
        else:
            # the two launches
            g1 = torch.empty((m, n), dtype=BF16, device=DEV)
            H.call("u2_conv_igemm", dy, wt, g1, None, None, b, h, w, c, c, h, w, n, n, 1, 1, 0, 0, 1, 1, 0, 0, variant)
            assert H.call_nostream("u2_conv_last_kernel") == K.K_STREAM + c // 32 * 10, "the data gradient did not run on the streaming kernel"
            dz_ref = torch.empty_like(g1)
            sums_ref = torch.zeros((2, n), device=DEV)
            H.call("u2_norm_bwd_reduce", g1, bits, y, mean, invstd, sums_ref, 1, m, n, n, 1, None, None, g2, dz_ref, None, 1)
        # the one launch
        dz = torch.full((m, n), 7.0, dtype=BF16, device=DEV)
        sums = torch.zeros((2, n), device=DEV)
        rc = H.call_status("u2_conv_dgrad_tail", dy_arg, wt, g2, y, bits, mean, invstd, dz, sums, b, h, w, c, c + pad, n, n, variant)
        assert rc == 0, "u2_conv_dgrad_tail declined a served shape"
        assert H.call_nostream("u2_conv_last_kernel") == code
        torch.cuda.synchronize()
        same = torch.equal(dz.view(torch.int16), dz_ref.view(torch.int16)) if mode == "exact" else torch.equal(dz, dz_ref)
        assert same, "%s: dz differs from the %s in %d elements" % (
            label, "float64 definition" if mode == "exact" else "two-launch path", int((dz.view(torch.int16) != dz_ref.view(torch.int16)).sum()))
        if mask_mode == "zeros":
            assert int((dz.view(torch.int16) != 0).sum()) == 0
        # the float64 sums of the same bf16 terms
        ref, mag = float64_sums(dz, y, mean, invstd)
        check_sums(label + " (fused)", sums, ref, mag, d)
        if sums_ref is not None:
            check_sums(label + " (two launches)", sums_ref, ref, mag, reduce_depth(1, m, n))
        if mode == "exact":
            small = mag[0] < TWO24
            if tiny:
                assert bool(small.all()), "precondition: sum|dz| = %g" % float(mag[0].max())
            print("tail %s: %d of %d columns of sum 0 must be exact" % (label, int(small.sum()), n))
            assert torch.equal(sums[0].to(F64)[small], ref[0][small]), "%s: sum 0 is not the exact integer in %d columns" % (
                label, int((sums[0].to(F64)[small] != ref[0][small]).sum()))
    torch.cuda.synchronize()
    print("tail %dx%d m=%d: %.2f s for the three mask modes" % (c, n, m, time.perf_counter() - t0))


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
def run_stage(F, H, monkeypatch, fuse, state, n_blocks=3, channels=(64, 256, 64), shape=(2, 13, 21), backward_fuse=None):
    """One forward / backward pass of a stage of n_blocks bottleneck blocks (channels: in, out, bottleneck) on a map of `shape`
    from `state` (parameters, input, output gradient); returns the captured tensors.  batch_norm_act is wrapped to reach the
    tails' tensors, _hip.call to count the reduce launches and to note the kernel behind every u2_conv_igemm launch,
    _hip.call_status to keep the operands, the outputs, the status and the kernel code of every u2_conv_dgrad_tail launch.
    backward_fuse: a list of switch positions - the graph is built once with `fuse` and its backward pass run once per entry, from
    the same forward tensors; a list of results is returned then."""
    from u2seg_amd.modeling.backbone import BottleneckBlock, ResNet

    F.set_tail_bwd_fuse(fuse)
    torch.manual_seed(0)
    c_in, c_out, c_mid = channels
    blocks = ResNet.make_stage(BottleneckBlock, n_blocks, in_channels=c_in, out_channels=c_out, stride_per_block=[1] * n_blocks,
                               bottleneck_channels=c_mid, norm="BN")
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
        state["x"] = randn_bf(tuple(shape) + (c_in,), gen(5))
        state["dout"] = randn_bf(tuple(shape) + (c_out,), gen(6))
    tails, calls, norms, igemm, fused = [], [], [], [], []
    real_bn, real_call, real_status = F.batch_norm_act, H.call, H.call_status

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
        rc = real_call(name, *args)
        if name == "u2_conv_igemm":   # (reduction width, output channels, filter taps, statistics asked for, kernel code)
            igemm.append((args[8], args[12], args[14] * args[15], args[4] is not None, H.call_nostream("u2_conv_last_kernel")))
        return rc

    def call_status(name, *args):
        if name != "u2_conv_dgrad_tail":
            return real_status(name, *args)
        # (dy and g2 are kept as copies made in front of the launch; y, bits, mean, invstd are the tail's saved tensors)
        rec = {"dy": args[0].clone(), "wd": args[1], "g2": args[2].clone(), "y": args[3], "bits": args[4], "mean": args[5],
               "invstd": args[6], "geom": args[9:16]}
        rec["rc"] = real_status(name, *args)
        rec["code"] = H.call_nostream("u2_conv_last_kernel")
        rec["dz"], rec["sums"] = args[7].clone(), args[8].clone()
        fused.append(rec)
        return rec["rc"]

    monkeypatch.setattr(F, "batch_norm_act", bn)
    monkeypatch.setattr(H, "call", call)
    monkeypatch.setattr(H, "call_status", call_status)
    x = state["x"].clone().requires_grad_(True)
    out = stage(x)
    runs = []
    flags = [fuse] if backward_fuse is None else list(backward_fuse)
    for i, flag in enumerate(flags):
        # (both the layer that would launch the fused form and the tail that would post its residual gradient look at the switch
        # when they run, so a graph built with it on takes the two launches while it is off)
        F.set_tail_bwd_fuse(flag)
        n_calls, n_fused = len(calls), len(fused)
        x.grad = None
        stage.zero_grad(set_to_none=True)
        F.reset_deferred_gradients()
        out.backward(state["dout"], retain_graph=i + 1 < len(flags))   # (the stage output's second handle receives nothing)
        torch.cuda.synchronize()
        F.assert_no_deferred_gradients()
        grads = {k: p.grad.clone() for k, p in stage.named_parameters()}
        runs.append({"tails": [dict(r) for r in tails], "norms": [dict(r) for r in norms], "calls": calls[n_calls:], "igemm": igemm,
                     "fused": fused[n_fused:], "dx": x.grad.clone(), "grads": grads, "stage": stage})
    monkeypatch.setattr(F, "batch_norm_act", real_bn)
    monkeypatch.setattr(H, "call", real_call)
    monkeypatch.setattr(H, "call_status", real_status)
    return runs[0] if backward_fuse is None else runs


def two_launches(F, H, run, k):
    """(g1, dz) of the tail of block k by u2_conv_igemm + u2_norm_bwd_reduce on the operands that run met: the gradient arriving at
    the conv1 output of block k + 1, that layer's data-gradient filter, the next tail's dz, the tail's saved tensors."""
    t = run["tails"][k]
    first = 3 if run["stage"][0].shortcut is None else 4   # norms of block 0: conv1, conv2, (shortcut,) conv3
    dy = run["norms"][first + 3 * k]["dx"].contiguous()      # conv1 of block k + 1
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


def test_stage_backward_fused_at_production_dispatch(H, monkeypatch):
    """Two bottleneck blocks 1024 -> 1024, bottleneck 256, on 8 x 50 x 84 (33 600 pixels), no variant word and no force bits: by
    the launcher's own fill rule (525 x 4 tiles >= 6 x 256 work-groups) the tail of block 0 is served inside block 1's conv1 data
    gradient on the production grid, 8 walkers per XCD and channel block with 8 or 9 tiles each against a ring of 5 - asserted
    from the geometry helper, the launch's status and its kernel code.  dz of the fused launch (its own output buffer) must be
    bit-equal to u2_conv_igemm (streaming kernel, production grid) + u2_norm_bwd_reduce on the operands the launch was given;
    the tail's dx / dz / dgamma / dbeta meet the float64 closed form under check_backward's bounds at the depth of the new
    epilogue on this grid (the forward statistics come from conv3's epilogue on the same grid: asserted).
    The two-launch form is a second backward pass over the SAME graph with the switch off: on this grid two forward passes are
    not bit-equal (every norm's statistics are sums of atomics; measured: 268 412 of 34 406 400 elements of block 0's conv3 output
    differ between two passes), a ReLU bit that differs moves the stage input gradient by a whole element of dz (0.29
    max-normalised), and the guards of the module's docstring - the two forms differ only in the order of the fp32 additions behind
    the sums - hold between backward passes from one forward state, which is what they are asserted on."""
    from u2seg_amd.layers import functional as F

    monkeypatch.delenv("U2_CONV_VARIANT", raising=False)
    shape, (c_in, c_out, c_mid) = (8, 50, 84), (1024, 1024, 256)
    m = shape[0] * shape[1] * shape[2]
    geo = stream_geometry(c_mid, c_out, m, False, tail=True)
    assert geo["served_unforced"] and geo["nwalk"] == 8 and walker_tiles(geo) == [8, 9] and geo["ring"] == 5
    was = F.TAIL_BWD_FUSE
    state = {}
    try:
        off, on = run_stage(F, H, monkeypatch, True, state, 2, (c_in, c_out, c_mid), shape, backward_fuse=[False, True])
        built_off = run_stage(F, H, monkeypatch, False, state, 2, (c_in, c_out, c_mid), shape)
    finally:
        F.set_tail_bwd_fuse(was)
    n_off, n_on = off["calls"].count("u2_norm_bwd_reduce"), on["calls"].count("u2_norm_bwd_reduce")
    print("u2_norm_bwd_reduce calls: %d with two launches, %d fused" % (n_off, n_on))
    assert not off["fused"] and len(on["fused"]) == 1
    # a graph built with the switch off makes the launches of the off pass, name for name (its values belong to another forward
    # pass and are compared with nothing)
    assert not built_off["fused"] and built_off["calls"] == off["calls"]
    fz = on["fused"][0]
    assert fz["rc"] == 0 and fz["code"] == K.K_STREAM + K.K_STREAM_TAIL + 80, (fz["rc"], fz["code"])
    assert tuple(fz["geom"]) == shape + (c_mid, c_mid, c_out, c_out)
    assert n_on == n_off - 1, "the fused path was not taken (a silent fall-back)"
    # the forward statistics behind mean / invstd: both conv3 launches ran on the streaming kernel's production grid
    conv3 = [rec for rec in on["igemm"] if rec[:4] == (c_mid, c_out, 1, True)]
    assert len(conv3) == 2 and all(rec[4] == K.K_STREAM + 80 for rec in conv3), conv3
    d_new = tail_depth(c_mid, c_out, m, tiny=False)
    # the fused launch against the two launches on its own operands
    g1, dz2 = torch.empty_like(fz["dz"]), torch.empty_like(fz["dz"])
    H.call("u2_conv_igemm", fz["dy"], fz["wd"], g1, None, None, *shape, c_mid, c_mid, shape[1], shape[2], c_out, c_out, 1, 1, 0, 0, 1, 1,
           0, 0, FORCED)
    assert H.call_nostream("u2_conv_last_kernel") == K.K_STREAM + 80
    sums2 = torch.zeros((2, c_out), device=DEV)
    H.call("u2_norm_bwd_reduce", g1, fz["bits"], fz["y"], fz["mean"], fz["invstd"], sums2, 1, m, c_out, c_out, 1, None, None, fz["g2"],
           dz2, None, 1)
    torch.cuda.synchronize()
    assert torch.equal(fz["dz"], dz2), "dz of the fused tail is not the two launches' on the same operands: %d elements differ" % int(
        (fz["dz"] != dz2).sum())
    ref, mag = float64_sums(fz["dz"].view(m, c_out), fz["y"].view(m, c_out), fz["mean"], fz["invstd"])
    check_sums("stage 256x1024 m=%d prod (fused)" % m, fz["sums"], ref, mag, d_new)
    # the closed form: block 0's tail in the fused run
    t = on["tails"][0]
    assert t["y"].data_ptr() == fz["y"].data_ptr() and torch.equal(on["tails"][1]["dz"], fz["g2"])
    nref = NormRef(t["y"].detach().view(1, m, c_out), t["gamma"], t["beta"], 1, d_new * U)
    gamma, beta = torch.nn.Parameter(t["gamma"].detach()), torch.nn.Parameter(t["beta"].detach())
    gamma.grad, beta.grad = on["grads"]["0.conv3.norm.weight"], on["grads"]["0.conv3.norm.bias"]
    check_backward(nref, "block 0 tail (fused, production grid)", [g1.view(1, m, c_out), fz["g2"].view(1, m, c_out)],
                   t["out"].detach().view(1, m, c_out), True, t["dx"].view(1, m, c_out), gamma, beta, d_new, fz["dz"].view(1, m, c_out))
    r = max_rel(on["dx"], off["dx"])
    print("stage input gradient at production dispatch, fused against two launches: %.3g" % r)
    assert r <= 2.0 ** -6
    worst = max((max_rel(g, off["grads"][k]), k) for k, g in on["grads"].items())
    print("parameter gradients at production dispatch, fused against two launches: worst %.3g (%s)" % worst)
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
