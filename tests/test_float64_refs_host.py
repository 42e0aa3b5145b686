"""CPU checks of tests/float64_refs.py, the float64 references tests/test_gpu_optim_resample_float64.py and
tests/test_gpu_conv_float64.py compare the HIP kernels with: each reference is held against an independent formulation in torch, so that a GPU test cannot pass or fail
because of a mistake in its own yardstick."""
import pytest
import torch
import torch.nn.functional as TF

from tests import float64_refs as R

F64 = torch.float64


def test_chunk_tables_tile_the_arena():
    ct, cb, cl, fc = R.chunk_tables(R.A2_SIZES)
    assert cb[0] == 0 and all(cb[i] + cl[i] == cb[i + 1] for i in range(len(cb) - 1)) and cb[-1] + cl[-1] == sum(R.A2_SIZES)
    assert [fc[t + 1] - fc[t] for t in range(len(R.A2_SIZES))] == [1, 1, 1, 1, 1, 1, 2, 4, 1, 1]
    starts = [sum(R.A2_SIZES[:t]) for t in range(len(R.A2_SIZES))]
    assert {s & 3 for s in starts} == {0, 1, 2, 3}
    for t, s in enumerate(starts):   # no chunk crosses a tensor
        for c in range(fc[t], fc[t + 1]):
            assert ct[c] == t and s <= cb[c] and cb[c] + cl[c] <= s + R.A2_SIZES[t]
    assert sum(R.A2_SIZES) < 1 << 20


@pytest.mark.parametrize("mom,clip,scale", [(0.9, 1.0, 1.0), (0.9, 1.0, 0.125), (0.0, 1.0, 0.5), (0.9, 0.0, 0.5)])
def test_sgd_clip_ref_equals_torch_sgd(mom, clip, scale):
    """sgd_clip_ref against torch.optim.SGD in float64 after per-parameter clip_grad_norm_(p, clip, 2.0) on gradients
    pre-scaled by `scale` (solver/build.py of the reference: one clip call per parameter), three steps, per-tensor weight decay
    through parameter groups; tensors above and below the clip threshold and an all-zero gradient.  1e-12 relative."""
    sizes = R.A2_SIZES
    g = torch.Generator().manual_seed(11)
    lr = 0.1
    wd = [(0.0, 1e-4, 5e-2)[t % 3] for t in range(len(sizes))]
    params = [torch.nn.Parameter(torch.randn(n, generator=g, dtype=F64)) for n in sizes]
    opt = torch.optim.SGD([{"params": [p], "weight_decay": w} for p, w in zip(params, wd)], lr=lr, momentum=mom)
    p = torch.cat([q.detach().clone() for q in params])
    m = torch.zeros_like(p)   # torch's first step: buf = grad, which is mom * 0 + grad
    for it in range(3):
        grads = []
        for t, n in enumerate(sizes):
            gt = torch.randn(n, generator=g, dtype=F64)
            target = (20.0, 0.05)[t % 2] / scale      # ||g|| scale above / below the threshold
            grads.append(gt * 0 if t == 2 else gt * (target / gt.norm()))
        for q, gt in zip(params, grads):
            q.grad = gt * scale
            if clip > 0:
                torch.nn.utils.clip_grad_norm_(q, clip, 2.0)
        opt.step()
        p, m = R.sgd_clip_ref(p, torch.cat(grads), m, sizes, wd, lr, mom, clip, scale)
        want_p = torch.cat([q.detach() for q in params])
        assert float((p - want_p).abs().max()) <= 1e-12 * float(want_p.abs().max()), it
        if mom:
            want_m = torch.cat([opt.state[q]["momentum_buffer"] for q in params])
            assert float((m - want_m).abs().max()) <= 1e-12 * float(want_m.abs().max()), it


@pytest.mark.parametrize("shape", [(2, 64, 13, 18), (1, 8, 1, 1), (1, 8, 2, 1), (3, 16, 1, 7), (2, 32, 14, 2), (1, 24, 5, 5)])
def test_slots_from_indices_equals_brute_force(shape):
    """The conversion of max_pool2d's return_indices to window slots against a scan of the nine taps (first maximum wins),
    on the tie-quantised input: every window holds ties, many hold negative values only."""
    x = R.tie_values(shape, torch.Generator().manual_seed(sum(shape)), "cpu")
    y, ind = TF.max_pool2d(x, 3, 2, 1, return_indices=True)
    best, slot = R.brute_force_slots(x)
    assert torch.equal(y, best)
    assert torch.equal(R.slots_from_indices(ind, shape[3]), slot)
    # the band form (explicit -inf rows, no vertical padding) names the same slots
    xb = TF.pad(x, (0, 0, 1, 1), value=float("-inf"))
    if xb.shape[2] >= 3:
        yb, indb = TF.max_pool2d(xb, 3, 2, (0, 1), return_indices=True)
        n = yb.shape[2]
        assert torch.equal(yb, best[:, :, :n]) and torch.equal(R.slots_from_indices(indb, shape[3], row_off=0), slot[:, :, :n])


def test_stem_unfold_ref_reproduces_conv2d():
    """unfold + the (kh, kw, c) reordering, multiplied by weight.permute(0, 2, 3, 1).reshape(64, 147), is conv2d(7x7, stride 2,
    pad 3) in float64; pixels outside the images and the conv padding give exact zeros."""
    g = torch.Generator().manual_seed(5)
    imgs = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in ((50, 70), (64, 61), (1, 1), (16, 32))]
    mean, std = torch.tensor([123.675, 116.28, 103.53]), torch.tensor([58.395, 57.12, 57.375])
    canvas, inside = R.stem_canvas(imgs, mean, std, 64, 96)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=F64)
    cols = R.stem_unfold_ref(canvas)
    assert cols.shape == (4, 32 * 48, 147)
    got = (cols @ w.permute(0, 2, 3, 1).reshape(64, 147).t()).view(4, 32, 48, 64).permute(0, 3, 1, 2)
    want = TF.conv2d(canvas, w, None, 2, 3)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((cols[R.stem_unfold_ref(inside) == 0] == 0).all())
    # image 2 is one pixel: only the windows that contain canvas pixel (0, 0) see it, at tap (3 - 2 oy, 3 - 2 ox)
    one = cols[2].view(32, 48, 7, 7, 3)
    assert int((one != 0).any(-1).sum()) == 4 and bool((one[1, 1, 1, 1] == canvas[2, :, 0, 0]).all())


# ---- the convolution references of tests/test_gpu_conv_float64.py ----
def test_rne_bf16_on_hand_made_ties():
    """bf16 keeps 8 significant bits: in [1, 2) the step is 2^-7, in [256, 512) it is 2.  Exact ties go to the even neighbour, a
    hair above or below a tie goes to the nearer one, bf16 values come back unchanged, the sign is symmetric."""
    s = 2.0 ** -7
    cases = [(1 + s / 2, 1.0), (1 + 3 * s / 2, 1 + 2 * s), (1 + s / 2 + 2.0 ** -40, 1 + s), (1 + 3 * s / 2 - 2.0 ** -40, 1 + s),
             (257.0, 256.0), (259.0, 260.0), (258.0, 258.0), (261.0, 260.0), (263.0, 264.0), (255.5, 256.0), (254.5, 254.0),
             (511.0, 512.0), (513.0, 512.0), (515.0, 516.0), (2.0 - s / 2, 2.0), (0.0, 0.0), (2.0 ** -10 * (1 + s / 2), 2.0 ** -10),
             (3.0 * 2.0 ** 20, 3.0 * 2.0 ** 20), (65.0 + 0.25, 65.0), (65.0 + 0.75, 66.0)]
    x = torch.tensor([c[0] for c in cases], dtype=F64)
    want = torch.tensor([c[1] for c in cases], dtype=F64)
    assert torch.equal(R.rne_bf16(x), want)
    assert torch.equal(R.rne_bf16(-x), -want)
    # float64 -> bf16 in one rounding is what torch does from fp32 for fp32 values; random fp32 values agree with torch's cast
    r = torch.randn(100000, generator=torch.Generator().manual_seed(1)).to(F64) * 300
    assert torch.equal(R.rne_bf16(r), r.float().bfloat16().to(F64))
    lo, hi = R.bf16_interval(torch.tensor([257.0, -3.0, 1.0], dtype=F64), torch.tensor([0.5, 0.5, 0.0], dtype=F64), relu=True)
    assert lo.tolist() == [256.0, 0.0, 1.0] and hi.tolist() == [258.0, 0.0, 1.0]
    lo, hi = R.bf16_interval(torch.tensor([257.0], dtype=F64), torch.tensor([0.0], dtype=F64), old=torch.tensor([3.0], dtype=F64))
    assert lo.tolist() == [260.0] and hi.tolist() == [260.0]   # bf16(257) = 256, bf16(259) = 260 (tie to even)


@pytest.mark.parametrize("geom", R.GENERIC_GEOMS + [R.ASYM_GEOM] + R.STRIDE2_GEOMS + R.HALO_GEOMS[:4])
def test_conv_refs_equal_torch_conv2d_and_autograd(geom):
    """unfold + matmul (forward), its transpose + fold (data gradient) and dy cols^T (weight gradient) against
    torch.nn.functional.conv2d in float64 and its autograd: strides 1 and 2, asymmetric filter and padding, one-pixel / one-row /
    one-column maps.  The magnitude sums are the same operations on |operands|: positive operands give A == |value|."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    x, wt, bias, gy, _ = R.conv_operands(geom, "real")
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    want = TF.conv2d(xr, wr, br, stride, (ph, pw))
    want.backward(gy)
    want = want.detach()
    tol = lambda t: 1e-12 * float(t.abs().max()) + 1e-300
    y, a = R.conv_fwd_ref(x, wt, stride, ph, pw, bias)
    assert y.shape == want.shape == gy.shape
    assert float((y - want).abs().max()) <= tol(want)
    dx, adx = R.conv_dgrad_ref(gy, wt, (h, w), stride, ph, pw)
    assert dx.shape == x.shape and float((dx - xr.grad).abs().max()) <= tol(xr.grad)
    dw, adw = R.conv_wgrad_ref(x, gy, kh, kw, stride, ph, pw)
    assert dw.shape == wt.shape and float((dw - wr.grad).abs().max()) <= tol(wr.grad)
    assert float((gy.sum((0, 2, 3)) - br.grad).abs().max()) <= tol(br.grad)
    # magnitude sums: >= |value| everywhere, and the value itself on |operands|
    assert bool((a >= y.abs() - tol(y)).all()) and bool((adx >= dx.abs() - tol(dx)).all()) and bool((adw >= dw.abs() - tol(dw)).all())
    ya, _ = R.conv_fwd_ref(x.abs(), wt.abs(), stride, ph, pw, bias.abs())
    assert float((ya - a).abs().max()) <= tol(a)
    dxa, _ = R.conv_dgrad_ref(gy.abs(), wt.abs(), (h, w), stride, ph, pw)
    assert float((dxa - adx).abs().max()) <= tol(adx)
    dwa, _ = R.conv_wgrad_ref(x.abs(), gy.abs(), kh, kw, stride, ph, pw)
    assert float((dwa - adw).abs().max()) <= tol(adw)


@pytest.mark.parametrize("geom", sorted(set(R.ALL_CONV_GEOMS)))
def test_exact_generator_preconditions(geom):
    """Every shape of the GPU module: the exact-input operands are integers that bf16 holds (|v| <= 256), and the magnitude sums
    of the forward (+ bias), the data gradient, the weight gradient and the column sums of the outputs stay below 2^24 - any
    order of fp32 additions is then exact.  The low-amplitude form also keeps the sums of squares there."""
    b, h, w, cin, cout, kh, kw, stride, ph, pw = geom
    x, wt, bias, gy, old = R.conv_operands(geom, "exact")
    for t in (x, wt, gy):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256
    for t in (bias, old):
        assert torch.equal(R.rne_bf16(t), t)
    y, a = R.conv_fwd_ref(x, wt, stride, ph, pw, bias)
    assert float(a.max()) < R.TWO24
    yy = R.rne_bf16(y)
    assert float(yy.abs().sum((0, 2, 3)).max()) < R.TWO24
    assert float(R.conv_dgrad_ref(gy, wt, (h, w), stride, ph, pw)[1].max()) < R.TWO24
    assert float(R.conv_wgrad_ref(x, gy, kh, kw, stride, ph, pw)[1].max()) + 256 < R.TWO24
    assert float(gy.abs().sum((0, 2, 3)).max()) < R.TWO24
    if geom in R.VARIANT_SHAPES + R.HALO_GEOMS:
        x1, w1, _, _, _ = R.conv_operands(geom, "exact", amp=1)
        y1 = R.conv_fwd_ref(x1, w1, stride, ph, pw)[0]
        assert torch.equal(R.rne_bf16(y1) ** 2, y1 ** 2) and float((y1 * y1).sum((0, 2, 3)).max()) < R.TWO24


def test_activation_like_operands():
    """The realistic generator: bf16 values, non-negative activations with one all-zero channel and a channel holding 2^6,
    per-channel means apart, gradients at 2^-10."""
    x, wt, bias, gy, old = R.conv_operands(R.VARIANT_SHAPES[0], "real")
    for t in (x, wt, bias, gy, old):
        assert torch.equal(R.bf16_round(t), t)
    assert float(x.min()) >= 0 and float(x[:, 0].abs().max()) == 0 and int((x[:, 1] == 64).sum()) >= 1
    means = x.mean((0, 2, 3))
    assert float(means.max()) > 3.5 and float(means[2:].min()) < 0.6
    assert 2.0 ** -11 < float(gy.std()) < 2.0 ** -9
    assert float(wt.mean((1, 2, 3)).abs().max()) > 0.2 / (64 * 9)


# ---- inference tails (tests/test_gpu_inference_tails_float64.py) ----
@pytest.mark.parametrize("p", R.PASTE_P)
def test_paste_ref_equals_oracle_on_exact_inputs(p):
    """paste_ref against OracleModel.paste_masks (grid_sample in fp32, then >= 0.5) on the exact inputs of the GPU test, every
    canvas: the sampled value is an fp32 number (so the fp32 oracle computes it without error) and not one pixel differs.  The
    constant-0.5 map has pixels exactly on the threshold, all on; the map one step below it is all off."""
    from oracle.model import OracleModel

    on_thr = 0
    for h, w in R.PASTE_CANVASES:
        probs, boxes = R.paste_exact_case(p, h, w)
        side = torch.cat([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]])
        assert bool((torch.log2(side) == torch.log2(side).round()).all()) and float(side.max()) <= 32
        assert torch.equal(boxes * 4, (boxes * 4).round()) and torch.equal(probs * 256, (probs * 256).round())
        assert (boxes.shape[0] * h * w) % 16 != 0 or (h * w) % 16 == 0
        v, inside = R.paste_ref(probs, boxes, h, w)
        assert torch.equal(v, v.float().to(F64)), (p, h, w)
        assert not bool(v[~inside].any())
        want = inside & (v >= 0.5)
        assert torch.equal(want, OracleModel.paste_masks(probs, boxes, (h, w))), (p, h, w)
        assert torch.equal(v, R.paste_fp32(probs, boxes, h, w).to(F64)), (p, h, w)
        on_thr += int((v[R.PASTE_HALF] == 0.5).sum())
        assert not bool(want[R.PASTE_BELOW].any()) and bool(inside[R.PASTE_BELOW].any()) == bool(inside[R.PASTE_HALF].any())
        assert bool(want[R.PASTE_HALF][v[R.PASTE_HALF] == 0.5].all())
        assert not bool(inside[1].any()) and not bool(inside[3].any())      # boxes wholly right of / below the canvas
    assert on_thr >= 3, on_thr


@pytest.mark.parametrize("p", [1, 7, 28])
def test_paste_ref_equals_grid_sample_float64(p):
    """paste_ref against torch's grid_sample in float64 on random fp32 inputs (values to 1e-13), and the `inside` predicate
    against where a map of ones samples to something positive."""
    h, w = 45, 53
    probs, boxes = R.paste_random_case(p, h, w, 6, 3)
    v, inside = R.paste_ref(probs, boxes, h, w)
    b = boxes.to(F64)
    gy = (torch.arange(h, dtype=F64) + 0.5 - b[:, 1:2]) / (b[:, 3:4] - b[:, 1:2]) * 2 - 1
    gx = (torch.arange(w, dtype=F64) + 0.5 - b[:, 0:1]) / (b[:, 2:3] - b[:, 0:1]) * 2 - 1
    grid = torch.stack([gx[:, None, :].expand(-1, h, w), gy[:, :, None].expand(-1, h, w)], dim=3)
    ref = TF.grid_sample(probs[:, None].to(F64), grid, align_corners=False)[:, 0]
    assert float((v - ref).abs().max()) <= 1e-13
    ones = TF.grid_sample(torch.ones_like(probs[:, None], dtype=F64), grid, align_corners=False)[:, 0]
    assert torch.equal(inside, ones > 0)
    assert 0.05 < float(inside.double().mean()) < 0.95


@pytest.mark.parametrize("s", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", R.SEM_MAPS + [(9, 11)])
def test_upsample_ref_equals_interpolate_float64(hw, s):
    g = torch.Generator().manual_seed(s)
    x = torch.randn((2, hw[0], hw[1], 16), generator=g).bfloat16()
    ref = TF.interpolate(x[..., :9].to(F64).permute(0, 3, 1, 2), scale_factor=s, mode="bilinear", align_corners=False)
    got = R.upsample_ref(x, 9, s)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-14 * 8


@pytest.mark.parametrize("k,cp", R.SEM_EXACT_CASES)
def test_upsample_exact_case_is_exact_and_holds_its_ties(k, cp):
    """The exact-input generator: bf16 values, |v| <= 32, multiples of 1/4; the float64 upsampling is an fp32 number everywhere;
    the ties it promises are there (so first-index-wins is really exercised) and first_argmax == torch.argmax."""
    for h, w in R.SEM_MAPS:
        for s in (2, 4):
            x = R.upsample_exact_case(2, h, w, cp, k, 1e30)
            xk = x[..., :k]
            assert torch.equal(xk, xk.bfloat16().to(F64)) and float(xk.abs().max()) <= 32 and torch.equal(xk * 4, (xk * 4).round())
            assert bool((x[1, ..., :k] < 0).all())
            ref = R.upsample_ref(x, k, s)
            assert torch.equal(ref, ref.float().to(F64))
            am = R.first_argmax(ref)
            assert torch.equal(am, ref.argmax(1))
            assert int(am[0, 0, 0]) == 0 and bool((ref[0, :, 0, 0] == ref[0, 0, 0, 0]).all())
            if k > 1:
                n_max = (ref == ref.max(1, keepdim=True).values).sum(1)
                assert bool((n_max > 1).any()) and bool((am != k - 1).all())   # the copy never wins over the channel it copies
                assert h * w == 1 or bool((am > 0).any())


def _resize_cases():
    return [((150, 200), (225, 300)), ((33, 47), (160, 224)), ((160, 224), (97, 133)), ((1, 47), (8, 100)), ((33, 1), (50, 7)),
            ((33, 47), (1, 1)), ((12, 20), (24, 40)), ((12, 20), (6, 10)), ((21, 13), (21, 13))]


@pytest.mark.parametrize("src,dst", _resize_cases())
def test_resize_ref_equals_interpolate_float64(src, dst):
    """resize_ref forms the scale in fp32 like ATen's fp32 kernel; ATen's float64 kernel forms it in float64.  The two source
    coordinates differ by at most 2^-24 scale (dst + 0.5) <= 2^-24 Hin (Win) per axis, bilinear interpolation is continuous and
    piecewise linear, so the values differ by at most 2^-24 (Hin + Win) times the largest step between neighbouring inputs.
    Power-of-two scales are the same number in both formats: equal to float64 round-off there."""
    g = torch.Generator().manual_seed(src[0] * 7 + dst[1])
    x = torch.randn((3,) + src, generator=g)
    ref = TF.interpolate(x.to(F64)[None], size=dst, mode="bilinear", align_corners=False)[0]
    got = R.resize_ref(x, *dst)
    step = max(float((x[:, 1:] - x[:, :-1]).abs().max()) if src[0] > 1 else 0.0,
               float((x[:, :, 1:] - x[:, :, :-1]).abs().max()) if src[1] > 1 else 0.0)
    exact_scale = all(float(torch.tensor(float(a)) / torch.tensor(float(b))) == a / b for a, b in zip(src, dst))
    bound = 1e-14 if exact_scale else 2.0 ** -24 * (src[0] + src[1]) * step
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= bound, (float((got - ref).abs().max()), bound)


@pytest.mark.parametrize("n,side,c,k", [(37, 7, 264, 800), (1, 1, 8, 1), (3, 14, 1024, 5), (2, 28, 64, 9)])
def test_mask_prob_ref_equals_conv2d_float64_and_channel_pick(n, side, c, k):
    """mask_prob_ref against the reference's order of operations - the K-channel 1x1 conv in float64 on the bf16-rounded operands,
    the predicted class's channel, bf16 rounding, sigmoid - on the exact-input generator (equal: every sum is exact) and on
    random weights (the float64 sums may differ in the last bit, so the rounded logits may differ on a rounding boundary: none
    does at these sizes).  The generator's claims: integer multiples of 2^-8 below 2^24 of them, some exact halves."""
    x, w, b, cls, ax, aw = R.mask_prob_case(n, side, c, k)
    assert torch.equal(x, x.bfloat16().to(F64)) and torch.equal(w, w.bfloat16().float()) and torch.equal(b, b.bfloat16().float())
    assert c * ax * aw + 255 < 1 << 24 and int(cls[0]) == 0 and int(cls[-1]) == k - 1
    g = torch.Generator().manual_seed(5)
    for wt, bs in ((w, b), (torch.randn((k, c), generator=g) / c ** 0.5, torch.randn(k, generator=g) * 0.1)):
        prob, z = R.mask_prob_ref(x, wt, bs, cls)
        conv = TF.conv2d(x.permute(0, 3, 1, 2), R.bf16_round(wt).view(k, c, 1, 1), R.bf16_round(bs))   # [n, k, side, side]
        sel = torch.gather(conv, 1, cls.view(n, 1, 1, 1).expand(n, 1, side, side))
        assert torch.equal(z, R.rne_bf16(sel)) and torch.equal(prob, torch.sigmoid(R.rne_bf16(sel)))
        assert torch.equal(z, sel.float().bfloat16().to(F64))   # torch's own fp32 -> bf16 rounding of the (here exact) sums
    if n * side * side >= 500:
        exact = torch.einsum("nyxc,nc->nyx", x, w.to(F64)[cls]) + b.to(F64)[cls].view(-1, 1, 1)
        a = exact.abs()
        ulp = 2.0 ** (torch.floor(torch.log2(a.clamp(min=2.0 ** -20))) - 7)
        half = (a >= 1) & (torch.remainder(a / ulp, 1.0) == 0.5)
        assert int(half.sum()) >= 3 and float(((a >= 1) & (a <= 8)).double().mean()) > 0.3


# ----------------------------------------------------------------------------------------------------------------------------
# box decisions (tests/test_gpu_box_decisions_float64.py): each reference against the oracle's restatement of the same reference
# routine - in float64 where the oracle takes it, else in fp32 on exact inputs, where the two precisions must agree bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
EDGE_GT, EDGE_CAND = R.EDGE_GT, R.EDGE_CAND


def test_iou_ref_equals_the_oracle_in_both_precisions():
    """Integer boxes: iou_ref == oracle.pairwise_iou run in fp32 (exact operands, one correctly rounded division) and == the fp32
    rounding of the oracle run in float64, bit for bit; fractional boxes: within one fp32 ulp of the float64 oracle."""
    from oracle import ops as O

    g = torch.Generator().manual_seed(1)
    gt, cand = R.int_boxes(37, g), R.int_boxes(1000, g)
    cand[:20] = gt[:20]                          # IoU 1
    cand[20] = torch.tensor([2000.0, 2000.0, 2047.0, 2047.0])
    ref = R.iou_ref(gt, cand)
    assert ref.dtype == torch.float32 and ref.shape == (37, 1000)
    assert torch.equal(ref, O.pairwise_iou(gt, cand)) and torch.equal(ref, O.pairwise_iou(gt.double(), cand.double()).float())
    assert float(ref.max()) == 1.0 and float(ref[:, 20].max()) == 0.0 and 0.1 < float((ref > 0).float().mean()) < 0.9
    edge = R.iou_ref(EDGE_GT, EDGE_CAND)[0]
    want = torch.tensor([0.5, 0.3, 0.7, 1.0, 0.0, 0.2, 0.4, 0.6, 0.8, 0.0], dtype=torch.float32)   # touching boxes: 0
    assert torch.equal(edge, want)
    frac = torch.rand((50, 4), generator=g) * 50
    frac[:, 2:] += frac[:, :2]
    assert float((R.iou_ref(frac[:10], frac) - O.pairwise_iou(frac[:10].double(), frac.double())).abs().max()) <= 2.0 ** -24


@pytest.mark.parametrize("lo,hi", [(0.3, 0.7), (0.5, 0.5)])
@pytest.mark.parametrize("allow", [False, True])
def test_match_ref_equals_the_oracle_matcher(lo, hi, allow):
    """match_ref == oracle.matcher on oracle.pairwise_iou, fp32 and float64 (integer boxes): random boxes with many tied maxima,
    identical ground truths (first index), IoUs exactly on 0.3 / 0.5 / 0.7 - RN32(3/10) == float32(0.3), so that candidate is NOT
    below lo -, a ground truth that overlaps nothing (the low-quality rule then marks every candidate positive), no ground truth."""
    from oracle import ops as O

    g = torch.Generator().manual_seed(2)
    gt, cand = R.int_boxes(6, g), R.int_boxes(700, g)
    gt[4] = gt[1]
    cases = [(gt, cand), (EDGE_GT, EDGE_CAND), (torch.cat([gt, torch.tensor([[1000.0, 1000.0, 1010.0, 1010.0]])]), cand),
             (gt[:0], cand)]
    for gi, ci in cases:
        m, lab, val = R.match_ref(gi, ci, lo, hi, allow)
        for dt in (torch.float32, torch.float64):
            mq = O.pairwise_iou(gi.to(dt), ci.to(dt))
            om, ol = O.matcher(mq.float(), [lo, hi], [0, -1, 1], allow)
            assert torch.equal(m, om) and torch.equal(lab, ol), (gi.shape, dt)
        if gi.shape[0]:
            assert torch.equal(val, O.pairwise_iou(gi, ci).max(dim=0).values)
    m, lab, _ = R.match_ref(EDGE_GT, EDGE_CAND, lo, hi, False)
    if (lo, hi) == (0.3, 0.7):
        assert lab.tolist() == [-1, -1, 1, 1, 0, 0, -1, -1, 1, 0]       # 3/10 is not below 0.3, 7/10 not below 0.7
    else:
        assert lab.tolist() == [1, 0, 1, 1, 0, 0, 0, 1, 1, 0]           # 1/2 is not below 0.5
    m, lab, _ = R.match_ref(gt, cand, lo, hi, False)
    assert not bool((m == 4).any()) and bool((m == 1).any())              # the identical pair: the first index
    if allow:
        assert bool((R.match_ref(cases[2][0], cand, lo, hi, True)[1] == 1).all())


def test_nms_ref_equals_the_oracle_nms():
    """nms_ref == oracle.ops.nms (the C restatement, fp32) on integer boxes: random grouped boxes at 0.5 / 0.65 / 0.7, every
    construction the GPU test uses, and max_keep as a prefix of the unlimited result.  The constructions' own claims (which
    positions die and why) are asserted here as well."""
    from oracle import ops as O

    def both(boxes, groups, thr, max_keep=None):
        n = boxes.shape[0]
        keep = R.nms_ref(boxes, groups, thr, n if max_keep is None else max_keep)
        want = O.nms(boxes, torch.arange(n, 0, -1).float(), thr, groups).tolist()
        assert keep == want[: len(keep)] and (max_keep is not None or len(keep) == len(want)), (n, thr)
        return keep

    g = torch.Generator().manual_seed(3)
    for thr in (0.5, 0.65, 0.7):
        b = R.int_boxes(300, g, span=32, min_side=40)
        grp = torch.randint(0, 3, (300,), generator=g)
        full = both(b, grp, thr)
        assert 20 < len(full) < 280
        assert both(b, grp, thr, 37) == full[:37]
        pairs = R.nms_threshold_pairs(thr)
        assert both(pairs, torch.zeros(4, dtype=torch.int64), thr) == [0, 1, 2]
    zero = torch.zeros(300, dtype=torch.int64)
    assert both(R.nms_ladder(300), zero, 0.5) == list(range(0, 300, 2))
    assert both(R.nms_ladder(300, 1), zero, 0.5) == [0] + list(range(1, 300, 2))
    b, dead = R.nms_lazy_column_case()
    assert both(b, zero, 0.5) == [i for i in range(300) if i not in dead]
    iou = R.nms_iou_ref(b)
    for v in list(range(130, 141)):                 # suppressed by position 3 and by nothing else
        assert [i for i in range(v) if float(iou[i, v]) > 0.5] == [3], v
    assert [i for i in range(200) if float(iou[i, 200]) > 0.5] == [3, 130]
    assert float(iou[4, 5]) > 0.5
    for v in range(150, 156):                       # position 5 would suppress them; nothing else does
        assert [i for i in range(v) if float(iou[i, v]) > 0.5] == [5], v
    b, dead = R.nms_helper_stride_case()
    assert both(b, torch.zeros(400, dtype=torch.int64), 0.5) == [i for i in range(400) if i not in dead]
    iou = R.nms_iou_ref(b)
    assert [i for i in range(390) if float(iou[i, 390]) > 0.5] == [200] and [i for i in range(395) if float(iou[i, 395]) > 0.5] == [5]
    same = torch.tensor([[5.0, 5.0, 25.0, 30.0]]).repeat(129, 1)
    assert both(same, torch.zeros(129, dtype=torch.int64), 0.5) == [0]
    assert both(same, torch.arange(129) % 3, 0.5) == [0, 1, 2]
    flat = torch.tensor([[10.0, 10.0, 10.0, 20.0]] * 3 + [[5.0, 5.0, 5.0, 5.0]] * 2 + [[8.0, 8.0, 12.0, 22.0]])
    assert both(flat, torch.zeros(6, dtype=torch.int64), 0.5) == list(range(6))     # 0 / 0 suppresses nothing
    assert both(R._grid_boxes(300), zero, 0.5, 100) == list(range(100))


def test_levels_ref_equals_the_oracle_on_float64_inputs_and_at_the_boundaries():
    """levels_ref == oracle.assign_boxes_to_levels on the same boxes cast to float64, and on the boundary boxes also == the oracle
    in fp32; the boundary boxes land on the upper side."""
    from oracle import ops as O

    b = R.level_boundary_boxes()
    g = torch.Generator().manual_seed(4)
    rnd = torch.rand((500, 4), generator=g) * 900
    rnd[:, 2:] = rnd[:, :2] + torch.rand((500, 2), generator=g) ** 3 * 1200
    for lo, hi in ((2, 5), (1, 6)):
        for boxes in (b, rnd):
            assert torch.equal(R.levels_ref(boxes, lo, hi), O.assign_boxes_to_levels(boxes.double(), lo, hi))
        assert torch.equal(R.levels_ref(b, lo, hi), O.assign_boxes_to_levels(b, lo, hi))
    lv = R.levels_ref(b, 1, 6) + 1
    assert lv[0:42:7].tolist() == lv[1:42:7].tolist() == lv[2:42:7].tolist() == [1, 2, 3, 4, 5, 6]     # on the boundary: upper side
    assert lv[3:42:7].tolist() == lv[5:42:7].tolist() == [1, 2, 3, 4, 5, 6]
    assert lv[4:42:7].tolist() == lv[6:42:7].tolist() == [1, 1, 2, 3, 4, 5]                             # just below
    assert lv[42:].tolist() == [1, 1]


def test_apply_deltas_ref_vs_the_oracle():
    """apply_deltas_ref against oracle.apply_deltas + clip_boxes (fp32 only): bit for bit on exact inputs (zero deltas, whole
    translations, boxes beyond the image), within fp32 error on random ones, and NaN where the oracle has NaN."""
    from oracle import ops as O

    g = torch.Generator().manual_seed(6)
    src = torch.randint(-40, 400, (60, 2), generator=g).float() / 2
    src = torch.cat([src, src + torch.randint(1, 200, (60, 2), generator=g).float() / 2], dim=1)
    for wt in R.CASCADE_WEIGHTS:
        km = torch.randint(-3, 4, (60, 2), generator=g).float()
        d = torch.cat([km * torch.tensor(wt[:2]), torch.zeros((60, 2))], dim=1)
        raw, clipped = R.apply_deltas_ref(src, d, wt, R.SCALE_CLAMP, torch.tensor(R.DELTA_SIZES[:1]))
        o_raw = O.apply_deltas(d, src, wt)
        assert torch.equal(raw, o_raw.double()) and torch.equal(clipped, O.clip_boxes(o_raw, R.DELTA_SIZES[0]).double())
        w_, h_ = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
        assert torch.equal(raw.float(), src + torch.stack([km[:, 0] * w_, km[:, 1] * h_] * 2, dim=1))
        s2, d2, img = R.delta_random_case(400, 7, wt)
        raw, clipped = R.apply_deltas_ref(s2, d2, wt, R.SCALE_CLAMP, torch.tensor(R.DELTA_SIZES), img)
        o_raw = O.apply_deltas(d2, s2, wt)
        assert float(((o_raw.double() - raw).abs() / raw.abs().clamp(min=1)).max()) < 1e-5
        assert float(raw.abs().max()) > 3000 and float((d2[:, 2:] / torch.tensor(wt[2:])).min()) < -19
        for i in range(3):
            sel = img == i
            assert float((O.clip_boxes(o_raw[sel], R.DELTA_SIZES[i]).double() - clipped[sel]).abs().max()) < 1e-3
            assert float(clipped[sel].min()) == 0.0 and float(clipped[sel][:, 0::2].max()) == R.DELTA_SIZES[i][1]
        for c in range(4):
            d3 = d2[:8].clone()
            d3[c, c] = float("nan")
            raw, clipped = R.apply_deltas_ref(s2[:8], d3, wt, R.SCALE_CLAMP, torch.tensor(R.DELTA_SIZES[:1]))
            o_raw = O.apply_deltas(d3, s2[:8], wt)
            assert torch.equal(torch.isnan(raw), torch.isnan(o_raw)) and int(torch.isnan(raw).any(dim=1).sum()) == 1
            assert bool(torch.isnan(raw[c, c % 2::2]).all())


@pytest.mark.parametrize("p", [1, 7, 28])
def test_mask_crop_ref_equals_the_oracle_on_exact_inputs(p):
    """mask_crop_ref >= 0.5 == oracle.crop_and_resize_masks (the C ROIAlign in fp32) on the exact-input case, where fp32 has no
    rounding; the fp32 averages themselves agree to the last bit of the one division; the case's claims hold: bin sums are fp32
    numbers, averages exactly 1/4, 2/4, 3/4, 4/9 and 5/9 occur, outside and empty ROIs give 0."""
    from oracle import ops as O

    masks, rois = R.mask_crop_exact_case(p)
    avg = R.mask_crop_ref(masks, rois, p)
    assert avg.shape == (rois.shape[0], p, p)
    want = O.roi_align(masks[:, None].float(), rois, p, 1.0)[:, 0]
    assert torch.equal(avg.float(), want)
    for r in range(rois.shape[0]):     # the C routine takes one mask per ROI row in crop_and_resize_masks: feed it that way
        got = O.crop_and_resize_masks(masks[int(rois[r, 0])][None].bool(), rois[r: r + 1, 1:], p)
        assert torch.equal(got[0], avg[r] >= 0.5), r
    sums = avg * 36           # every grid has 1, 4, 6 or 9 samples a bin... times 36: an integer multiple of 1/64 when exact
    assert torch.equal(sums * 64, torch.round(sums * 64))
    seen = set(avg.flatten().tolist())
    for v in (0.25, 0.5, 0.75, 4.0 / 9, 5.0 / 9):
        assert v in seen, (p, v)
    assert not bool(avg[-5:].any()) and bool(avg[-10:-5].any())
    assert 0.2 < float((avg >= 0.5).double().mean()) < 0.8


def test_mask_crop_batch_case_layout():
    masks, rois, img = R.mask_crop_batch_case()
    assert len(masks) == 35 and len({tuple(m.shape) for m in masks}) == 2
    assert sorted(set(img.tolist())) == [0, 5, 31, 32, 34] and img.tolist() == sorted(img.tolist()) and rois.shape[0] == img.numel()


def test_mask_crop_random_case_margin_on_the_cpu():
    """The random-input crop: the share of pixels whose float64 average lies within 4 x max |fp32 form - float64| of 0.5 is below
    0.1 %, and the reference's own fp32 form decides like float64 everywhere else."""
    from oracle import ops as O

    masks, rois = R.mask_crop_random_case()
    avg = R.mask_crop_ref(masks, rois, 28)
    v32 = O.roi_align(masks[:, None].float(), rois, 28, 1.0)[:, 0].double()
    margin = 4 * float((v32 - avg).abs().max())
    assert 0 < margin < 1e-4      # a few ulps of a coordinate near 50 (3.8e-6 each) times a slope of at most 1 per pixel
    near = (avg - 0.5).abs() < margin
    assert float(near.double().mean()) <= 1e-3
    assert torch.equal((v32 >= 0.5)[~near], (avg >= 0.5)[~near])
    assert 0.2 < float((avg >= 0.5).double().mean()) < 0.8


def test_kmeans_update_ref_equals_the_oracle_and_a_hand_worked_case():
    """kmeans_update_ref: four points worked by hand (an out-of-range label on either side, an empty cluster); sums / counts ==
    oracle.ops.kmeans_update's centroids (scatter_add_ + bincount in float64) on in-range labels; sum_abs against a loop."""
    from oracle import ops as O

    x = torch.tensor([[1.0, -2.0], [3.0, 4.0], [-5.0, 6.0], [7.0, 8.0], [100.0, 100.0], [-100.0, 100.0]])
    lab = torch.tensor([2, 0, 2, 0, -1, 3])
    s, n, a = R.kmeans_update_ref(x, lab, 3)
    assert s.dtype == F64 and n.dtype == torch.int64 and a.dtype == F64
    assert s.tolist() == [[10.0, 12.0], [0.0, 0.0], [-4.0, 4.0]] and n.tolist() == [2, 0, 2]
    assert a.tolist() == [[10.0, 12.0], [0.0, 0.0], [6.0, 8.0]]
    g = torch.Generator().manual_seed(3)
    x = torch.randn((500, 7), generator=g)
    x[::5] *= 1e3
    for pattern in ("uniform", "rr", "holes", "runs"):
        lab = R.kmeans_labels(pattern, 500, 23, g)
        assert int(lab.min()) >= 0 and int(lab.max()) < 23
        s, n, a = R.kmeans_update_ref(x, lab, 23)
        want_c, want_n = O.kmeans_update(x.double(), lab, 23)
        assert torch.equal(n.double(), want_n)
        full = n > 0
        assert float(((s / n[:, None])[full] - want_c[full]).abs().max()) <= 1e-12 * float(want_c[full].abs().max())
        assert bool(torch.isnan(want_c[~full]).all()) and not bool(s[~full].any())
        for j in range(23):
            assert float((a[j] - x[lab == j].double().abs().sum(0)).abs().max()) <= 1e-12 * (1 + float(a[j].max()))
        if pattern == "holes":
            assert n[0] == 0 and n[22] == 0 and not bool(n[7:11].any()) and bool((n[1:7] > 0).all())
    # a cluster of -0.0 rows sums to +0; a NaN row poisons its own cluster only
    x = torch.tensor([[-0.0, 1.0], [float("nan"), 2.0], [3.0, float("inf")]])
    s, n, a = R.kmeans_update_ref(x, torch.tensor([0, 1, 2]), 3)
    assert not bool(torch.signbit(s[0, 0])) and bool(torch.isnan(s[1, 0])) and float(s[2, 1]) == float("inf")
    assert int(torch.isnan(s).sum()) == 1 and int(torch.isinf(s).sum()) == 1


def test_kmeans_label_runs_end_where_the_kernel_counts():
    lab = R.kmeans_labels("runs", 2000, 300, None)
    ends = (torch.nonzero(lab[1:] != lab[:-1])[:, 0] + 1).tolist()
    assert ends == R.KM_RUN_ENDS and all(e in ends for e in (7, 8, 9, 255, 256, 257, 511, 512, 513))
    assert int(R.kmeans_labels("runs", 2000, 5, None).max()) == 4
    assert R.kmeans_labels("rr", 10, 3, None).tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]


def test_gamma32_is_highams_constant():
    g = R.gamma32(torch.tensor([0, 1, 1000, 1 << 17]))
    assert g[0] == 0 and g[1] == 2.0 ** -24 / (1 - 2.0 ** -24) and abs(float(g[3]) - 2.0 ** -7 / (1 - 2.0 ** -7)) < 1e-18
    # fp32 summation in two different orders stays inside the bound (the bound is what the GPU tests use, not these sums)
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1)) * 100
    exact, abs_sum = float(x.double().sum()), float(x.double().abs().sum())
    seq = torch.zeros((), dtype=torch.float32)
    for v in x:
        seq = seq + v
    for got in (float(seq), float(x.sum())):
        assert abs(got - exact) <= float(R.gamma32(999)) * abs_sum


def test_kmeans_argmin_ref_equals_the_oracle_and_torch_argmin_on_nan():
    """kmeans_argmin_ref == oracle.ops.kmeans_assign in float64 on finite centroids, whatever the chunking; with NaN rows it is
    torch.argmin of the distance matrix (the NaN wins, the first NaN among several); the gap is the relative distance between the
    two nearest FINITE centroids; a duplicated centroid is a zero gap decided for the lower index."""
    from oracle import ops as O

    g = torch.Generator().manual_seed(9)
    cen = torch.randn((12, 16), generator=g) * 2
    x = cen[torch.randint(0, 12, (300,), generator=g)] + 0.5 * torch.randn((300, 16), generator=g)
    c = cen + 0.3 * torch.randn((12, 16), generator=g)
    lab, gap = R.kmeans_argmin_ref(x, c)
    assert torch.equal(lab, O.kmeans_assign(x.double(), c.double()))
    lab2, gap2 = R.kmeans_argmin_ref(x, c, budget=16 * 12 * 7)      # chunks of 7 rows
    assert torch.equal(lab, lab2) and torch.equal(gap, gap2)
    d = ((x.double()[:, None] - c.double()[None]) ** 2).sum(-1)
    two = d.sort(dim=1).values[:, :2]
    assert torch.equal(gap, (two[:, 1] - two[:, 0]) / two[:, 0]) and float(gap.min()) > 1e-3
    for rows, want in (((5,), 5), ((7, 3), 3), ((0, 11), 0)):
        cn = c.clone()
        for r in rows:
            cn[r, 2] = float("nan")
        labn, gapn = R.kmeans_argmin_ref(x, cn)
        dn = ((x.double()[:, None] - cn.double()[None]) ** 2).sum(-1)
        assert torch.equal(labn, torch.argmin(dn, dim=1)) and bool((labn == want).all())
        keep = [j for j in range(12) if j not in rows]
        assert torch.equal(gapn, R.kmeans_argmin_ref(x, c[keep])[1])
    cd = c.clone()
    cd[9] = cd[4]
    labd, gapd = R.kmeans_argmin_ref(x, cd)
    assert not bool((labd == 9).any()) and bool((gapd[lab == 4] == 0).all()) and bool((labd[lab == 4] == 4).all())
    cf = c.clone()
    cf[6] = 1e20
    labf, _ = R.kmeans_argmin_ref(x, cf)
    assert not bool((labf == 6).any()) and torch.equal(labf[lab != 6], lab[lab != 6])
    assert R.kmeans_argmin_ref(x[:3], c[:1])[1].tolist() == [float("inf")] * 3


def test_knn_ref_equals_the_oracle_in_float64_and_a_hand_worked_case():
    """knn_ref == oracle.ops.knn on float64 inputs (the oracle stores its distances in fp32: compared after that rounding), for any
    chunking; a hand-worked case with a tie and a duplicate; a train row with NaN / Inf is ranked behind every finite one."""
    from oracle import ops as O

    g = torch.Generator().manual_seed(4)
    xt, xq = torch.randn((157, 24), generator=g), torch.randn((61, 24), generator=g)
    xt[90] = xt[12]                                              # a duplicate: equal distances from every query
    d, ind, dist = R.knn_ref(xt, xq, 9)
    assert d.dtype == F64 and ind.dtype == torch.int64 and dist.shape == (61, 157) and d.shape == ind.shape == (61, 9)
    want_ind, want_d = O.knn(xt.double(), xq.double(), 9)
    assert torch.equal(ind, want_ind) and torch.equal(d.float(), want_d)
    assert torch.equal(torch.gather(dist, 1, ind), d) and bool((d[:, 1:] >= d[:, :-1]).all())
    for budget in (1, 157 * 24 * 7, 1 << 30):                    # one row, seven rows, everything at a time
        d2, ind2, dist2 = R.knn_ref(xt, xq, 9, budget=budget)
        assert torch.equal(d, d2) and torch.equal(ind, ind2) and torch.equal(dist, dist2)
    # by hand: the query (0, 0); train rows 0 and 3 tie at distance 25, rows 1 and 4 are the same point at distance 1
    yt = torch.tensor([[3.0, 4.0], [1.0, 0.0], [0.0, 6.0], [-5.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    d, ind, dist = R.knn_ref(yt, torch.zeros((1, 2)), 5)
    assert dist.tolist() == [[25.0, 1.0, 36.0, 25.0, 1.0, 4.0]]
    assert ind.tolist() == [[1, 4, 5, 0, 3]] and d.tolist() == [[1.0, 1.0, 4.0, 25.0, 25.0]]
    yt[1, 0], yt[5, 1] = float("nan"), float("inf")
    d, ind, _ = R.knn_ref(yt, torch.zeros((1, 2)), 6)
    assert ind.tolist() == [[4, 0, 3, 2, 5, 1]] and d[0, :4].tolist() == [1.0, 25.0, 25.0, 36.0]
    assert float(d[0, 4]) == float("inf") and bool(torch.isnan(d[0, 5]))


def test_knn_decidable_on_three_points_and_the_key_bound():
    """knn_decidable by hand: train points 0, 3, 3.01 on a line and the query 0 - distances 0, 9, 9.0601.  With E = 0.1 the third
    lies within 2 E of the second: k = 2 is decidable with one spare candidate and not with none; k = 1 (nothing within 0.2 of 0)
    and k = 3 (there is no fourth) are decidable without any; with E = 0.01 so is k = 2.  knn_key_bound: its formula on a case
    small enough to evaluate by hand, and - a plausibility check, not where the bound comes from - the expanded-form key in fp32
    on the CPU stays inside it."""
    yt = torch.tensor([[0.0], [3.0], [3.01]], dtype=F64)
    dist = R.knn_ref(yt, torch.zeros((1, 1), dtype=F64), 1)[2]
    assert (dist - torch.tensor([[0.0, 9.0, 9.0601]], dtype=F64)).abs().max() < 1e-12
    e = torch.tensor([0.1], dtype=F64)
    assert R.knn_decidable(dist, 2, e, spare=1).tolist() == [True] and R.knn_decidable(dist, 2, e, spare=0).tolist() == [False]
    assert R.knn_decidable(dist, 1, e, spare=0).tolist() == [True] and R.knn_decidable(dist, 3, e, spare=0).tolist() == [True]
    assert R.knn_decidable(dist, 2, e / 10, spare=0).tolist() == [True]
    assert R.knn_decidable(dist, 2, e).tolist() == [True] and R.KN_SPARE == 4
    # two train rows (2, 0) and (-2, 0): mean 0, mean|y| = (2, 0); the query (1, 1): a = (1, 1) + delta, b = (2, 0) + delta
    yt, xq = torch.tensor([[2.0, 0.0], [-2.0, 0.0]]), torch.tensor([[1.0, 1.0]])
    dl = float(R.gamma32(2)) * 2.0
    want = float(R.gamma32(5)) * ((2 + dl) ** 2 + 2 * (1 + dl) * (2 + dl))
    assert abs(float(R.knn_key_bound(yt, xq)[0]) - want) <= 1e-15 * want
    # a third train row (NaN, 0): its finite elements count for the mean of now three rows - still (0, 0), sum|y| / 3 = (4/3, 0) -,
    # the row itself is not in the maximum
    bad = torch.cat([yt, torch.tensor([[float("nan"), 0.0]])])
    dl = float(R.gamma32(3)) * 4.0 / 3.0
    want = float(R.gamma32(5)) * ((2 + dl) ** 2 + 2 * (1 + dl) * (2 + dl))
    assert abs(float(R.knn_key_bound(bad, xq)[0]) - want) <= 1e-15 * want
    g = torch.Generator().manual_seed(8)
    for d, off in ((16, 0.0), (48, 0.0), (32, 100.0), (768, 0.0)):
        yt, xq = torch.randn((300, d), generator=g) + off, torch.randn((40, d), generator=g) + off
        m32 = yt.mean(0)
        y1, x1 = yt - m32, xq - m32
        key32 = (y1 * y1).sum(1)[None, :] - 2 * (x1 @ y1.T)
        y2, x2 = yt.double() - m32.double(), xq.double() - m32.double()
        key64 = (y2 * y2).sum(1)[None, :] - 2 * (x2 @ y2.T)
        e = R.knn_key_bound(yt, xq)
        assert bool(((key32.double() - key64).abs() <= e[:, None]).all())
        assert float(e.max()) < 1e-2 * float(R.knn_dists(yt, xq).min())


def test_lattice_rows_are_what_the_exact_cases_need():
    g = torch.Generator().manual_seed(2)
    for n in (1, 2, 31, 320, 641):
        y = R.lattice_rows(n, 16, g)
        assert y.shape == (n, 16) and y.dtype == torch.float32
        R.assert_lattice(y, R.lattice_rows(5, 16, g))
        assert torch.equal(y[0:n - 1:2], -y[1:n:2]) and (n % 2 == 0 or not bool(y[-1].any()))
    with pytest.raises(AssertionError):
        R.assert_lattice(torch.ones((2, 16)), torch.ones((1, 16)))
    with pytest.raises(AssertionError):
        R.assert_lattice(R.lattice_rows(4, 16, g), torch.full((1, 16), 0.5))


def test_usl_reg_ref_equals_the_oracle_and_names_the_other_outcome_at_the_edge():
    """usl_reg_ref's value is regularizer64's (momentum 0.5: 1 - momentum is the same number in both); its bound holds for the same
    update computed in fp32 on the CPU (a plausibility check, not where the bound comes from); and by hand: selected rows at 1, 2,
    2.000001 and 10 on a line, the data row at 0 with the label of the row at 2, H = 2 with the same-cluster mask - the second and
    third distances (4 and 4.000004) are closer than 2 gamma_18 * 4, so fp32 may put either second: the reference masks the second
    (1 + 1e-10), the other outcome keeps the third unmasked (1 + 1 / 4.000004); with the label on the nearest row nothing is open."""
    from tests.usl_select_oracle import regularizer64

    g = torch.Generator().manual_seed(6)
    x, y = torch.randn((90, 32), generator=g), torch.randn((40, 32), generator=g)
    x[3] = y[5]
    labels = torch.randint(0, 43, (90,), generator=g)
    labels[3] = 5
    reg = torch.rand(90, generator=g)
    for alpha in (1, 0.5, 2):
        for exclude in (False, True):
            ref = R.usl_reg_ref(x, y, labels, reg, 7, alpha, 0.5, 0.5, exclude)
            assert torch.equal(ref[0], regularizer64(x, y, labels, reg, 7, alpha, 0.5, exclude)) and bool(ref[2].all()) and not bool(ref[3][2].any())
            d32 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
            v, j = torch.sort(d32, dim=1, stable=True)
            v, j = v[:, :7].clone(), j[:, :7]
            if exclude:
                v[j == labels[:, None]] = 1e10
            else:
                v[v == 0] = 1e10
            p = v if alpha == 1 else (v.sqrt() if alpha == 0.5 else v * v)
            got = reg * 0.5 + (1 / p).sum(1) * 0.5
            assert bool(R.usl_reg_within(got, ref).all())
            assert float((ref[1] / ref[0]).max()) < 1e-5
    sel = torch.zeros((4, 16))
    sel[:, 0] = torch.tensor([1.0, 2.0, 2.000001, 10.0])
    x0, zero = torch.zeros((1, 16)), torch.zeros(1)
    want, bound, checked, (want_alt, _, rows) = R.usl_reg_ref(x0, sel, torch.tensor([1]), zero, 2, 1, 0.0, 1.0, True)
    d3 = float(sel[2, 0].double() ** 2)
    assert rows.tolist() == [True] and checked.tolist() == [True] and 4 < d3 < 4 * (1 + 2 * float(R.gamma32(18)))
    assert abs(float(want[0]) - (1 + 1e-10)) < 1e-15 and abs(float(want_alt[0]) - (1 + 1 / d3)) < 1e-15
    assert R.usl_reg_within(torch.tensor([1.0]), (want, bound, checked, (want_alt, bound, rows))).tolist() == [True]
    assert R.usl_reg_within(torch.tensor([1.0 + 1 / 4.0]), (want, bound, checked, (want_alt, bound, rows))).tolist() == [True]
    assert R.usl_reg_within(torch.tensor([1.1]), (want, bound, checked, (want_alt, bound, rows))).tolist() == [False]
    ref = R.usl_reg_ref(x0, sel, torch.tensor([0]), zero, 2, 1, 0.0, 1.0, True)
    assert not bool(ref[3][2].any()) and bool(ref[2].all()) and abs(float(ref[0][0]) - (1e-10 + 0.25)) < 1e-15
    # three rows inside the window: not a plain swap any more, the row is unchecked
    sel[3, 0] = 2.000002
    ref = R.usl_reg_ref(x0, sel, torch.tensor([1]), zero, 2, 1, 0.0, 1.0, True)
    assert ref[2].tolist() == [False] and ref[3][2].tolist() == [False]


# ----------------------------------------------------------------------------------------------------------------------------
# the E step's decision rule and gap ladder (tests/test_gpu_kmeans_assign_float64.py)
# ----------------------------------------------------------------------------------------------------------------------------
def test_kmeans_key_bound_equals_a_brute_force_loop():
    """E_i = gamma_(D+3) max_j (|c_j|^2 + 2 |x_i|.|c_j|) by explicit loops on a tiny case with signs, a NaN centroid row (left out of
    the maximum) and a NaN point (E_i NaN)."""
    g = torch.Generator().manual_seed(3)
    x, c = torch.randn((4, 5), generator=g), torch.randn((3, 5), generator=g) * 3
    c[1, 2] = float("nan")
    x[3, 0] = float("nan")
    e = R.kmeans_key_bound(x, c)
    gam = (5 + 3) * 2.0 ** -24 / (1 - (5 + 3) * 2.0 ** -24)
    for i in range(3):
        best = 0.0
        for j in (0, 2):
            cc = sum(float(c[j, t]) ** 2 for t in range(5))
            xc = sum(abs(float(x[i, t])) * abs(float(c[j, t])) for t in range(5))
            best = max(best, cc + 2 * xc)
        assert abs(float(e[i]) - gam * best) <= 1e-15 * gam * best
    assert bool(torch.isnan(e[3])) and e.dtype == F64


def test_kmeans_decision_rule_on_a_hand_worked_case():
    """Centroids 0, 2, 2 (a duplicate of the second) and 10 on a line, D = 1, E_i = gamma_4 max (c^2 + 2 |x| c).  x = 0.5: gap
    2.25 - 0.25, decidable, only label 0 passes.  x = 1 - 2^-22: distances differ by 2^-20, far below 2 E (E ~ 2.9e-5): labels 0, 1
    and 2 pass (the band's rows are not all the same: any of them may win), 3 does not.  x = 3: the band holds the two duplicates
    alone - label 1 passes, label 2 does not.  A NaN point: label 0 only.  A label outside [0, K) never passes."""
    c = torch.tensor([[0.0], [2.0], [2.0], [10.0]])
    x = torch.tensor([[0.5], [1 - 2.0 ** -22], [3.0], [float("nan")]])
    ref = R.kmeans_decision_ref(x, c)
    gam = float(R.gamma32(4))
    assert torch.allclose(ref["e"][:3], gam * torch.tensor([110.0, 100 + 20 * (1 - 2.0 ** -22), 160.0], dtype=F64), rtol=1e-14, atol=0)
    assert ref["ref"].tolist() == [0, 0, 1, 0] and ref["decidable"].tolist() == [True, False, False, False]
    assert float(ref["gap"][0]) == 2.0 and float(ref["gap"][2]) == 0.0
    assert abs(float(ref["gap"][1]) - 2.0 ** -20) < 1e-15 and ref["nan"].tolist() == [False, False, False, True]
    assert ref["low"].tolist()[:3] == [0, 0, 1] and ref["same"].tolist()[:3] == [True, False, True]
    assert abs(float(ref["rel"][0]) - 2.0 / (0.5 * 10.0)) < 1e-15
    assert R.kmeans_band(ref).tolist() == [4, 0, 0, 0]
    for labels, want in (([0, 0, 1, 0], [True] * 4), ([1, 1, 2, 1], [False, True, False, False]), ([2, 2, 3, 2], [False, True, False, False]),
                         ([3, 3, 0, 3], [False] * 4), ([0, -1, 4, 0], [True, False, False, True])):
        assert R.kmeans_rule_ok(x, c, torch.tensor(labels), ref).tolist() == want, labels
    assert R.kmeans_rule_report("p", x, c, torch.tensor([0, 0, 1, 0]), ref) is None
    msg = R.kmeans_rule_report("the path", x, c, torch.tensor([1, 3, 1, 5]), ref)
    assert msg.startswith("the path: 1 decidable labels differ") and "1 undecidable" in msg and "1 NaN rows" in msg and "row 0 got 1" in msg
    assert "gap 2.000000e+00" in msg and "band 4" in msg
    # K = 1: every point decidable, whatever the distance
    one = R.kmeans_decision_ref(x[:3], c[:1])
    assert one["decidable"].tolist() == [True] * 3 and one["ref"].tolist() == [0] * 3


def test_kmeans_ladder_pairs_cover_the_meeting_places():
    assert R.kmeans_ladder_pairs(1) == [] and R.kmeans_ladder_pairs(2) == [(0, 1, 2)]
    assert R.kmeans_ladder_pairs(17) == [(0, 1, 2), (15, 16, 5)]
    assert R.kmeans_ladder_pairs(40) == [(0, 1, 2), (15, 16, 5), (3, 19, 8), (31, 32, 11), (38, 39, 2)]
    assert R.kmeans_ladder_pairs(321)[-1] == (319, 320, 2) and len(R.kmeans_ladder_pairs(321)) == 5
    assert R.kmeans_ladder_pairs(641)[4:] == [(639, 640, 2), (319, 320, 5), (5, 325, 2), (640, 7, 5)]      # 640 is made once: 7 from it
    assert R.kmeans_ladder_pairs(1280)[4:] == [(1278, 1279, 2), (319, 320, 5), (5, 325, 2)]
    for k in (2, 17, 40, 300, 320, 321, 641, 1280):
        made = [b for _, b, _ in R.kmeans_ladder_pairs(k)]
        assert len(set(made)) == len(made) and {m for _, _, m in R.kmeans_ladder_pairs(k)} <= {2, 5, 8, 11}


@pytest.mark.parametrize("k,d,n,off", R.KM_ALL_CASES, ids=["K%d-D%d-N%d-off%d" % e for e in R.KM_ALL_CASES])
def test_kmeans_gap_ladder_offers_what_the_gpu_cases_assume(k, d, n, off):
    """Every case of the GPU module, on the CPU: inputs are fp32 and finite; a full-size case meets the band counts and the
    undecidable share (kmeans_check_ladder) with ladder rows at both ends of the scale; decidable ladder rows of the two narrowest
    bands sit at the work-group edges; every centroid pair is some point's two nearest; and a plain fp32 program - |c|^2 - 2 x c^T
    and torch.argmin - obeys the decision rule at every point while differing from float64 at some undecidable ones: the rule
    is neither vacuous nor stricter than fp32 arithmetic allows."""
    x, c, ref, is_lad = R.kmeans_gap_ladder(k, d, n, off)
    assert x.dtype == c.dtype == torch.float32 and x.shape == (n, d) and c.shape == (k, d)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(c).all()) and not bool(ref["nan"].any())
    again = R.kmeans_decision_ref(x, c, budget=k * d * 37)           # the reference went through the placement's permutation with its rows
    assert all(torch.equal(ref[name], again[name]) for name in ("ref", "low", "same", "decidable")) and torch.allclose(ref["gap"], again["gap"])
    band = R.kmeans_band(ref)
    if n >= 2048 and k >= 2:
        counts, share = R.kmeans_check_ladder(ref, n, d)
        assert share >= 0.002                                         # and there ARE undecidable points
        edges = [e % n for e in R.KM_EDGE_ROWS]
        present = [b for b in (1, 2, 3, 4) if bool(((band == b) & is_lad).any())][:2]
        assert bool(is_lad[edges].all()) and set(band[edges].tolist()) == set(present) and present[0] == (2 if d >= 768 else 1)
        top2 = torch.topk(R.knn_dists(c, x), 2, dim=1, largest=False).indices.sort(dim=1).values
        for a, b, _ in R.kmeans_ladder_pairs(k):
            assert bool(((top2[:, 0] == min(a, b)) & (top2[:, 1] == max(a, b)) & is_lad).any()), (a, b)
    lab = R.kmeans_fp32_plain(x, c)
    msg = R.kmeans_rule_report("plain fp32", x, c, lab, ref)
    assert msg is None, msg
    differs = lab != ref["ref"]
    assert not bool((differs & ref["decidable"]).any())
    if n >= 2048 and k >= 2:
        assert bool(differs.any())


def test_kmeans_rule_on_scaled_inputs_and_nan_rows():
    """The variants the GPU module derives from the (40, 64) ladder: inputs times 2^-40 and 2^40 (every quantity of the rule scales
    exactly: same arg-min, same decidable set) and three NaN rows (label 0 there, every other row's reference untouched); the plain
    fp32 program obeys the rule on each."""
    x, c, ref, _ = R.kmeans_gap_ladder(40, 64, R.KM_N_STD, 0.0)
    for power in (-40, 40):
        xs, cs = x * 2.0 ** power, c * 2.0 ** power
        rs = R.kmeans_decision_ref(xs, cs)
        assert torch.equal(rs["ref"], ref["ref"]) and torch.equal(rs["decidable"], ref["decidable"])
        for name in ("gap", "e"):                                     # (to rounding: a float64 matrix product need not repeat its order)
            assert torch.allclose(rs[name], ref[name] * 4.0 ** power, rtol=1e-12, atol=0)
        assert R.kmeans_rule_report("plain fp32", xs, cs, R.kmeans_fp32_plain(xs, cs), rs) is None
    xn = x.clone()
    xn[0, 3], xn[300], xn[-1, -1] = float("nan"), float("nan"), float("nan")
    rn = R.kmeans_decision_ref(xn, c)
    keep = ~rn["nan"]
    assert rn["nan"].nonzero()[:, 0].tolist() == [0, 300, R.KM_N_STD - 1] and not bool(rn["decidable"][~keep].any())
    assert all(torch.equal(rn[name][keep], ref[name][keep]) for name in ("ref", "decidable", "low", "same"))
    assert all(torch.allclose(rn[name][keep], ref[name][keep], rtol=1e-12, atol=0) for name in ("gap", "e"))
    lab = R.kmeans_fp32_plain(xn, c)
    assert lab[~keep].tolist() == [0, 0, 0] and R.kmeans_rule_report("plain fp32", xn, c, lab, rn) is None
    lab[300] = 1
    assert "1 NaN rows are not 0" in R.kmeans_rule_report("plain fp32", xn, c, lab, rn)


# ---- conv_stream.hip launch geometry (tests/test_gpu_tail_bwd_fused.py, tests/test_gpu_conv_float64.py) ----
@pytest.mark.parametrize("c,n,m,tiny,tm,tiles_n,nwalk,tiles_m,xcnt,counts", [
    # the 8-work-group grid: one walker per XCD and channel block owns its XCD's whole range
    (64, 256, 7515, True, 128, 1, 1, 59, (8, 7), [7, 8]),
    (128, 512, 3739, True, 64, 2, 1, 59, (8, 7), [7, 8]),
    (256, 1024, 3739, True, 64, 4, 1, 59, (8, 7), [7, 8]),
    # the production grid: 256 work-groups per resident group, nwalk walkers per XCD and channel block
    (256, 1024, 26779, False, 64, 4, 8, 419, (53, 52), [6, 7]),
    (128, 512, 106651, False, 64, 2, 32, 1667, (209, 208), [6, 7]),
    (64, 256, 426331, False, 128, 1, 64, 3331, (417, 416), [6, 7]),
    (64, 256, 546, False, 128, 1, 64, 5, (1, 0), [1]),
    (128, 512, 546, False, 64, 2, 32, 9, (2, 1), [1]),
    (256, 1024, 546, False, 64, 4, 8, 9, (2, 1), [1]),
    (256, 1024, 5595, False, 64, 4, 8, 88, (11, 11), [1, 2]),
    (256, 1024, 33600, False, 64, 4, 8, 525, (66, 65), [8, 9]),
    # the shapes the tests had before: never past the ring's end
    (64, 256, 1024, True, 128, 1, 1, 8, (1, 1), [1]),
    (256, 1024, 1024, True, 64, 4, 1, 16, (2, 2), [2]),
])
def test_stream_geometry_of_the_tail_cases(c, n, m, tiny, tm, tiles_n, nwalk, tiles_m, xcnt, counts):
    """The restated launch geometry on hand-worked values (59 = 8 * 7 + 3 tiles: XCDs 0-2 own 8, the others 7, and so on), so
    that a slip in the helper cannot make the regime assertions of the GPU tests vacuous."""
    geo = R.stream_geometry(c, n, m, tiny, tail=True)
    assert geo["ring"] == 5 and geo["steps_per_tile"] == 1
    assert (geo["TM"], geo["tiles_n"], geo["nwalk"], geo["tiles_m"]) == (tm, tiles_n, nwalk, tiles_m)
    assert (geo["xcnt"][0], geo["xcnt"][7]) == xcnt and sum(geo["xcnt"]) == tiles_m
    assert R.walker_tiles(geo) == counts
    # every tile has exactly one owner: walker k of XCD x takes tiles xbase + k, xbase + k + nwalk, ...
    owned = sorted(geo["xbase"][x] + k + i * geo["nwalk"] for x in range(8) for k in range(geo["nwalk"])
                   for i in range(geo["my_tiles"][x][k]))
    assert owned == list(range(tiles_m))
    assert all(t == 0 for x in range(8) for k, t in enumerate(geo["my_tiles"][x]) if k >= geo["xcnt"][x])
    # the fill rule: at least 6 tiles per work-group of the production grid; it is not applied to the 8-work-group grid
    assert geo["served_unforced"] == (None if tiny else tiles_m * tiles_n >= 6 * 256 * (1 if c == 256 else 2))


def test_stream_geometry_hand_worked_walkers():
    """256 -> 1024 at 26 779 pixels: XCD 0 owns 53 tiles, its 8 walkers 7 7 7 7 7 6 6 6; XCD 7 owns 52: 7 7 7 7 6 6 6 6.
    5 595 pixels (88 tiles, 11 per XCD): walkers 0-2 two tiles, 3-7 one.  546 pixels under 64 -> 256: five tiles, one walker each on
    XCDs 0-4 and nothing anywhere else."""
    geo = R.stream_geometry(256, 1024, 26779, False, tail=True)
    assert geo["my_tiles"][0] == [7, 7, 7, 7, 7, 6, 6, 6] and geo["my_tiles"][7] == [7, 7, 7, 7, 6, 6, 6, 6]
    assert geo["xbase"][:4] == [0, 53, 106, 159] and geo["xbase"][7] == 159 + 4 * 52
    geo = R.stream_geometry(256, 1024, 5595, False, tail=True)
    assert all(row == [2, 2, 2, 1, 1, 1, 1, 1] for row in geo["my_tiles"])
    geo = R.stream_geometry(64, 256, 546, False, tail=True)
    assert [sum(row) for row in geo["my_tiles"]] == [1, 1, 1, 1, 1, 0, 0, 0] and all(row[1:] == [0] * 63 for row in geo["my_tiles"])


def test_tail_depth_follows_the_geometry():
    # NF rows + 4 + the busiest walker's tiles + waves + 8 nwalk atomics; the three values the earlier cases were checked with
    assert R.tail_depth(64, 256, 546, True) == 8 + 4 + 1 + 4 + 8
    assert R.tail_depth(256, 1024, 1024, True) == 2 + 4 + 2 + 8 + 8
    assert R.tail_depth(128, 512, 40, True) == 4 + 4 + 1 + 4 + 8
    assert R.tail_depth(64, 256, 426331, False) == 8 + 4 + 7 + 4 + 512
    assert R.tail_depth(256, 1024, 33600, False) == 2 + 4 + 9 + 8 + 64
    # the plain kernel's statistics: 32 -> 40 has 4 waves along the pixels (NF = 2), 64 walkers; 256 -> 520: NF = 2, 8 waves, 10 walkers
    assert R.stream_stats_depth(R.stream_geometry(32, 40, 589825, False)) == 2 + 4 + 10 + 4 + 512
    assert R.stream_stats_depth(R.stream_geometry(256, 520, 30721, False)) == 2 + 4 + 7 + 8 + 80


@pytest.mark.parametrize("cin,cout,cfg,ring,nwalk,steps", [
    (32, 520, (128, 1, 4, 1), 8, 21, 1), (32, 40, (128, 4, 4, 1), 8, 64, 1), (64, 520, (128, 1, 4, 2), 5, 21, 1),
    (64, 104, (128, 2, 4, 2), 5, 64, 1), (128, 40, (64, 4, 4, 4), 5, 64, 1), (256, 520, (64, 2, 8, 8), 5, 10, 1),
    (256, 104, (64, 2, 4, 4), 5, 64, 2), (256, 40, (64, 4, 4, 4), 5, 64, 2)])
def test_stream_geometry_of_the_plain_kernel(cin, cout, cfg, ring, nwalk, steps):
    """The twelve instantiations' tile, ring and walker counts as conv_stream.hip's launcher states them (a 256-channel tile of
    the narrow layers arrives in two 128-channel ring steps), and STREAM_RING_PIXELS restated."""
    assert R.stream_cfg(cin, cout) == cfg
    geo = R.stream_geometry(cin, cout, 1000, False)
    assert (geo["ring"], geo["nwalk"], geo["steps_per_tile"]) == (ring, nwalk, steps)
    if steps == 1:
        assert geo["ring"] * geo["TM"] == R.STREAM_RING_PIXELS[cin]


def test_stream_production_geoms_are_in_steady_state():
    assert len(R.STREAM_PROD_GEOMS) == 8 and not set(R.STREAM_PROD_GEOMS) & set(R.ALL_CONV_GEOMS)
    for geom in R.STREAM_PROD_GEOMS:
        m, cin, cout = geom[2], geom[3], geom[4]
        geo = R.stream_geometry(cin, cout, m, False)
        counts = R.walker_tiles(geo)
        assert counts[-1] == geo["ring"] + 2 and geo["ring"] + 1 in counts, (geom, counts)
        assert len(set(geo["xcnt"])) == 2 and m % geo["TM"] == 1
        assert (geo["tiles_n"] > 1) == (cout == 520)
        # the smallest such count: one tile fewer leaves no walker with ring + 2 tiles
        assert max(R.walker_tiles(R.stream_geometry(cin, cout, m - 1, False))) == geo["ring"] + 1


def _topk_rows(kind, rows, n, bf16, seed):
    """Rows for the checks of topk_rows_ref: random, heavily tied, or full of NaNs of both signs, infinities and zeros of both
    signs."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((rows, n), generator=g)
    if kind == "tied":
        v = v.mul(2).round().div(2)
    if kind == "special":
        v = v.round()
        pick = torch.randint(0, 12, (rows, n), generator=g)
        bits = v.view(torch.int32)
        for j, b in enumerate((0x7FC00000, -0x400000, 0x7F800001, -0x7FFFFF, 0x7F800000, -0x800000, -0x80000000)):
            bits[pick == j] = b         # NaNs (+quiet, -quiet, +signalling, -signalling), +inf, -inf, -0.0
    return v.bfloat16() if bf16 else v


def _canonical(v):
    """fp32 values as the selection returns them: +0.0 for -0.0, the quiet NaN for every NaN; as bit patterns."""
    v = torch.where(torch.isnan(v), torch.full_like(v, float("nan")), v + 0.0)
    return v.contiguous().view(torch.int32)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", ["random", "tied", "special"])
def test_topk_rows_ref_equals_a_stable_sort(kind, bf16):
    """topk_rows_ref against torch.sort(stable=True), which ranks every NaN greatest and -0 equal to +0: the whole order
    (k = n), a prefix, k beyond the row; the returned values are the gathered ones in canonical form."""
    rows, n = 3, 1500
    v = _topk_rows(kind, rows, n, bf16, 3)
    if kind == "special":
        assert bool((v.float().view(torch.int32) == -0x80000000).any()) and int(torch.isnan(v.float()).sum()) > 100
    for largest in (True, False):
        sv, si = torch.sort(v.float(), dim=1, descending=largest, stable=True)
        for k in (n, 1, 37, n + 5):
            rv, ri, rc = R.topk_rows_ref(v, k, largest)
            m = min(k, n)
            assert rc.tolist() == [m] * rows and torch.equal(ri[:, :m].long(), si[:, :m])
            assert torch.equal(rv[:, :m].contiguous().view(torch.int32), _canonical(sv[:, :m]))
            assert bool((ri[:, m:] == 0).all()) and bool((rv[:, m:] == (float("-inf") if largest else float("inf"))).all())


@pytest.mark.parametrize("kind", ["tied", "special"])
def test_topk_rows_ref_equals_the_sorted_fallback(kind):
    """topk_rows_ref against layers.select._topk_rows_sorted on the CPU with the same specs: a mask that leaves rows with fewer
    participants than k and with none, the (group, pitch) view of a 32-wide map, k below and beyond the row; bit for bit."""
    from u2seg_amd.layers.select import _topk_rows_sorted

    g = torch.Generator().manual_seed(9)
    rows, n = 4, 2000
    for bf16 in (False, True):
        v = _topk_rows(kind, rows, n, bf16, 5)
        mask = torch.randint(0, 3, (rows, n), generator=g).to(torch.int8)
        mask[2] = 0
        mask[3, 20:] = 0
        m = _topk_rows(kind, 2, 700 * 32, True, 6).reshape(2, 700, 32)
        specs = [dict(vals=v, k=k, largest=largest, mask=mk, mask_value=2) for k in (1, 300, n, n + 7) for largest in (True, False)
                 for mk in (None, mask)]
        specs += [dict(vals=m, k=k, largest=largest, group=gr, pitch=32, n=700 * gr) for k in (50, 2100) for largest in (True, False)
                  for gr in (3, 5)]
        for sp in specs:
            fv, fi, fc = _topk_rows_sorted(sp)
            rv, ri, rc = R.topk_rows_ref(**sp)
            assert torch.equal(fc.int(), rc) and torch.equal(fi.int(), ri), (sp["k"], sp["largest"])
            assert torch.equal(fv.contiguous().view(torch.int32), rv.view(torch.int32)), (sp["k"], sp["largest"])


# ----------------------------------------------------------------------------------------------------------------------------
# head losses (tests/test_gpu_losses_float64.py): each reference against an independent formulation, float64 against float64
# ----------------------------------------------------------------------------------------------------------------------------
def _close12(got, ref, what):
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * max(scale, 1e-300), (
        what, float((got - ref).abs().max()), scale)


@pytest.mark.parametrize("case", [(5, 81, 88), (37, 11, 13), (9, 513, 520), (1, 2, 8)])
def test_softmax_ce_ref_equals_autograd_of_cross_entropy(case):
    from tests import loss_cases as C

    z, lab = C.softmax_case(*case)
    nc = case[1]
    ref = R.softmax_ce_ref(z, lab, nc)
    zz = z[:, :nc].to(F64).requires_grad_(True)
    ce = TF.cross_entropy(zz, lab, reduction="sum")
    ce.backward()
    _close12(ref["loss"], ce.detach(), "loss")
    _close12(ref["grad"], zz.grad, "grad")
    _close12(ref["rows"][:, 0], TF.cross_entropy(zz.detach(), lab, reduction="none"), "rows")
    assert float((ref["p"].sum(1) - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("case", [(3, 1, 1, 28, 32, 255, False), (1, 8, 1, 28, 32, 255, False), (3, 1, 16, 28, 32, 255, False),
                                  (3, 8, 16, 17, 64, 255, False), (1, 8, 16, 28, 32, 255, True), (1, 7, 15, 28, 32, 0, False),
                                  (3, 8, 16, 1, 8, 255, False)])
def test_semseg_ce_ref_equals_two_tap_index_arithmetic(case):
    """The loss, the count and the gradient from an explicit per-pixel two-tap interpolation (_source_index / _bilinear) and its
    transpose written as four scatter-adds."""
    from tests import loss_cases as C

    b, h, w, nc, lp, ignore, sat = case
    z, t = C.sem_case(*case)
    ref = R.semseg_ce_ref(z, t, nc, ignore)
    x = z[..., :nc].to(F64).permute(0, 3, 1, 2)
    ys, xs = R._source_index(4 * h, h, 0.25), R._source_index(4 * w, w, 0.25)
    up = R._bilinear(x, ys, xs)                                   # [b, nc, 4h, 4w]
    _close12(ref["up"].detach(), up, "up")
    tl = t.long()
    valid = tl != ignore
    lse = torch.logsumexp(up, 1)
    zt = up.gather(1, tl.clamp_max(nc - 1)[:, None])[:, 0]
    loss = torch.where(valid, lse - zt, torch.zeros_like(lse)).sum()
    assert ref["count"] == int(valid.sum()) and 0 < ref["count"] < valid.numel()
    _close12(ref["loss"], loss, "loss")
    gp = torch.exp(up - lse[:, None]) - TF.one_hot(tl.clamp_max(nc - 1), nc).permute(0, 3, 1, 2).to(F64)
    gp = gp * valid[:, None]
    (y0, y1, ly), (x0, x1, lx) = ys, xs
    gz = torch.zeros((b, nc, h, w), dtype=F64)
    for yi, wy in ((y0, 1 - ly), (y1, ly)):
        for xi, wx in ((x0, 1 - lx), (x1, lx)):
            flat = (yi[:, None] * w + xi[None, :]).reshape(-1)
            gz.view(b, nc, h * w).index_add_(2, flat, (gp * wy[:, None] * wx[None, :]).reshape(b, nc, -1))
    _close12(ref["grad"], gz.permute(0, 2, 3, 1), "grad")


@pytest.mark.parametrize("case", [(3, 7, False, 5), (2, 12, True, 80), (1, 2, False, 1)])
def test_mask_bce_ref_equals_bce_with_logits_of_conv2d(case):
    from tests import loss_cases as C

    n, side, _, k = case
    x, w, bias, cls, tgt = C.mask_case(*case)
    ref = R.mask_bce_ref(x, w, bias, cls, tgt)
    xd = x.to(F64).view(n, side, side, -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd = R.bf16_round(w).view(k, -1, 1, 1).requires_grad_(True)
    bd = R.bf16_round(bias).requires_grad_(True)
    conv = TF.conv2d(xd, wd, bd)                                                        # [n, k, side, side]
    sel = conv[torch.arange(n), cls].reshape(n, -1)
    _close12(ref["logit"], sel.detach(), "logit")
    loss = TF.binary_cross_entropy_with_logits(sel, tgt.to(F64), reduction="sum")
    loss.backward()
    _close12(ref["loss"], loss.detach(), "loss")
    _close12(ref["dx"], xd.grad.permute(0, 2, 3, 1).reshape(n, side * side, -1), "dx")
    _close12(ref["dW"], wd.grad.view(k, -1), "dW")
    _close12(ref["db"], bd.grad, "db")
    # the magnitude sums bound their sums; at a given z the loss moves with it
    assert bool((ref["logit_abs"] + R.bf16_round(bias)[cls].abs()[:, None] >= ref["logit"].abs()).all())
    assert bool((ref["dW_abs"] >= ref["dW"].abs() - 1e-15).all())
    z = R.rne_bf16(ref["logit"])
    at = R.mask_bce_ref(x, w, bias, cls, tgt, z)
    _close12(at["loss"], TF.binary_cross_entropy_with_logits(z, tgt.to(F64), reduction="sum"), "loss at z")
    # phases: the re-ordering is a permutation and its own inverse pair
    if side % 2 == 0:
        assert torch.equal(C.from_phases(C.to_phases(x, side), side), x)
        s = side // 2
        p = ((3 % s) * s + (1 % s)) * 4 + 2 + 1
        assert torch.equal(C.to_phases(x, side)[:, p], x[:, (2 * (3 % s) + 1) * side + 2 * (1 % s) + 1])


@pytest.mark.parametrize("case", [(3, 255, 2, 8, 16, False), (2, 257, 3, 16, 0, True), (1, 1, 1, 8, 16, False), (2, 64, 4, 8, 16, False)])
def test_rpn_level_ref_equals_the_oracle_statement(case):
    """The statement of test_rpn_loss (tests/test_gpu_parity.py), in float64: oracle.ops.get_deltas on the anchors and the
    matched boxes, L1 over the positives, BCE-with-logits over the labelled anchors, autograd."""
    from oracle import ops as O
    from tests import loss_cases as C

    c = C.rpn_case(*case)
    a, bsz = c["a"], case[0]
    o, d, lab, mt = C.rpn_views(c)
    ref = R.rpn_level_ref(o, d, lab, mt, c["gt"], c["anchors"], a)
    oc = o.to(F64).reshape(bsz, -1).requires_grad_(True)
    dc = d.to(F64).reshape(bsz, -1, 4).requires_grad_(True)
    lab = lab.long()
    pos, valid = lab == 1, lab >= 0
    tgt = torch.stack([O.get_deltas(c["anchors"].to(F64), c["gt"][b].to(F64)[mt[b].long()], (1.0, 1.0, 1.0, 1.0)) for b in range(bsz)])
    loc = (dc[pos] - tgt[pos]).abs().sum()
    cls = TF.binary_cross_entropy_with_logits(oc[valid], lab[valid].to(F64), reduction="sum")
    (cls + loc).backward()
    _close12(ref["loss_cls"], cls.detach(), "cls")
    _close12(ref["loss_loc"], loc.detach(), "loc")
    _close12(ref["dobj"].reshape(bsz, -1), oc.grad, "dobj")
    assert torch.equal(ref["ddlt"].reshape(bsz, -1, 4), dc.grad)
    assert int(pos.sum()) > 0 and int((~valid).sum()) > 0 or bsz == 1


@pytest.mark.parametrize("weights", R.CASCADE_WEIGHTS)
def test_box_l1_ref_equals_the_oracle_get_deltas(weights):
    from oracle import ops as O
    from tests import loss_cases as C

    pred, prop, gt, lab, _ = C.box_case(257, 32, False, weights)
    ref = R.box_l1_ref(pred, prop, gt, lab, C.BOX_BG, weights)
    fg = lab < C.BOX_BG
    pd = pred[:, :4].to(F64).requires_grad_(True)
    loss = (pd[fg] - O.get_deltas(prop.to(F64), gt.to(F64), weights)[fg]).abs().sum()
    loss.backward()
    _close12(ref["loss"], loss.detach(), "loss")
    assert torch.equal(ref["grad"], pd.grad) and torch.equal(ref["fg"], fg) and 0 < int(fg.sum()) < 257
    assert list(C.BOX_WEIGHTS) == list(R.CASCADE_WEIGHTS)
