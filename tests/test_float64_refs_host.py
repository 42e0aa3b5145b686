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
