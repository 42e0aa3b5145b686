"""The inference tails (u2seg_amd/csrc/postprocess.hip: mask paste, panoptic merge, semantic upsample + argmax, fp32 bilinear
resize, folded mask predictor + sigmoid) per element against float64 - the other tests of these kernels accept a share of wrong
pixels (1e-3 of a canvas, 64 per mask), skip every pixel near a decision, or compare one launch of a kernel with another.

References: tests/float64_refs.py (paste_ref, upsample_ref, resize_ref, mask_prob_ref - plain torch in float64 on the CPU, written
from the reference's formulas and held against independent formulations by tests/test_float64_refs_host.py) and, for the panoptic
merge, OracleModel.combine_panoptic (plain integer code).  Two kinds of check:

A. exact inputs, bit for bit, nothing excused.  Inputs are dyadic numbers chosen so that every product and every partial sum of the
   operation is an fp32 number (each generator's docstring derives it, each test asserts that the float64 result equals its own
   fp32 rounding); the fp32 kernel then has no rounding to hide behind, whatever its operation order: pasted masks, upsampled
   logits, argmax maps and resized maps must equal the reference everywhere, the mask predictor's logit must be the one bf16
   number the exact sum rounds to, the merge's map and segment list must equal the oracle's.  Ties and decisions that sit exactly
   on their threshold are built in.

B. random fp32 inputs, measured margin.  The margin is 4 x the largest deviation of the REFERENCE's own fp32 form (ATen on the CPU)
   from float64 on the very inputs of the test - the factor pays for the kernel's different, equally valid operation order - never
   a figure taken from the kernel.  A decision (threshold, argmax) may differ only where the float64 value lies inside that margin
   of it; the share of such pixels is capped at 0.1 %, and the same holds asserted for the reference's fp32 form alone.
   Values seen when this was written stand next to each assert."""
import pytest
import torch
import torch.nn.functional as TF

from tests import float64_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
BF16 = torch.bfloat16
SENTINEL = -7.0


class Env:
    pass


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from u2seg_amd import _hip
    from u2seg_amd.layers import functional
    from u2seg_amd.modeling import inference
    from u2seg_amd.structures import Boxes, Instances

    _hip.load()
    e = Env()
    e.hip, e.F, e.inf, e.Boxes, e.Instances = _hip, functional, inference, Boxes, Instances
    return e


def status(E, name, *args):
    """The launcher's return value (E.hip.call raises on anything but 0)."""
    rc = E.hip.call_nostream(name, *args, E.hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def report(name, what, value):
    print("TAILS64 %s | %s | %.4g" % (name, what, value))


def assert_same_mask(name, got, want):
    """A pasted bool canvas against the reference, every pixel; the stored bytes are 0 or 1."""
    got = got.cpu()
    assert got.dtype == torch.bool and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    raw = got.view(torch.uint8)
    assert int(raw.max()) <= 1 if raw.numel() else True, (name, "a byte other than 0 / 1")
    bad = raw != want.to(torch.uint8)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d pixels differ; first at (mask, y, x) = %s: got %d, want %d" % (
            name, int(bad.sum()), bad.numel(), i, int(raw[i]), int(want[i])))


# ----------------------------------------------------------------------------------------------------------------------------
# mask paste
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", R.PASTE_P)
def test_paste_exact_inputs_bit_for_bit(E, p):
    """paste_masks_in_image on float64_refs.paste_exact_case, every canvas of PASTE_CANVASES ((45, 53): masks start mid-word;
    (5, 3): a word spans rows and masks; (1, 1); (9, 8): W = 8; (16, 64): aligned rows), 13 masks (the byte tail and the memset tail
    of the zero fill wherever H W is no multiple of 16): boxes wholly off each side, partly off, covering the canvas, smaller than a
    pixel, 32 wide under P = 1 and 2.  Thresholds: 0.5 (the constant-0.5 map's interior is exactly on it and must be on, the map
    one step below all off), 1/256 and 1 (exact as well), and 0, where every pixel the map can reach at all - the `inside`
    predicate - is on, out to the rim of what the map can reach: a pixel that the rectangle the kernel samples per mask (paste_reach)
    leaves out is a pixel missing here.  (At 0.5 a lit pixel has its centre inside the box, far from that rectangle's rim.)"""
    on_thr = 0
    for h, w in R.PASTE_CANVASES:
        probs, boxes = R.paste_exact_case(p, h, w)
        v, inside = R.paste_ref(probs, boxes, h, w)
        assert torch.equal(v, v.float().to(F64)), "precondition: the float64 sample is an fp32 number"
        pd, bd = probs.to(DEV), boxes.to(DEV)
        for thr in (0.5, 0.0, 1.0 / 256, 1.0):
            got = E.inf.paste_masks_in_image(pd, bd, (h, w), thr)
            assert_same_mask("P %d canvas %s thr %g" % (p, (h, w), thr), got, inside & (v >= thr))
        on_thr += int((v[R.PASTE_HALF] == 0.5).sum())
    assert on_thr >= 3   # pixels exactly on the threshold were compared


def test_paste_random_inputs_decide_like_float64_outside_the_margin(E):
    """Random fp32 maps (smooth blobs and salt-and-pepper noise) and arbitrary fp32 boxes, P = 28 and 7, 45 x 53: a pixel may
    differ from paste_ref >= 0.5 only where |v64 - 0.5| < margin.  margin = 4 x max |grid_sample_fp32 - v64| over these inputs."""
    for p, seed in ((28, 11), (7, 12)):
        h, w = 45, 53
        probs, boxes = R.paste_random_case(p, h, w, 12, seed)
        v, inside = R.paste_ref(probs, boxes, h, w)
        v32 = R.paste_fp32(probs, boxes, h, w).to(F64)
        dev = float((v32 - v).abs().max())
        margin = 4 * dev      # measured on the CPU when written: dev 1.41e-6 (P = 28), 4.97e-7 (P = 7) -> margin 5.64e-6, 1.99e-6;
        #                       no pixel of either case lies inside its margin (0 of 7389 / 11096 in-box pixels)
        report("paste random P %d" % p, "max |fp32 - float64|", dev)
        assert 0 < margin < 1e-5
        near = inside & ((v - 0.5).abs() < margin)
        share = float(near.sum()) / float(inside.sum())
        report("paste random P %d" % p, "share of in-box pixels inside the margin", share)
        assert share <= 1e-3 and int(inside.sum()) > 5000
        want = inside & (v >= 0.5)
        assert torch.equal((v32 >= 0.5)[~near], want[~near])          # the reference's fp32 form alone: no mismatch outside
        got = E.inf.paste_masks_in_image(probs.to(DEV), boxes.to(DEV), (h, w)).cpu()
        bad = (got != want) & ~near
        assert not bool(bad.any()), (p, int(bad.sum()), bad.nonzero()[:4].tolist())
        assert 0.1 < float(want[inside].double().mean()) < 0.9


def test_paste_batched_launch_66_images_vs_float64(E):
    """paste_masks_in_images: 66 images (PASTE_MAXIMG = 64: two chunks) of mixed tiny canvases, images without masks in the middle,
    at the chunk boundary and at the end, exact inputs: every image bit for bit against paste_ref (not against the per-image
    launch, which is the same kernel)."""
    p = 7
    canvases = R.PASTE_CANVASES + [(7, 13), (3, 40)]
    counts = [3, 13, 1, 0, 5, 2, 13, 4]
    masks, boxes, shapes, want = [], [], [], []
    for i in range(66):
        h, w = canvases[i % len(canvases)]
        n = 0 if i in (20, 41, 63, 65) else counts[i % len(counts)]
        pr, bx = R.paste_exact_case(p, h, w)
        sel = [(i + 5 * j) % pr.shape[0] for j in range(n)]
        pr, bx = pr[sel], bx[sel]
        v, inside = R.paste_ref(pr, bx, h, w)
        assert torch.equal(v, v.float().to(F64))
        masks.append(pr.to(DEV))
        boxes.append(bx.to(DEV))
        shapes.append((h, w))
        want.append(inside & (v >= 0.5))
    got = E.inf.paste_masks_in_images(masks, boxes, shapes)
    assert len(got) == 66
    lit = 0
    for i in range(66):
        assert_same_mask("image %d canvas %s" % (i, shapes[i]), got[i], want[i])
        lit += int(want[i].sum())
    assert lit > 1000 and any(int(want[i].sum()) > 0 for i in (64,))


# ----------------------------------------------------------------------------------------------------------------------------
# semantic upsample + argmax
# ----------------------------------------------------------------------------------------------------------------------------
def sem_upsample(E, xd, k, s):
    """F.sem_seg_upsample; the launcher itself where the wrapper's activation check (channels % 32 == 0) does not admit the map."""
    if xd.shape[3] % 32 == 0:
        return E.F.sem_seg_upsample(xd, k, s)
    b, h, w, cp = xd.shape
    out = torch.empty((b, k, h * s, w * s), dtype=torch.float32, device=xd.device)
    amax = torch.empty((b, h * s, w * s), dtype=torch.int64, device=xd.device)
    E.hip.call("u2_semseg_upsample", xd, out, amax, b, h, w, cp, k, s)
    return out, amax


def nhwc_bf16(x):
    got = x.to(BF16)
    keep = ~torch.isnan(x)
    assert torch.equal(got.to(F64)[keep & (x.abs() < 1e29)], x[keep & (x.abs() < 1e29)]), "precondition: bf16 values"
    return got.to(DEV)


@pytest.mark.parametrize("k,cp", R.SEM_EXACT_CASES)
def test_semseg_upsample_exact_inputs_bit_for_bit(E, k, cp):
    """F.sem_seg_upsample (u2_semseg_upsample itself for Cp = 8) on float64_refs.upsample_exact_case, S in {2, 4}, maps (1, 1), (1, 5), (7, 1), (3, 5), K at the edges of
    the kernel's 8-channel groups: the logits equal upsample_ref bit for bit and the argmax is the FIRST maximum everywhere -
    identical channels, a patch where all channels are equal and an all-negative image are built in.  Pad channels [K, Cp) hold
    1e30 (NaN for (7, 32)) and must influence nothing."""
    pad = float("nan") if (k, cp) == (7, 32) else 1e30
    for h, w in R.SEM_MAPS:
        for s in (2, 4):
            x = R.upsample_exact_case(2, h, w, cp, k, pad)
            ref = R.upsample_ref(x, k, s)
            assert torch.equal(ref, ref.float().to(F64)), "precondition: the float64 logit is an fp32 number"
            out, amax = sem_upsample(E, nhwc_bf16(x), k, s)
            name = "K %d Cp %d map %s S %d" % (k, cp, (h, w), s)
            assert out.shape == ref.shape and out.dtype == torch.float32 and amax.dtype == torch.int64, name
            assert torch.equal(out.cpu().to(F64), ref), name
            assert torch.equal(amax.cpu(), R.first_argmax(ref)), name


def test_semseg_upsample_scale_1_null_pointers_and_refusals(E):
    """S = 1 is the identity; the ABI's two null-pointer variants (logits only, argmax only) write what the full call writes;
    the launcher refuses K > 64, K > Cp, Cp % 8 != 0 and S < 1 with -1 and writes nothing."""
    b, h, w, cp, k = 2, 3, 5, 32, 28
    x = R.upsample_exact_case(b, h, w, cp, k, 1e30)
    xd = nhwc_bf16(x)
    out, amax = E.F.sem_seg_upsample(xd, k, 1)
    ident = x[..., :k].permute(0, 3, 1, 2)
    assert torch.equal(out.cpu().to(F64), ident) and torch.equal(amax.cpu(), R.first_argmax(ident))
    ref = R.upsample_ref(x, k, 4)
    out = torch.full((b, k, 4 * h, 4 * w), SENTINEL, dtype=torch.float32, device=DEV)
    amax = torch.full((b, 4 * h, 4 * w), int(SENTINEL), dtype=torch.int64, device=DEV)
    assert status(E, "u2_semseg_upsample", xd, out, None, b, h, w, cp, k, 4) == 0
    assert torch.equal(out.cpu().to(F64), ref)
    assert status(E, "u2_semseg_upsample", xd, None, amax, b, h, w, cp, k, 4) == 0
    assert torch.equal(amax.cpu(), R.first_argmax(ref))
    for cp_, k_, s_ in ((72, 65, 2), (8, 9, 2), (12, 7, 2), (32, 28, 0), (32, 0, 2)):
        xr = torch.zeros((b, h, w, cp_), dtype=BF16, device=DEV)
        so = max(s_, 1)
        out = torch.full((b, max(k_, 1), so * h, so * w), SENTINEL, dtype=torch.float32, device=DEV)
        amax = torch.full((b, so * h, so * w), int(SENTINEL), dtype=torch.int64, device=DEV)
        assert status(E, "u2_semseg_upsample", xr, out, amax, b, h, w, cp_, k_, s_) == -1, (cp_, k_, s_)
        assert bool((out == SENTINEL).all()) and bool((amax == int(SENTINEL)).all()), (cp_, k_, s_)


def test_semseg_upsample_above_the_grid_cap(E):
    """B = 1, 368 x 368, S = 4, K = 1, Cp = 8: 2 166 784 output pixels, more than the launch's 8192 x 256 threads, so the grid-stride
    loop takes a second pass.  Exact inputs, every pixel compared."""
    x = R.upsample_exact_case(1, 368, 368, 8, 1, 1e30)
    ref = R.upsample_ref(x, 1, 4)
    assert ref.numel() > 8192 * 256 and torch.equal(ref, ref.float().to(F64))
    out, amax = sem_upsample(E, nhwc_bf16(x), 1, 4)
    assert torch.equal(out.cpu().to(F64), ref) and not bool(amax.any())


def test_semseg_upsample_scale_3_random_inputs(E):
    """S = 3 (weights in thirds: nothing is exact), random bf16 logits N(0, 3^2), K = 28 of Cp = 32 and K = 54 of 64: the logits
    within tol = 4 x max |ATen fp32 (CPU) - upsample_ref| on the same inputs; the argmax equal wherever the float64 top-2 gap
    exceeds 2 tol; at most 0.1 % of the pixels excused, and ATen's fp32 argmax held to the same.  (bf16 logits tie exactly now and
    then - typically 2 to 4 of these 1782 / 1440 pixels; the seeds are ones without, ties are the exact-input test's business.)"""
    for (b, h, w, cp, k, seed) in ((2, 9, 11, 32, 28, 3), (2, 5, 16, 64, 54, 6)):
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn((b, h, w, cp), generator=g) * 3).to(BF16)
        ref = R.upsample_ref(x, k, 3)
        aten = TF.interpolate(x[..., :k].float().permute(0, 3, 1, 2), scale_factor=3, mode="bilinear", align_corners=False)
        dev = float((aten.to(F64) - ref).abs().max())
        tol = 4 * dev      # measured on the CPU when written: dev 9.06e-6 (K = 28), 9.46e-6 (K = 54) -> tol 3.62e-5, 3.78e-5 (the fp32
        #                    source coordinate near 11 carries half an ulp, 5e-7, times a step between neighbours of up to ~ 20)
        report("upsample S 3 K %d" % k, "max |ATen fp32 - float64|", dev)
        assert 0 < tol < 1e-4
        out, amax = E.F.sem_seg_upsample(x.to(DEV), k, 3)
        err = float((out.cpu().to(F64) - ref).abs().max())
        report("upsample S 3 K %d" % k, "max |kernel - float64| / tol", err / tol)
        assert err <= tol
        top2 = ref.topk(2, dim=1).values
        decided = (top2[:, 0] - top2[:, 1]) > 2 * tol
        assert float((~decided).double().mean()) <= 1e-3
        want = R.first_argmax(ref)
        assert torch.equal(aten.argmax(1)[decided], want[decided])       # the reference's fp32 form alone
        assert torch.equal(amax.cpu()[decided], want[decided])
        assert torch.equal(amax, out.argmax(1))                          # and it is the argmax of the logits written


# ----------------------------------------------------------------------------------------------------------------------------
# fp32 bilinear resize
# ----------------------------------------------------------------------------------------------------------------------------
RESIZE_GENERAL = [((150, 200), (225, 300)), ((33, 47), (160, 224)), ((160, 224), (97, 133)), ((1, 47), (8, 100)), ((33, 1), (50, 7)),
                  ((33, 47), (1, 1))]


def test_resize_exact_scales_bit_for_bit(E):
    """sem_seg_postprocess x2 up and x1/2 down on dyadic inputs (multiples of 1/4, |v| <= 16: weights 1/4, 3/4 or 1/2, every
    product and sum an fp32 number), the source a window of a wider and taller map (channel and row strides differ from the
    window); and the same size through the ABI (the wrapper returns the window itself): the identity, bit for bit."""
    g = torch.Generator().manual_seed(8)
    full = torch.randint(-64, 65, (5, 19, 27), generator=g).float() / 4
    fd = full.to(DEV)
    for img, out in (((12, 20), (24, 40)), ((12, 20), (6, 10)), ((7, 5), (14, 10)), ((19, 27), (38, 54)), ((18, 26), (9, 13))):
        ref = R.resize_ref(full[:, : img[0], : img[1]], *out)
        assert torch.equal(ref, ref.float().to(F64)), "precondition: the float64 value is an fp32 number"
        got = E.inf.sem_seg_postprocess(fd, img, *out)
        assert got.shape == ref.shape and got.dtype == torch.float32 and torch.equal(got.cpu().to(F64), ref), (img, out)
    g = torch.Generator().manual_seed(9)
    full = torch.randn((3, 40, 50), generator=g)
    win = full.to(DEV)[:, :33, :47]
    out = torch.full((3, 33, 47), SENTINEL, dtype=torch.float32, device=DEV)
    assert status(E, "u2_bilinear_resize_f32", win, out, 3, 33, 47, win.stride(0), win.stride(1), 33, 47) == 0
    assert torch.equal(out.cpu(), full[:, :33, :47])
    assert torch.equal(R.resize_ref(full[:, :33, :47], 33, 47), full[:, :33, :47].to(F64))
    assert E.inf.sem_seg_postprocess(full.to(DEV), (33, 47), 33, 47).shape == (3, 33, 47)


def test_resize_general_scales_vs_float64(E):
    """sem_seg_postprocess at the scales of RESIZE_GENERAL (up, down, Hin = 1, Win = 1, a 1 x 1 output), N(0, 1) maps read as
    windows of a wider, taller map: within tol = 4 x max |ATen fp32 (CPU) - resize_ref| over these same inputs (all cases pooled:
    they share one value distribution, and the 1 x 1 output has three elements of its own)."""
    g = torch.Generator().manual_seed(3)
    full = torch.randn((3, 170, 240), generator=g)
    fd = full.to(DEV)
    refs, dev = [], 0.0
    for img, out in RESIZE_GENERAL:
        win = full[:, : img[0], : img[1]]
        ref = R.resize_ref(win, *out)
        aten = TF.interpolate(win[None], size=out, mode="bilinear", align_corners=False)[0]
        dev = max(dev, float((aten.to(F64) - ref).abs().max()))
        refs.append(ref)
    tol = 4 * dev          # measured on the CPU when written: dev 4.22e-5 ((160, 224) -> (97, 133)) -> tol 1.69e-4: the fp32 source
    #                        coordinate near 200 carries half an ulp, 7.6e-6, times a step between neighbours of up to ~ 6
    report("resize", "max |ATen fp32 - float64|", dev)
    assert 0 < tol < 1e-3
    for (img, out), ref in zip(RESIZE_GENERAL, refs):
        got = E.inf.sem_seg_postprocess(fd, img, *out)
        assert got.shape == ref.shape and got.dtype == torch.float32, (img, out)
        err = float((got.cpu().to(F64) - ref).abs().max())
        report("resize %s -> %s" % (img, out), "max |kernel - float64| / tol", err / tol)
        assert err <= tol, (img, out, err, tol)


# ----------------------------------------------------------------------------------------------------------------------------
# folded mask predictor + sigmoid
# ----------------------------------------------------------------------------------------------------------------------------
def mask_prob(E, xd, w, b, cls, phased=False):
    """F.mask_predict_prob; the launcher itself where the wrapper's activation check (channels % 32 == 0) does not admit x."""
    if xd.shape[3] % 32 == 0:
        return E.F.mask_predict_prob(xd, w, b, cls, phased=phased)
    n = xd.shape[0]
    side, c = (xd.shape[1] * 2, xd.shape[3] // 4) if phased else (xd.shape[1], xd.shape[3])
    out = torch.empty((n, 1, side, side), dtype=torch.float32, device=xd.device)
    E.hip.call("u2_mask_predict_prob", xd, w.reshape(w.shape[0], -1).contiguous(), b, cls, out, n, side, c, int(phased))
    return out


def check_prob(name, got, z):
    """fp32 probabilities against the expected bf16 logit z (float64), without a tolerance on expf: with
    ulp(z) = 2^(floor(log2 |z|) - 7), the bf16 spacing at z,
      z == 0:       p == 0.5;
      0 < |z| <= 8: |log(p / (1 - p)) - z| <= ulp / 4 (the fp32 error of p moves that logit by < 4e-4 at z = 8, where ulp / 4 is
                    1.6e-2, and by < 1e-6 near 0, where ulp / 4 >= 2^-17 for |z| >= 2^-8, the smallest non-zero logit);
      |z| > 8:      sigmoid(z - ulp / 4) - 2^-23 <= p <= sigmoid(z + ulp / 4) + 2^-23 (the sigmoid is monotone; 2^-23 pays for the
                    fp32 roundings of 1 + e^-z and of the quotient, each at most 2^-24 on a value below 1).
    A logit that is one bf16 ulp off fails all three."""
    p = got.cpu().to(F64)
    assert p.shape == z.shape, (name, p.shape, z.shape)
    az = z.abs()
    ulp = 2.0 ** (torch.floor(torch.log2(az.clamp(min=2.0 ** -100))) - 7)
    mid = (az > 0) & (az <= 8)
    logit = torch.log(p / (1 - p))
    ok = torch.where(az == 0, p == 0.5, torch.where(mid, (logit - z).abs() <= ulp / 4,
                                                     (p >= torch.sigmoid(z - ulp / 4) - 2.0 ** -23)
                                                     & (p <= torch.sigmoid(z + ulp / 4) + 2.0 ** -23)))
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        raise AssertionError("%s: %d of %d probabilities off; first at %s: p %r (logit %r), expected logit %r, bf16 ulp %r" % (
            name, int((~ok).sum()), ok.numel(), i, float(p[i]), float(logit[i]), float(z[i]), float(ulp[i])))
    return float(mid.double().mean())


@pytest.mark.parametrize("side", [1, 7, 14, 28])
@pytest.mark.parametrize("c", [8, 64, 256, 264, 520, 1024])
def test_mask_predict_prob_exact_inputs(E, c, side):
    """F.mask_predict_prob (u2_mask_predict_prob itself for C = 8, 264, 520) on float64_refs.mask_prob_case: x small integers, weights and bias integers times 2^-8, all bf16 numbers.
    Bound: every partial sum is an integer times 2^-8 of magnitude <= (C ax aw + 255) 2^-8 with C ax aw + 255 < 2^24 (asserted), so
    the fp32 sum is exact in any order and the stored logit must be RNE_bf16(exact sum) - unique; exact halves (odd multiples of
    2^-8 in [1, 2), asserted present by the host test) round to even.  C: one lane group (8), a quarter chunk (64), one full
    256-channel chunk, a partly filled second (264), a partly filled third (520), all four (1024); S2^2 odd and even; N = 1 with
    K = 1 and N = 37 with K = 800, first and last class selected; `phased` for the even sides: the same bits as the plain layout."""
    for n, k in ((1, 1), (37, 800)):
        x, w, b, cls, ax, aw = R.mask_prob_case(n, side, c, k)
        assert c * ax * aw + 255 < 1 << 24
        _, z = R.mask_prob_ref(x, w, b, cls)
        xd = x.to(BF16).to(DEV)
        assert torch.equal(xd.cpu().to(F64), x)
        wd, bd, cd = w.view(k, c, 1, 1).to(DEV), b.to(DEV), cls.to(DEV)
        got = mask_prob(E, xd, wd, bd, cd)
        name = "C %d S2 %d N %d K %d" % (c, side, n, k)
        assert got.shape == (n, 1, side, side) and got.dtype == torch.float32, name
        share = check_prob(name, got, z)
        if n * side * side >= 500:
            assert share > 0.3, (name, share)     # most logits are where bf16 rounds and the sigmoid still resolves them
        if side % 2 == 0:
            hs = side // 2
            xp = xd.view(n, hs, 2, hs, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(n, hs, hs, 4 * c).contiguous()  # [n, h, w, (dy, dx, c)]
            got_p = mask_prob(E, xp, wd, bd, cd, phased=True)
            assert torch.equal(got_p, got), name
            check_prob(name + " phased", got_p, z)


def test_mask_predict_prob_writes_only_its_n_p_elements_and_refusals(E):
    """Through the ABI with a guarded output: with an odd number of positions P = S2^2 the last position pair of a detection is half
    empty - nothing may be written past detection n's P elements (for the last detection: past the buffer), and the elements
    before the guard are the reference's.  Refusals: C = 4, C = 12, C = 1032 and `phased` with an odd side return -1, write nothing."""
    for n, side, c, k in ((1, 1, 8, 1), (3, 7, 264, 5), (2, 3, 64, 2)):
        x, w, b, cls, _, _ = R.mask_prob_case(n, side, c, k, seed=1)
        _, z = R.mask_prob_ref(x, w, b, cls)
        pp = side * side
        out = torch.full((n * pp + 64,), SENTINEL, dtype=torch.float32, device=DEV)
        assert status(E, "u2_mask_predict_prob", x.to(BF16).to(DEV), w.to(DEV), b.to(DEV), cls.to(DEV), out, n, side, c, 0) == 0
        assert bool((out[n * pp:] == SENTINEL).all()), (n, side, c)
        check_prob("guarded C %d S2 %d" % (c, side), out[: n * pp].view(n, 1, side, side), z)
    for side, c, phased in ((2, 4, 0), (2, 12, 0), (2, 1032, 0), (7, 64, 1)):
        xr = torch.zeros((2, side, side, c), dtype=BF16, device=DEV)
        wr, br = torch.zeros((3, c), device=DEV), torch.zeros(3, device=DEV)
        cr = torch.zeros(2, dtype=torch.int64, device=DEV)
        out = torch.full((2 * side * side,), SENTINEL, dtype=torch.float32, device=DEV)
        assert status(E, "u2_mask_predict_prob", xr, wr, br, cr, out, 2, side, c, phased) == -1, (side, c, phased)
        assert bool((out == SENTINEL).all()), (side, c, phased)


# ----------------------------------------------------------------------------------------------------------------------------
# panoptic merge
# ----------------------------------------------------------------------------------------------------------------------------
OVERLAP_THR, STUFF_AREA_THR, SCORE_THR = 0.5, 5, 0.5


def rect(h, w, y0, y1, x0, x1):
    m = torch.zeros((h, w), dtype=torch.bool)
    m[y0:y1, x0:x1] = True
    return m


def sem0():
    """6 x 8 label map: label 3 on exactly STUFF_AREA_THR pixels (kept), label 4 on one fewer (dropped), label 7 on 24, label 255
    (the kernel's top slot) on 6, label 0 ("things") on the rest."""
    s = torch.zeros((6, 8), dtype=torch.int64)
    s[0, :5], s[1, :4], s[2:5, :], s[5, :6] = 3, 4, 7, 255
    return s


def panoptic_cases():
    """name -> (masks [K, H, W] bool, scores [K] fp32, sem [H, W] int64).  Thresholds (OVERLAP_THR, STUFF_AREA_THR, SCORE_THR)."""
    r = lambda *a: rect(6, 8, *a)     # noqa: E731
    none = torch.zeros((6, 8), dtype=torch.bool)
    cases = {}
    cases["no instances; stuff area == threshold kept, one less dropped; label 255"] = (torch.zeros((0, 6, 8), dtype=torch.bool), [], sem0())
    cases["every score below the threshold"] = (torch.stack([r(2, 4, 0, 3), r(3, 5, 2, 6)]), [0.25, 0.4990234375], sem0())
    cases["score == threshold kept, the next below dropped"] = (torch.stack([r(3, 5, 2, 6), r(2, 4, 0, 3)]), [0.4990234375, 0.5], sem0())
    cases["empty mask in the middle of the order"] = (torch.stack([r(2, 4, 0, 3), none, r(3, 5, 2, 6)]), [0.75, 0.875, 0.625], sem0())
    # mask 0: rows 2-3 x cols 0-2 (6 px).  mask 1: row 2, cols 0-5 (6 px, 3 claimed): 2 inter == area -> kept, claims 3.
    # mask 2: row 3 cols 0-4 and (2, 5) (6 px, 4 claimed): one pixel more -> rejected.  mask 3: row 4 + (3, 0): 9 px, 1 claimed: kept.
    m2 = r(3, 4, 0, 5) | r(2, 3, 5, 6)
    m3 = r(4, 5, 0, 8) | r(3, 4, 0, 1)
    cases["overlap ratio == threshold kept, one pixel more rejected"] = (torch.stack([r(2, 4, 0, 3), r(2, 3, 0, 6), m2, m3]),
                                                                        [0.875, 0.75, 0.625, 0.5], sem0())
    # the instance takes one of label 3's five pixels (4 left: dropped) and none of label 255's
    cases["stuff area one below the threshold after an instance"] = (torch.stack([r(0, 1, 0, 1)]), [0.75], sem0())
    # tied scores: the detection order decides.  (0) cols 0-3, (1) cols 2-5: 2 of 4 claimed, kept; (2) cols 0-7: 6 of 8, rejected
    cases["tied scores"] = (torch.stack([r(2, 3, 0, 4), r(2, 3, 2, 6), r(2, 3, 0, 8)]), [0.75, 0.75, 0.75], sem0())
    cases["tied scores, other order"] = (torch.stack([r(2, 3, 0, 8), r(2, 3, 2, 6), r(2, 3, 0, 4)]), [0.75, 0.75, 0.75], sem0())
    # 8 x 1: label 3 on six pixels; mask 0 rows 6-7; mask 1 rows 5-6 (1 of 2 claimed: kept) takes one of label 3's: 5 left, kept
    col = torch.tensor([3, 3, 3, 3, 3, 3, 0, 9], dtype=torch.int64).view(8, 1)
    cases["one-column map"] = (torch.stack([rect(8, 1, 6, 8, 0, 1), rect(8, 1, 5, 7, 0, 1)]), [0.75, 0.625], col)
    cases["one pixel"] = (torch.ones((1, 1, 1), dtype=torch.bool), [0.5], torch.full((1, 1), 255, dtype=torch.int64))
    return cases


def run_merge(E, items, mask_res=0, window=False):
    """items: list of (masks bool [K, H, W] (CPU or device), scores, sem int64 [H, W] CPU, boxes or None) -> the batch routine's
    results next to OracleModel.combine_panoptic's, compared bit for bit (map and segment list)."""
    from oracle.model import OracleModel

    insts, sems, keep = [], [], []
    for masks, scores, sem, boxes in items:
        k, h, w = masks.shape
        inst = E.Instances((h, w))
        inst.pred_masks = masks.to(DEV)
        inst.scores = torch.tensor(scores, dtype=torch.float32).to(DEV)
        inst.pred_classes = ((torch.arange(k) * 37 + 11) % 800).to(DEV)
        if boxes is not None:
            inst.pred_boxes = E.Boxes(boxes.to(DEV))
        insts.append(inst)
        if window:   # the label map as an int64 window of a wider, taller map: the row pitch is not W
            wide = torch.full((h + 2, w + 5), 200, dtype=torch.int64)
            wide[1: 1 + h, 2: 2 + w] = sem
            wide = wide.to(DEV)
            keep.append(wide)
            sems.append(wide[1: 1 + h, 2: 2 + w])
            assert sems[-1].stride(0) == w + 5
        else:
            sems.append(sem.to(DEV))
    got = E.inf.combine_semantic_and_instance_outputs_batch(insts, sems, OVERLAP_THR, STUFF_AREA_THR, SCORE_THR, mask_res)
    assert len(got) == len(items)
    out = []
    for i, ((masks, scores, sem, _), (pan, info)) in enumerate(zip(items, got)):
        k = masks.shape[0]
        ref_pan, ref_info = OracleModel.combine_panoptic(masks.cpu(), torch.tensor(scores, dtype=torch.float32),
                                                         (torch.arange(k) * 37 + 11) % 800, sem, OVERLAP_THR, STUFF_AREA_THR, SCORE_THR)
        assert pan.dtype == torch.int32 and torch.equal(pan.cpu(), ref_pan), (i, pan.cpu().tolist(), ref_pan.tolist())
        assert info == ref_info, (i, info, ref_info)
        out.append((pan.cpu(), info))
    return out


def test_panoptic_merge_decision_edges_vs_oracle(E):
    """combine_semantic_and_instance_outputs_batch on hand-made maps of a few dozen pixels (far fewer than the work-group has
    threads), one launch per case and all in one launch, the label map dense and as an int64 window of a wider map: map and segment
    list equal OracleModel.combine_panoptic's bit for bit.  What each case pins is spelled out so that it cannot erode."""
    cases = panoptic_cases()
    res = {}
    for name, (masks, scores, sem) in cases.items():
        (res[name],) = run_merge(E, [(masks, scores, sem, None)])
        (again,) = run_merge(E, [(masks, scores, sem, None)], window=True)
        assert torch.equal(again[0], res[name][0]) and again[1] == res[name][1], name
    both = run_merge(E, [(m, s, sem, None) for (m, s, sem) in cases.values()])
    assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(both, res.values()))

    def things(name):
        return [d["instance_id"] for d in res[name][1] if d["isthing"]]

    def stuff(name):
        return {d["category_id"]: d["area"] for d in res[name][1] if not d["isthing"]}

    first = "no instances; stuff area == threshold kept, one less dropped; label 255"
    assert things(first) == [] and stuff(first) == {3: 5, 7: 24, 255: 6}
    assert things("every score below the threshold") == []
    assert things("score == threshold kept, the next below dropped") == [1]
    assert things("empty mask in the middle of the order") == [0, 2]
    assert things("overlap ratio == threshold kept, one pixel more rejected") == [0, 1, 3]
    assert stuff("stuff area one below the threshold after an instance") == {7: 24, 255: 6}
    assert things("tied scores") == [0, 1] and things("tied scores, other order") == [0]
    assert things("one-column map") == [0, 1] and stuff("one-column map") == {3: 5}
    assert things("one pixel") == [0] and stuff("one pixel") == {}


def test_panoptic_merge_41_images_in_one_call(E):
    """41 images (PM_MAXIMG = 40: two launches) of different sizes, one without instances, random rectangles with scores on a grid of
    1/8 (ties, and scores equal to the threshold), labels from {0, 3, 4, 7, 255}: every image equals the oracle."""
    g = torch.Generator().manual_seed(41)
    sizes = [(6, 8), (7, 1), (3, 5), (1, 1), (10, 12), (33, 35)]
    labels = torch.tensor([0, 3, 4, 7, 255])
    items = []
    for i in range(41):
        h, w = sizes[i % len(sizes)]
        k = 0 if i == 17 else 1 + i % 6
        masks = torch.zeros((k, h, w), dtype=torch.bool)
        for j in range(k):
            y0, x0 = int(torch.randint(0, h, (1,), generator=g)), int(torch.randint(0, w, (1,), generator=g))
            masks[j, y0: y0 + 1 + int(torch.randint(0, h, (1,), generator=g)), x0: x0 + 1 + int(torch.randint(0, w, (1,), generator=g))] = True
        scores = (torch.randint(2, 9, (k,), generator=g).float() / 8).tolist()
        sem = labels[torch.randint(0, 5, ((h + 1) // 2, (w + 2) // 3), generator=g)].repeat_interleave(2, 0).repeat_interleave(3, 1)[:h, :w]
        items.append((masks, scores, sem.contiguous(), None))
    out = run_merge(E, items)
    assert sum(len(info) for _, info in out) > 60 and out[17][1] == [d for d in out[17][1] if not d["isthing"]]
    assert any(d["isthing"] for d in out[40][1]) or any(d["isthing"] for d in out[39][1])


@pytest.mark.parametrize("p", [1, 2, 28])
def test_panoptic_merge_bounded_scan_equals_full_scan_and_oracle(E, p):
    """mask_res = P restricts each instance's scan to the pixels its pasted mask can reach.  Masks: the device paste of the
    exact-input cases above (boxes at and beyond the borders; P = 1, 2: the reach past the box is largest), thresholds 0.5 and 0
    (at 0 every reachable pixel is on, so a scan rectangle one pixel short loses area): equal to the mask_res = 0 result and to
    the oracle."""
    n_things = 0
    for h, w in ((45, 53), (9, 8), (5, 3)):
        probs, boxes = R.paste_exact_case(p, h, w)
        g = torch.Generator().manual_seed(p + h)
        scores = (torch.randint(4, 17, (boxes.shape[0],), generator=g).float() / 16).tolist()
        sem = torch.tensor([0, 3, 7, 255])[torch.randint(0, 4, (h, w), generator=g)]
        sem[: h // 2] = 7
        for thr in (0.5, 0.0):
            masks = E.inf.paste_masks_in_image(probs.to(DEV), boxes.to(DEV), (h, w), thr)
            (full,) = run_merge(E, [(masks, scores, sem, boxes)], mask_res=0)
            (bounded,) = run_merge(E, [(masks, scores, sem, boxes)], mask_res=p)
            assert torch.equal(full[0], bounded[0]) and full[1] == bounded[1]
            n_things += sum(d["isthing"] for d in full[1])
    assert n_things >= 6, n_things   # instances were merged (with P = 1 at 0.5 a small canvas may hold none)
