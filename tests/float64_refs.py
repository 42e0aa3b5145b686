"""Float64 reference helpers of tests/test_gpu_optim_resample_float64.py and tests/test_gpu_conv_float64.py, in a plain module so that the CPU tests of
tests/test_float64_refs_host.py check exactly what the GPU tests use.  Plain torch ops only; nothing here touches the HIP
library.  Every function works on whatever device its inputs live on."""
import torch
import torch.nn.functional as TF

F64 = torch.float64
CHUNK = 1 << 16        # solver/build.py CHUNK: elements per optimizer chunk
OPT_THREADS = 1024     # optim.hip: threads per chunk

# Tensor sizes of the direct optimizer test, in arena order.  Offsets (b & 3 in brackets):
#   5 @ 0 [0]            aligned start, head 0, one float4, tail 1
#   3 @ 5 [1]            the head takes the whole tensor (nvec == 0)
#   9 @ 8 [0]
#   2 @ 17 [1]           head = min(3, 2): the whole tensor
#   1 @ 19 [3]           head 1: the whole tensor
#   65 536 @ 20 [0]      exactly one full chunk
#   65 537 @ 65 556 [0]  the second chunk has one element (no head, no float4, tail 1)
#   196 613 @ 131 093 [1]  four chunks, every one starts at b & 3 == 1, the last has 5 elements
#   6 @ 327 706 [2]      head 2, one float4
#   7 @ 327 712 [0]      one float4 and the tail of 3
A2_SIZES = [5, 3, 9, 2, 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 6, 7]


def chunk_tables(sizes):
    """The optimizer's chunk tables by the rule of FlatSGD.__init__, restated: a tensor of n elements at arena offset `off`
    is cut into ceil(n / CHUNK) chunks [off + s, off + min(s + CHUNK, n)); first_chunk[t] .. first_chunk[t + 1] are tensor t's.
    Returns python lists (chunk_tensor, chunk_begin, chunk_len, first_chunk)."""
    chunk_tensor, chunk_begin, chunk_len, first_chunk = [], [], [], []
    off = 0
    for t, n in enumerate(sizes):
        first_chunk.append(len(chunk_tensor))
        s = 0
        while s < n:
            chunk_tensor.append(t)
            chunk_begin.append(off + s)
            chunk_len.append(min(CHUNK, n - s))
            s += CHUNK
        off += n
    first_chunk.append(len(chunk_tensor))
    return chunk_tensor, chunk_begin, chunk_len, first_chunk


def sumsq_depth(n_chunks):
    """d: the longest chain of fp32 roundings behind a tensor's squared norm n2 in optim.hip (all terms non-negative):
      sumsq_kernel, per thread: a chunk has at most CHUNK / 4 float4, OPT_THREADS threads -> 16 loop passes; an element's square (1),
        the two levels of the pass's (x^2 + y^2) + (z^2 + w^2) tree (2), then one `s +=` per pass from its own on (<= 16): 19;
      the head / tail element's `s +=`: 1;   wave_sum: 6 shuffle levels;   the 16 wave sums added in order: 16;
      sgd_kernel: one addition per chunk of the tensor.
    Recursive summation of non-negative terms over a chain of length d errs by at most d u relative (to first order)."""
    per_thread = 1 + 2 + (CHUNK // 4 + OPT_THREADS - 1) // OPT_THREADS
    return per_thread + 1 + 6 + OPT_THREADS // 64 + n_chunks


def _per_tensor(values, sizes, like):
    """[n_tensors] -> one value per arena element."""
    v = torch.as_tensor(values, dtype=F64, device=like.device)
    return torch.repeat_interleave(v, torch.as_tensor(sizes, device=like.device))


def sgd_clip_coef(g, sizes, clip, scale):
    """Per-tensor gradient coefficient of clip_grad_norm_(p, clip, 2.0) on gradients pre-scaled by `scale` (float64, [n_tensors]):
    min(clip / (||g|| scale + 1e-6), 1) scale; `scale` where clip == 0 (no clipping)."""
    g = g.to(F64)
    if clip == 0:
        return torch.full((len(sizes),), float(scale), dtype=F64, device=g.device)
    norms = torch.stack([piece.norm() for piece in torch.split(g, list(sizes))])
    return torch.clamp(clip / (norms * scale + 1e-6), max=1.0) * scale


def sgd_clip_ref(p, g, m, sizes, wd, lr, mom, clip, scale):
    """One step of per-parameter L2 clipping + SGD(momentum, weight decay) over a flat arena, in float64:
    m' = mom m + g coef + wd p,  p' = p - lr m'.  p, g, m: [sum(sizes)]; wd: one value per tensor.  Returns (p', m')."""
    p, g, m = p.to(F64), g.to(F64), m.to(F64)
    coef = _per_tensor(sgd_clip_coef(g, sizes, clip, scale), sizes, p)
    m1 = mom * m + g * coef + _per_tensor(wd, sizes, p) * p
    return p - lr * m1, m1


def sgd_clip_bounds(p, g, m, sizes, wd, lr, mom, clip, scale, u):
    """Per-element bounds (e_p, e_m) of the fp32 kernel's error on (p', m') of sgd_clip_ref - the derivation is in the
    docstring of test_sgd_clip_step_abi_vs_float64."""
    p, g, m = p.to(F64), g.to(F64), m.to(F64)
    coef = sgd_clip_coef(g, sizes, clip, scale)
    if clip == 0:
        eps_c = torch.zeros(len(sizes), dtype=F64)   # coef is the scalar handed in: no arithmetic behind it
    else:
        eps_c = torch.tensor([(sumsq_depth(-(-n // CHUNK)) / 2 + 4) * u for n in sizes], dtype=F64)
    gc = (g * _per_tensor(coef, sizes, p)).abs()
    wp = (_per_tensor(wd, sizes, p) * p).abs()
    e_m = _per_tensor(eps_c, sizes, p) * gc + 4 * u * (gc + wp + (mom * m).abs())
    m1 = mom * m + g * _per_tensor(coef, sizes, p) + _per_tensor(wd, sizes, p) * p
    e_p = lr * e_m + 2 * u * (p.abs() + lr * m1.abs())
    return e_p, e_m


# ---- max pool 3x3 stride 2 ----
def slots_from_indices(ind, w_in, row_off=-1, col_off=-1):
    """max_pool2d(..., return_indices=True) -> the window slot ky * 3 + kx (uint8) the kernels record.  ind: [B, C, Ho, Wo]
    flat indices iy * w_in + ix into the (unpadded) input plane; window (oy, ox) starts at input row 2 oy + row_off and column
    2 ox + col_off (padding 1: -1; a band whose first row is already the window's first: 0)."""
    ho, wo = ind.shape[2], ind.shape[3]
    iy = torch.div(ind, w_in, rounding_mode="floor")
    ix = ind - iy * w_in
    oy = torch.arange(ho, device=ind.device).view(1, 1, ho, 1)
    ox = torch.arange(wo, device=ind.device).view(1, 1, 1, wo)
    ky, kx = iy - (2 * oy + row_off), ix - (2 * ox + col_off)
    assert bool(((ky >= 0) & (ky < 3) & (kx >= 0) & (kx < 3)).all())
    return (ky * 3 + kx).to(torch.uint8)


def brute_force_slots(x):
    """Pooled values and winner slots of a 3x3 / stride 2 / pad 1 max pool by an explicit scan of the nine taps in slot
    order; a later tap wins only if strictly greater (the first maximum wins), padding never does.  x: [B, C, H, W]."""
    b, c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = TF.pad(x, (1, 2, 1, 2), value=float("-inf"))
    best = torch.full((b, c, ho, wo), float("-inf"), dtype=x.dtype, device=x.device)
    slot = torch.zeros((b, c, ho, wo), dtype=torch.uint8, device=x.device)
    for k in range(9):
        tap = xp[:, :, k // 3: k // 3 + 2 * ho: 2, k % 3: k % 3 + 2 * wo: 2]
        win = tap > best
        best = torch.where(win, tap, best)
        slot = torch.where(win, torch.full_like(slot, k), slot)
    return best, slot


def tie_values(shape, generator, device):
    """Multiples of 0.5 in [-2, 0]: many exact ties, and windows whose values are all negative."""
    return -0.5 * torch.randint(0, 5, shape, generator=generator, device=device).to(F64)


# ---- stem input ----
def stem_unfold_ref(canvas):
    """canvas [B, 3, Hp, Wp] (normalised image on the zero canvas) -> im2col rows of the 7x7 / stride 2 / pad 3 stem conv,
    [B, Ho * Wo, 147] with K ordered (kh, kw, c): the layout u2_stem_im2col_batch writes and weight.permute(0, 2, 3, 1) reads."""
    b = canvas.shape[0]
    cols = TF.unfold(canvas, kernel_size=7, stride=2, padding=3)         # [B, 3 * 49, L], K ordered (c, kh, kw)
    length = cols.shape[2]
    return cols.view(b, 3, 7, 7, length).permute(0, 4, 2, 3, 1).reshape(b, length, 147)


def stem_canvas(images, mean, std, hpad, wpad):
    """(img - mean) / std in float64 on the zero canvas, and the indicator of canvas pixels inside an image."""
    b = len(images)
    dev = images[0].device
    canvas = torch.zeros((b, 3, hpad, wpad), dtype=F64, device=dev)
    inside = torch.zeros((b, 3, hpad, wpad), dtype=F64, device=dev)
    mean, std = mean.to(F64).view(3, 1, 1), std.to(F64).view(3, 1, 1)
    for i, im in enumerate(images):
        h, w = im.shape[1], im.shape[2]
        canvas[i, :, :h, :w] = (im.to(F64) - mean) / std
        inside[i, :, :h, :w] = 1
    return canvas, inside


# ---- convolution family (tests/test_gpu_conv_float64.py) ----
TWO24 = float(1 << 24)   # every integer below it is an fp32 value: sums of integer terms with sum |term| < 2^24 are exact in any order
U24 = 2.0 ** -24         # fp32 unit roundoff


def rne_bf16(x):
    """float64 -> the nearest bf16 value, ties to even, as float64.  Integer arithmetic on the float64 bit pattern (45 of the
    52 fraction bits go), so the same on every device; bf16's exponent range is not modelled: |x| is 0 or in [2^-126, 2^127)."""
    x = x.to(F64).contiguous()
    ax = x.abs()
    assert bool(((ax == 0) | ((ax >= 2.0 ** -126) & (ax < 2.0 ** 127))).all())
    bits = x.view(torch.int64)
    bits = bits + ((1 << 44) - 1) + ((bits >> 45) & 1)
    return (bits & ~((1 << 45) - 1)).view(F64)


def conv_out_size(h, w, kh, kw, stride, ph, pw):
    return (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1


def _cols(x, kh, kw, stride, ph, pw):
    return TF.unfold(x, (kh, kw), padding=(ph, pw), stride=stride)   # [B, C * KH * KW, Ho * Wo], K ordered (c, kh, kw)


def conv_fwd_ref(x, w, stride, ph, pw, bias=None):
    """Convolution from unfold + matmul in float64 with its magnitude sum: (y, A), both [B, N, Ho, Wo];
    y = sum of terms x w (+ bias), A = sum of |term| (+ |bias|).  x [B, C, H, W], w [N, C, KH, KW]."""
    b, _, h, wd = x.shape
    n, _, kh, kw = w.shape
    ho, wo = conv_out_size(h, wd, kh, kw, stride, ph, pw)
    cols = _cols(x.to(F64), kh, kw, stride, ph, pw)
    wm = w.to(F64).reshape(n, -1)
    y, a = wm @ cols, wm.abs() @ cols.abs()
    if bias is not None:
        y, a = y + bias.to(F64).view(1, n, 1), a + bias.to(F64).abs().view(1, n, 1)
    return y.view(b, n, ho, wo), a.view(b, n, ho, wo)


def conv_dgrad_ref(dy, w, in_hw, stride, ph, pw):
    """Data gradient built the same way: the columns' gradient w^T dy folded back onto the input, and its magnitude sum.
    dy [B, N, Ho, Wo] -> (dx, A) [B, C, H, W]."""
    b, n = dy.shape[:2]
    _, c, kh, kw = w.shape
    wm = w.to(F64).reshape(n, -1)
    d = dy.to(F64).reshape(b, n, -1)
    fold = lambda t: TF.fold(t, in_hw, (kh, kw), padding=(ph, pw), stride=stride)
    return fold(wm.t() @ d), fold(wm.abs().t() @ d.abs())


def conv_wgrad_ref(x, dy, kh, kw, stride, ph, pw):
    """Weight gradient dw[n][c][kh][kw] = sum over images and output pixels of dy x(source pixel), and its magnitude sum."""
    b, c = x.shape[:2]
    n = dy.shape[1]
    cols = _cols(x.to(F64), kh, kw, stride, ph, pw)
    d = dy.to(F64).reshape(b, n, -1)
    dw = torch.einsum("bnl,bkl->nk", d, cols)
    a = torch.einsum("bnl,bkl->nk", d.abs(), cols.abs())
    return dw.view(n, c, kh, kw), a.view(n, c, kh, kw)


def fp32_sum_bound(length, a):
    """E = (L + 2) 2^-24 A: an fp32 sum of L terms in any order errs by at most (L - 1) u A to first order (each of the L - 1
    additions rounds a partial sum that is at most A in magnitude); the products of two bf16 values are exact in fp32; the 2 pays
    for the bias add and the epilogue, and the slack of 1 covers the second-order terms (L u << 1 at every L used here)."""
    return (length + 2) * U24 * a


def bf16_interval(ref, e, relu=False, old=None):
    """[lo, hi] of the stored bf16 value for an fp32 result within e of ref: RNE_bf16 of both ends (rounding is monotone), then -
    both monotone too - the accumulating epilogue's second rounding RNE_bf16(. + old) and the ReLU."""
    lo, hi = rne_bf16(ref - e), rne_bf16(ref + e)
    if old is not None:
        lo, hi = rne_bf16(lo + old.to(F64)), rne_bf16(hi + old.to(F64))
    if relu:
        lo, hi = lo.clamp(min=0), hi.clamp(min=0)
    return lo, hi


def exact_amp(length, other=None):
    """Amplitude a of the exact-input generator: integers uniform in {-a .. a} have variance a (a + 1) / 3, so a sum of
    `length` products with a factor of amplitude `other` (default: a itself) has the standard deviation
    sqrt(length a (a + 1) / 3 other (other + 1) / 3) - the smallest a in 2 .. 16 that puts it at 512 or more (a good share of the
    sums then lies past 256, where bf16 no longer holds every integer); 16 for short sums."""
    for a in range(2, 17):
        o = a if other is None else other
        if (length * a * (a + 1) * o * (o + 1)) ** 0.5 / 3 >= 512:
            return a
    return 16


def ints(shape, amp, g):
    return torch.randint(-amp, amp + 1, tuple(shape), generator=g).to(F64)


def bf16_round(t):
    return t.float().bfloat16().to(F64)


def conv_operands(geom, mode, amp=None):
    """Operands of one convolution case as float64 tensors whose values are bf16 numbers: x [B, Cin, H, W], w [N, Cin, KH, KW],
    bias [N], gy [B, N, Ho, Wo], old [B, N, Ho, Wo] (the accumulating epilogue's stored values).
    geom = (B, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w).
    mode "exact": small integers (amplitudes by exact_amp of the forward and data-gradient sum lengths - the taps that fall
      inside the map, not those in the padding - or `amp` for all).
    mode "real": x = relu(N(mu_c, 1)), mu_c drawn from {0, 1, 4}, channel 0 all zero, channel 1 with a few values of 2^6;
      w = N(0, 1 / K) + a per-filter offset U(-1, 1) / K; gy = N(0, 1) 2^-10."""
    b, h, wd, cin, cout, kh, kw, stride, ph, pw = geom
    g = torch.Generator().manual_seed(sum((i + 1) * 7919 * v for i, v in enumerate(geom)) % (2 ** 31) + (mode == "real"))
    ho, wo = conv_out_size(h, wd, kh, kw, stride, ph, pw)
    k = kh * kw * cin
    if mode == "exact":
        # the terms an output really has: taps inside the map (a one-pixel map under a 7x7 filter meets one tap), on average
        inside = float(_cols(torch.ones((1, 1, h, wd), dtype=F64), kh, kw, stride, ph, pw).sum(1).mean())
        a_f = amp or exact_amp(max(1, round(cin * inside)))
        x, w = ints((b, cin, h, wd), a_f, g), ints((cout, cin, kh, kw), a_f, g)
        bias, old = ints((cout,), 16 * a_f, g), ints((b, cout, ho, wo), 16 * a_f, g)
        # data gradient: taps * Cout terms, of which a stride-s layer meets one in s^2
        a_g = amp or exact_amp(max(1, round(cout * inside * ho * wo / (h * wd))), a_f)   # every term of y is one of dx too
        gy = ints((b, cout, ho, wo), a_g, g)
        return x, w, bias, gy, old
    assert mode == "real"
    mu = torch.tensor([0.0, 1.0, 4.0], dtype=F64)[torch.randint(0, 3, (cin,), generator=g)]
    x = torch.relu(torch.randn((b, cin, h, wd), generator=g, dtype=F64) + mu.view(1, cin, 1, 1))
    x[:, 0] = 0
    if cin > 1:
        flat = x[:, 1].reshape(-1).clone()
        flat[torch.randint(0, flat.numel(), (min(3, flat.numel()),), generator=g)] = 64.0
        x[:, 1] = flat.view(b, h, wd)
    w = torch.randn((cout, cin, kh, kw), generator=g, dtype=F64) / k ** 0.5 \
        + (torch.rand((cout, 1, 1, 1), generator=g, dtype=F64) * 2 - 1) / k
    bias = torch.randn((cout,), generator=g, dtype=F64) * 0.1
    gy = torch.randn((b, cout, ho, wo), generator=g, dtype=F64) * 2.0 ** -10
    old = torch.relu(torch.randn((b, cout, ho, wo), generator=g, dtype=F64) + 1)
    return tuple(bf16_round(t) for t in (x, w, bias, gy, old))


def g3(b, h, w, cin, cout, k=3, stride=1, pad=None):
    """geom of a square filter with symmetric padding (default: 'same' for odd k)."""
    pad = k // 2 if pad is None else pad
    return (b, h, w, cin, cout, k, k, stride, pad, pad)


# The cases of tests/test_gpu_conv_float64.py, here so that the CPU twin checks the generator's preconditions on every one.
VARIANT_SHAPES = [g3(2, 36, 32, 64, 256), g3(2, 35, 31, 64, 256)]
GENERIC_LAYERS = [(32, 8, 1, 1, 0), (64, 40, 3, 1, 1), (128, 96, 3, 2, 1), (256, 40, 1, 2, 0), (32, 28, 5, 1, 2), (32, 64, 7, 2, 3)]
GENERIC_MAPS = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 19, 23), (1, 8, 8)]
GENERIC_GEOMS = [g3(b, h, w, cin, cout, k, s, p) for (cin, cout, k, s, p) in GENERIC_LAYERS for (b, h, w) in GENERIC_MAPS]
ASYM_GEOM = (2, 9, 11, 32, 40, 1, 3, 1, 0, 1)   # KH != KW, pad_h != pad_w (C ABI only)
STRIDE2_MAPS = [(1, 1), (1, 2), (2, 1), (7, 9), (8, 10)]
STRIDE2_GEOMS = [g3(2, h, w, 64, 64, k, 2, p) for (k, p) in ((1, 0), (3, 1)) for (h, w) in STRIDE2_MAPS]
HALO_MAPS = [(1, 5, 7), (2, 16, 32), (2, 17, 33), (1, 33, 65)]
HALO_CHANNELS = [(64, 64), (96, 40), (256, 64), (32, 8)]
HALO_GEOMS = [g3(b, h, w, cin, cout) for (cin, cout) in HALO_CHANNELS for (b, h, w) in HALO_MAPS]
# conv_stream.hip: pixels one work-group's LDS ring holds (ring stages x pixel tile) by input channels; with the 8-work-group
# grid of the tests (bit 16) a channel block's eight walkers pass their ring's end at 8 x that many pixels
STREAM_RING_PIXELS = {32: 8 * 128, 64: 5 * 128, 128: 5 * 64, 256: 5 * 64}
STREAM_CIN, STREAM_COUT = [32, 64, 128, 256], [40, 104, 264, 520]


def stream_pixel_counts(cin):
    full = 8 * STREAM_RING_PIXELS[cin]
    return [1, 63, full - 1, full + 1]


STREAM_GEOMS = [g3(1, 1, m, cin, cout, 1) for cin in STREAM_CIN for cout in STREAM_COUT for m in stream_pixel_counts(cin)]
ACC_GEOMS = [g3(2, 37, 41, 64, 256, 1), g3(3, 20, 24, 256, 1024, 1), g3(1, 1, 1, 64, 256, 1)]
LONGK_GEOMS = [g3(2, 5, 7, 2048, 512, 1), g3(1, 65, 1, 768, 2304, 1), g3(1, 65, 1, 3072, 768, 1)]
FC_GEOM = g3(37, 7, 7, 256, 1024, 7, 1, 0)
WGRAD_TAP_GEOMS = [g3(2, 21, 27, 128, 136), g3(2, 21, 27, 256, 264, 1)]
WGRAD_HALO_GEOMS = [g3(*s) for s in ((1, 5, 7, 32, 32), (2, 14, 14, 64, 64), (1, 13, 17, 128, 136), (1, 1, 1, 32, 32), (1, 1, 9, 64, 40))]
WGRAD_STREAM_GEOMS = [g3(1, 1, 1, 64, 256, 1), g3(1, 19, 17, 264, 520, 1), g3(2, 33, 21, 256, 40, 1), g3(1, 37, 29, 64, 256, 1)]
FUSED_GEOMS = [g3(1, 1, 1, 64, 256, 1), g3(2, 37, 41, 64, 256, 1), g3(2, 37, 41, 40, 200, 1), g3(1, 1, 1, 128, 512, 1),
               g3(2, 37, 41, 128, 512, 1), g3(2, 37, 41, 72, 264, 1)]
ALL_CONV_GEOMS = (VARIANT_SHAPES + GENERIC_GEOMS + [ASYM_GEOM] + STRIDE2_GEOMS + HALO_GEOMS + STREAM_GEOMS + ACC_GEOMS + LONGK_GEOMS
                  + [FC_GEOM] + WGRAD_TAP_GEOMS + WGRAD_HALO_GEOMS + WGRAD_STREAM_GEOMS + FUSED_GEOMS)
