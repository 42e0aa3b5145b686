"""Float64 reference helpers of tests/test_gpu_optim_resample_float64.py, tests/test_gpu_conv_float64.py,
tests/test_gpu_inference_tails_float64.py, tests/test_gpu_box_decisions_float64.py, tests/test_gpu_kmeans_update_float64.py,
tests/test_gpu_kmeans_assign_float64.py, tests/test_gpu_topk_rows.py and (the streaming kernels' launch geometry) tests/test_gpu_tail_bwd_fused.py, in a plain module so that the CPU tests of
tests/test_float64_refs_host.py check exactly what the GPU tests use.  Plain torch ops only; nothing here touches the HIP
library.  Every function works on whatever device its inputs live on."""
import math

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


def conv_operands(geom, mode, amp=None, forward_only=False):
    """Operands of one convolution case as float64 tensors whose values are bf16 numbers: x [B, Cin, H, W], w [N, Cin, KH, KW],
    bias [N], gy [B, N, Ho, Wo], old [B, N, Ho, Wo] (the accumulating epilogue's stored values; gy and old are None with
    forward_only, for the cases whose outputs are large: x, w and bias are the same either way).
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
        bias = ints((cout,), 16 * a_f, g)
        if forward_only:
            return x, w, bias, None, None
        old = ints((b, cout, ho, wo), 16 * a_f, g)
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
    if forward_only:
        return tuple(bf16_round(t) for t in (x, w, bias)) + (None, None)
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

# (TM pixels per tile, waves along the pixels, waves per work-group) of the three tail instantiations, by reduction width C
TAIL_CFG = {64: (128, 1, 4), 128: (64, 1, 4), 256: (64, 2, 8)}


def stream_cfg(c, n, tail=False):
    """(TM, PSW, NWV, KSS) of the instantiation launch_conv_stream / launch_conv_stream_tail pick for C input and N output
    channels; KSS: 32-channel slabs per ring step (a tile of C = 32 KS channels arrives in KS / KSS steps)."""
    if tail:
        assert (c, n) in ((64, 256), (128, 512), (256, 1024)), "launch_conv_stream_tail serves these three"
        return TAIL_CFG[c] + (c // 32,)
    psw = 1 if n > 128 else 2 if n > 64 else 4
    if c == 256:
        return (64, 2, 8, 8) if n > 128 else (64, psw, 4, 4)
    return {32: 128, 64: 128, 128: 64}[c], psw, 4, c // 32


def stream_geometry(c, n, m, tiny, tail=False):
    """launch_stream_cfg and the first lines of conv_stream_kernel, restated: the ring depth, the grid and the pixel tiles every
    work-group of one channel block walks.  XCD x (work-groups x, x + 8, ...) owns a contiguous range of xcnt pixel tiles; its
    work-groups are (walker, channel block) pairs and the nwalk walkers of a channel block take the range's tiles round robin
    (walker k: tiles k, k + nwalk, ...); walkers beyond the range return at once.  my_tiles[xcd][walker] is 0 for those.
    tiny: the 8-work-groups-per-channel-block grid of CV_TINY_GRID; otherwise 256 work-groups per resident group of a CU."""
    tm, psw, nwv, kss = stream_cfg(c, n, tail)
    stage = tm * kss * 64
    per_cu = 2 if nwv == 4 else 1
    ring = min(8, (80 if per_cu == 2 else 160) * 1024 // stage)
    tiles_m = -(-m // tm)
    tiles_n = -(-n // (nwv // psw * 64))
    grid = 8 * tiles_n if tiny else 256 * per_cu
    assert ring >= 2 and grid // 8 >= tiles_n, "the launcher declines"
    nwalk = grid // 8 // tiles_n
    q8, r8 = divmod(tiles_m, 8)
    xcnt = [q8 + (x < r8) for x in range(8)]
    xbase = [x * (q8 + 1) if x < r8 else r8 * (q8 + 1) + (x - r8) * q8 for x in range(8)]
    my_tiles = [[(xcnt[x] - k + nwalk - 1) // nwalk if k < xcnt[x] else 0 for k in range(nwalk)] for x in range(8)]
    return dict(TM=tm, PSW=psw, NWV=nwv, steps_per_tile=c // 32 // kss, ring=ring, tiles_m=tiles_m, tiles_n=tiles_n, grid=grid,
                nwalk=nwalk, xcnt=xcnt, xbase=xbase, my_tiles=my_tiles,
                served_unforced=None if tiny else tiles_m * tiles_n >= 6 * grid)   # (the fill rule is not applied to the tiny grid)


def walker_tiles(geo):
    """The tile counts of the work-groups that have work, as a sorted list of the distinct values."""
    return sorted({t for row in geo["my_tiles"] for t in row if t > 0})


def stream_stats_depth(geo):
    """Longest chain of fp32 additions behind one column sum of the streaming kernel's epilogues, from its launch geometry: a
    lane's running sum over the NF rows it holds of a tile, the 16-row transposing sum (4), one addition per tile of the
    work-group into the lane's total (the busiest walker's count), the work-group flush over its waves, one atomicAdd per
    work-group of the channel block."""
    nf = geo["TM"] // geo["PSW"] // 16
    return nf + 4 + max(walker_tiles(geo)) + geo["NWV"] + 8 * geo["nwalk"]


def tail_depth(c, n, m, tiny):
    """Longest chain of fp32 additions behind one column sum of the TAIL epilogue (launch_stream_cfg / conv_stream_kernel):
    a lane's running sum over the NF rows it holds of a tile, the 16-row transposing sum (4), one addition per tile of the
    work-group into the lane's total (the busiest walker's count, from stream_geometry), the work-group flush over its waves,
    one atomicAdd per work-group of the channel block."""
    return stream_stats_depth(stream_geometry(c, n, m, tiny, tail=True))


def stream_steady_pixels(cin, cout):
    """The smallest pixel count at which the production grid of the plain streaming kernel is in steady state with uneven shares:
    some walker owns ring + 2 tiles, another ring + 1, the XCDs' ranges differ in length and the last tile is ragged (one row)."""
    tm = stream_cfg(cin, cout)[0]
    geo = stream_geometry(cin, cout, 1, False)
    tp = 8 * (geo["ring"] + 1) * geo["nwalk"] + 1   # the longest range, ceil(tp / 8) tiles, must give its first walker ring + 2
    while True:
        geo = stream_geometry(cin, cout, (tp - 1) * tm + 1, False)
        counts = walker_tiles(geo)
        if counts[-1] >= geo["ring"] + 2 and geo["ring"] + 1 in counts and tp % 8:
            return (tp - 1) * tm + 1
        tp += 1


# the plain streaming kernel on its production grid (CV_STREAM_FORCE alone): one cout with several channel blocks, one with one.
# Not part of ALL_CONV_GEOMS: the host-side consumers of that list need no tensors of this size.
STREAM_PROD_COUT = [520, 40]
STREAM_PROD_GEOMS = [g3(1, 1, stream_steady_pixels(cin, cout), cin, cout, 1) for cin in STREAM_CIN for cout in STREAM_PROD_COUT]
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


# ---- inference tails (tests/test_gpu_inference_tails_float64.py) ----
def _paste_axis(n_pix, lo, hi, p):
    """Source coordinate of every pixel centre along one axis, [n_masks, n_pix]: the normalised grid value of
    layers/mask_ops.py (pixel centre mapped so that the box spans [-1, 1]) and grid_sample's unnormalisation with
    align_corners=False, ((g + 1) P - 1) / 2."""
    pix = torch.arange(n_pix, dtype=F64) + 0.5
    g = (pix[None] - lo[:, None]) / (hi - lo)[:, None] * 2 - 1
    return ((g + 1) * p - 1) / 2


def _paste_taps(coord, p):
    """[n, L] source coordinates -> [n, L, p] bilinear weights of the p texels; a tap outside the map has no column: zeros padding."""
    i0 = torch.floor(coord)
    w1 = coord - i0
    j = torch.arange(p, dtype=F64)
    return (1 - w1)[..., None] * (j == i0[..., None]).to(F64) + w1[..., None] * (j == i0[..., None] + 1).to(F64)


def paste_ref(probs, boxes, h, w):
    """layers/mask_ops.py:17-147 before the threshold, in float64: the P x P maps probs [n, P, P] sampled over boxes [n, 4]
    (x0, y0, x1, y1) by grid_sample(bilinear, align_corners=False, zeros padding) at the centres of an h x w canvas.
    Returns (v [n, h, w] float64, inside [n, h, w] bool); `inside`: the sample point lies less than one texel outside the map on
    both axes (-1 < coordinate < P) - everywhere else all four taps are padding and the value is an exact 0."""
    probs, boxes = probs.to(F64).cpu(), boxes.to(F64).cpu()
    p = probs.shape[-1]
    ix = _paste_axis(w, boxes[:, 0], boxes[:, 2], p)
    iy = _paste_axis(h, boxes[:, 1], boxes[:, 3], p)
    v = torch.einsum("nyi,nij,nxj->nyx", _paste_taps(iy, p), probs, _paste_taps(ix, p))
    inside = ((iy > -1) & (iy < p))[:, :, None] & ((ix > -1) & (ix < p))[:, None, :]
    return v, inside


def paste_fp32(probs, boxes, h, w):
    """The reference's own fp32 form of the same (mask_ops.py's grid + F.grid_sample on the CPU), before the threshold:
    what the margins of the random-input paste test are measured with."""
    probs, boxes = probs.float().cpu(), boxes.float().cpu()
    n = probs.shape[0]
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    img_y = (torch.arange(0, h, dtype=torch.float32) + 0.5 - y0) / (y1 - y0) * 2 - 1
    img_x = (torch.arange(0, w, dtype=torch.float32) + 0.5 - x0) / (x1 - x0) * 2 - 1
    grid = torch.stack([img_x[:, None, :].expand(n, h, w), img_y[:, :, None].expand(n, h, w)], dim=3)
    return TF.grid_sample(probs[:, None], grid, align_corners=False)[:, 0]


PASTE_P = [1, 2, 7, 14, 28]
PASTE_CANVASES = [(45, 53), (5, 3), (1, 1), (9, 8), (16, 64)]
PASTE_HALF, PASTE_BELOW = 6, 7   # maps of paste_exact_case that are constant 0.5 / constant 0.5 - 1/256


def paste_exact_case(p, h, w):
    """Exact inputs of the paste on an h x w canvas: 13 boxes (x0, y0, x1, y1) whose sides are powers of two (1/4 .. 32) and whose
    corners are multiples of 1/4, and maps whose values are multiples of 1/256.  Every source coordinate is then a multiple of
    2^-7, every bilinear weight product one of 2^-14 and every term one of 2^-22 below 1: the sampled value is an fp32 number
    in whatever order it is formed (the tests assert it).  13 masks: 13 h w is no multiple of 16 unless h w is.
    Map PASTE_HALF is constant 0.5 (interior pixels sit exactly on the 0.5 threshold), map PASTE_BELOW constant 0.5 - 1/256."""
    g = torch.Generator().manual_seed(1000 * p + 10 * h + w)
    q = lambda v: float(int(v * 4)) / 4    # noqa: E731
    xywh = [
        (-40.25, 0.0, 32, 8),                 # 0 wholly left of the canvas (with P = 1 its reach still comes back in)
        (w + 8.5, 1.0, 16, 4),                # 1 wholly right
        (0.0, -20.75, 8, 16),                 # 2 wholly above
        (2.0, h + 4.25, 4, 2),                # 3 wholly below
        (-3.25, -2.5, 8, 4),                  # 4 partly off, top left
        (w - 2.75, h - 1.5, 4, 8),            # 5 partly off, bottom right
        (q((w - 32) / 2), q((h - 32) / 2), 32, 32),   # 6 covers the canvas (or its middle): constant 0.5
        (q((w - 16) / 2) + 0.25, q((h - 8) / 2) - 0.25, 16, 8),   # 7 constant 0.5 - 1/256
        (q(w / 2) + 0.25, q(h / 2) + 0.25, 0.5, 0.25),   # 8 smaller than a pixel, covers no pixel centre
        (q(w / 3) + 0.25, q(h / 3) + 0.25, 1, 1),        # 9 one pixel wide, across four pixels
        (4.25, 1.0, 32, 1),                   # 10 32 wide, 1 high: the widest reach past the box with P = 1, 2
        (0.0, 0.0, 1, 32),                    # 11 1 wide, 32 high, at the origin
        (w - 32.0, h - 32.0, 32, 32),         # 12 ends exactly at the canvas corner
    ]
    boxes = torch.tensor([[x, y, x + bw, y + bh] for x, y, bw, bh in xywh], dtype=torch.float32)
    n = boxes.shape[0]
    probs = torch.randint(0, 257, (n, p, p), generator=g).float() / 256
    probs[PASTE_HALF] = 0.5
    probs[PASTE_BELOW] = 0.5 - 1.0 / 256
    probs[12] = (torch.randint(0, 2, (p, p), generator=g) * 256).float() / 256   # 0 / 1 checker noise
    return probs, boxes


def paste_random_case(p, h, w, n, seed):
    """Random fp32 inputs of the paste: n smooth maps (a sigmoid blob each) and n salt-and-pepper maps (uniform noise), boxes
    with arbitrary fp32 corners, some reaching past the canvas."""
    g = torch.Generator().manual_seed(seed)
    lin = torch.linspace(-1, 1, p) if p > 1 else torch.zeros(1)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    cx, cy = torch.rand(n, generator=g) - 0.5, torch.rand(n, generator=g) - 0.5
    rad = 0.4 + 0.5 * torch.rand(n, generator=g)
    smooth = torch.sigmoid(6 * (rad[:, None, None] - ((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2).sqrt()))
    probs = torch.cat([smooth, torch.rand((n, p, p), generator=g)]).float()
    x0 = torch.rand(2 * n, generator=g) * (w + 6) - 6
    y0 = torch.rand(2 * n, generator=g) * (h + 6) - 6
    bw = 0.3 + torch.rand(2 * n, generator=g) * 1.2 * w
    bh = 0.3 + torch.rand(2 * n, generator=g) * 1.2 * h
    return probs, torch.stack([x0, y0, x0 + bw, y0 + bh], dim=1).float()


def _source_index(n_out, n_in, scale):
    """ATen's area_pixel_compute_source_index (align_corners=False) and guard_index_and_lambda along one axis:
    src = max(scale (dst + 0.5) - 0.5, 0); i0 = min(floor(src), n_in - 1); i1 = i0 + (i0 < n_in - 1); lambda = src - i0 in [0, 1]."""
    src = (float(scale) * (torch.arange(n_out, dtype=F64) + 0.5) - 0.5).clamp(min=0)
    i0 = torch.floor(src).clamp(max=n_in - 1)
    lam = (src - i0).clamp(0, 1)
    i0 = i0.long()
    return i0, i0 + (i0 < n_in - 1).long(), lam


def _bilinear(x, ys, xs):
    """x [..., H, W] float64; value = h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11), ATen's upsample_bilinear2d."""
    (y0, y1, ly), (x0, x1, lx) = ys, xs
    row = lambda r: (1 - lx) * r[..., x0] + lx * r[..., x1]   # noqa: E731
    return (1 - ly)[:, None] * row(x[..., y0, :]) + ly[:, None] * row(x[..., y1, :])


def upsample_ref(x, k, s):
    """F.interpolate(logits, scale_factor=s, mode="bilinear", align_corners=False) of the first k channels of an NHWC map
    x [B, H, W, Cp] in float64 (scale = 1 / s): [B, k, H s, W s]."""
    x = x[..., :k].to(F64).cpu().permute(0, 3, 1, 2)
    h, w = x.shape[2], x.shape[3]
    return _bilinear(x, _source_index(h * s, h, 1.0 / s), _source_index(w * s, w, 1.0 / s))


def resize_ref(x, hout, wout):
    """F.interpolate(x, size=(hout, wout), mode="bilinear", align_corners=False) of x [C, Hin, Win]: the scale as ATen forms it
    for fp32 maps - the fp32 quotient in / out - everything after it in float64."""
    x = x.to(F64).cpu()
    hin, win = x.shape[1], x.shape[2]
    sc = lambda a, b: float(torch.tensor(float(a), dtype=torch.float32) / torch.tensor(float(b), dtype=torch.float32))   # noqa: E731
    return _bilinear(x, _source_index(hout, hin, sc(hin, hout)), _source_index(wout, win, sc(win, wout)))


def first_argmax(v, dim=1):
    """Index of the first maximum along dim, written as a count: the number of entries before the first one equal to the maximum."""
    is_max = v == v.max(dim=dim, keepdim=True).values
    return (is_max.long().cumsum(dim) == 0).long().sum(dim)


SEM_EXACT_CASES = [(1, 8), (7, 8), (8, 8), (9, 32), (28, 32), (54, 64), (64, 64), (7, 32), (1, 64)]   # (K, Cp)
SEM_MAPS = [(1, 1), (1, 5), (7, 1), (3, 5)]


def upsample_exact_case(b, h, w, cp, k, pad):
    """Exact inputs of the semantic upsample: bf16 multiples of 1/4 with |v| <= 32 in channels [0, k); with s in {2, 4} the
    interpolation weights are multiples of 1/8, every product and sum a multiple of 2^-8 below 64: fp32 numbers, in any order.
    Built-in ties: the last channel copies channel k // 2 and both are raised by 16 on every other pixel of all images but the
    last (two identical, mostly maximal channels: the lower index must win); all channels of the first image's top-left 2 x 2 pixels are equal (index 0 must win);
    the last image is negative everywhere.  Pad channels [k, cp) hold `pad` (1e30 or NaN): they must influence nothing.
    Returns NHWC float64 holding bf16 values (pad channels included)."""
    g = torch.Generator().manual_seed(b * 100000 + h * 10000 + w * 1000 + cp * 10 + k)
    x = torch.randint(-64, 65, (b, h, w, cp), generator=g).to(F64) / 4     # |v| <= 16
    x[b - 1] = -x[b - 1].abs() - 0.25                                        # the last image: every value negative
    if k > 1:
        lo = k // 2 if k > 2 else 0
        checker = ((torch.arange(h)[:, None] + torch.arange(w)[None]) % 2 == 0).to(F64)
        x[: b - 1, :, :, lo] += 16 * checker                                 # (not in the negative image)
        x[..., k - 1] = x[..., lo]
    x[0, :2, :2, :k] = x[0, 0, 0, 0].item()
    x[..., k:] = pad
    return x


def mask_prob_ref(x, w, b, cls):
    """mask_rcnn_inference (roi_heads/mask_head.py:115-158) on the predicted class's channel only: the exact dot product of the
    bf16-rounded operands in float64, the logit rounded to bf16 as the predictor conv's output is, float64 sigmoid.
    x [N, S, S, C] (bf16 values), w [K, C] or [K, C, 1, 1], b [K], cls [N] -> (prob [N, 1, S, S], rounded logit z [N, 1, S, S])."""
    x = x.to(F64).cpu()
    wq = bf16_round(w.detach().cpu().reshape(w.shape[0], -1))[cls.cpu().long()]   # [N, C]
    bq = bf16_round(b.detach().cpu())[cls.cpu().long()]
    z = rne_bf16(torch.einsum("nyxc,nc->nyx", x, wq) + bq.view(-1, 1, 1))[:, None]
    return torch.sigmoid(z), z


MASK_PROB_Q = 2.0 ** -8   # quantum of the exact mask-predictor case: weights and bias are integers times this


def mask_prob_case(n, side, c, k, seed=0):
    """Exact inputs of the folded mask predictor: x integers in [-ax, ax] (bf16 values), weights and bias integers (|.| <= 255, so
    bf16 values) times 2^-8.  Every product and partial sum is an integer times 2^-8 of magnitude at most
    (c ax aw + 255) 2^-8 < 2^24 2^-8 - an fp32 number in any order - so the fp32 logit is the exact sum and its bf16 rounding is
    unique (ties to even on exact halves).  Amplitudes put the logits' standard deviation near 2.5: most |z| lie in [1, 8], where
    bf16 has fewer than 8 fractional bits - z in [1, 2) odd multiples of 2^-8 are exact halves, [2, 8) rounds properly.
    Selected classes: the first and the last of the k, the rest random.  Returns (x [n, side, side, c] float64, w [k, c] fp32,
    b [k] fp32, cls [n] int64, ax, aw)."""
    g = torch.Generator().manual_seed(seed + 7919 * n + 104729 * side + 31 * c + k)
    for ax in (8, 2):
        aw = round((6.25 * 65536 * 9 / (c * ax * (ax + 1))) ** 0.5)
        if aw <= 255:
            break
    aw = max(1, min(aw, 255))
    x = ints((n, side, side, c), ax, g)
    w = (ints((k, c), aw, g) * MASK_PROB_Q).float()
    b = (ints((k,), 255, g) * MASK_PROB_Q).float()
    cls = torch.randint(0, k, (n,), generator=g)
    cls[0] = 0
    cls[-1] = k - 1
    return x, w, b, cls, ax, aw


# ---- box decisions (tests/test_gpu_box_decisions_float64.py) ----
def _inter_union(a, b):
    """Areas of intersection and union of every pair, [len(a), len(b)] float64 (structures/boxes.py:312-358)."""
    a, b = a.to(F64).cpu(), b.to(F64).cpu()
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    h = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = w * h
    return inter, area_a[:, None] + area_b[None, :] - inter


def iou_ref(gt, cand):
    """pairwise_iou (structures/boxes.py:312-358), [G, n], formed in float64 and rounded once to fp32; 0 where the boxes do not
    intersect.

    Exactness for integer coordinates below 2^11: every side is an integer below 2^11, every area, intersection and union an
    integer below 2^23 - all fp32 numbers, whatever the order of the subtractions and the one product, so an fp32 routine
    divides the exact integers `inter` and `union` and, dividing correctly rounded, returns RN32(inter / union).  Here the
    quotient of the same two integers is rounded to float64 first and then to fp32; for a quotient of two p-bit numbers a
    first rounding to q >= 2 p + 2 bits cannot change the second (the quotient is no midpoint of two p-bit numbers, and it
    lies no nearer to one than 2^-(2p+1) relative), and 53 >= 2 * 24 + 2.  So float32(float64(inter) / float64(union)) IS the
    value a correct fp32 routine returns, bit for bit: an approximate division is a failure, not a tolerance question."""
    inter, union = _inter_union(gt, cand)
    return torch.where(inter > 0, inter / union, torch.zeros((), dtype=F64)).float()


def match_ref(gt, cand, lo, hi, allow_low_quality):
    """Matcher (modeling/matcher.py:62-127) with thresholds [lo, hi] and labels [0, -1, 1] on iou_ref(gt, cand), for one image.
    Returns (match [n] int64: the FIRST ground truth attaining the candidate's maximum; labels [n] int8: v < lo -> 0, v < hi -> -1,
    else 1, v the fp32 maximum and lo, hi rounded to fp32 as the kernel receives them; mval [n] fp32).  Low-quality matches as the
    reference has them: every candidate whose IoU with a ground truth EQUALS that ground truth's maximum over the candidates is
    positive - so a ground truth that overlaps nothing (maximum 0) makes every candidate it does not overlap positive.
    No ground truth: match 0, label 0, value 0."""
    n = cand.shape[0]
    if gt.shape[0] == 0:
        return torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int8), torch.zeros(n, dtype=torch.float32)
    iou = iou_ref(gt, cand)
    mval = iou.max(dim=0).values
    rows = torch.arange(gt.shape[0])[:, None].expand_as(iou)
    match = torch.where(iou == mval[None], rows, torch.full_like(rows, gt.shape[0])).min(dim=0).values
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    labels = torch.where(mval < lo32, 0, torch.where(mval < hi32, -1, 1)).to(torch.int8)
    if allow_low_quality:
        best = iou.max(dim=1).values
        labels[(iou == best[:, None]).any(dim=0)] = 1
    return match, labels, mval


def nms_iou_ref(boxes):
    """The IoU the NMS decides on (torchvision's nms, layers/nms.py:5-20): inter / union without the `inter > 0` guard of
    pairwise_iou, so two zero-area boxes give 0 / 0 = NaN, which is not greater than any threshold.  float64, rounded to fp32
    (iou_ref's argument)."""
    inter, union = _inter_union(boxes, boxes)
    return (inter / union).float()


def nms_ref(boxes_sorted, groups, thr, max_keep):
    """Greedy NMS within groups (layers/nms.py:5-20) over boxes already sorted by descending score: the positions kept, in order,
    at most max_keep.  A later box of the same group is suppressed when RN32(iou) > float32(thr).
    Only for thresholds whose fp32 value is at or below the decimal - 0.5 (exact), 0.65 (fp32 0.64999998), 0.7 (0.69999999):
    then no RN32(iou) lies between the double and the fp32 threshold, and a routine comparing in either precision decides alike.
    0.3 (fp32 0.30000001) is no such threshold: an IoU of exactly 3/10 rounds to that fp32 number, which exceeds the double 0.3."""
    n = boxes_sorted.shape[0]
    iou = nms_iou_ref(boxes_sorted)
    groups = groups.cpu().long()
    thr32 = torch.tensor(thr, dtype=torch.float32)
    assert float(thr32) <= thr, "threshold outside the contract of nms_ref"
    dead = torch.zeros(n, dtype=torch.bool)
    later = torch.arange(n)
    keep = []
    for i in range(n):
        if len(keep) >= max_keep:
            break
        if dead[i]:
            continue
        keep.append(i)
        dead |= (iou[i] > thr32) & (groups == groups[i]) & (later > i)
    return keep


def levels_ref(boxes, min_level, max_level, canonical_size=224, canonical_level=4):
    """assign_boxes_to_levels (modeling/poolers.py:23-59) in float64: floor(canonical_level + log2(sqrt(area) / canonical_size
    + 1e-8)) clamped to [min_level, max_level], minus min_level.

    Boundaries.  A box with sqrt(area) = 224 * 2^k lands on the upper side: in float64 the 1e-8 lifts the logarithm just above
    k.  In fp32 area and its root are exact, s / 224 = 2^k exactly, and 1e-8 (2^-26.6) is below half an ulp of 2^k for k >= -2
    (ulp 2^(k-23), half of it >= 2^-26 = 1.49e-8), so the sum rounds back to 2^k, whose log2 is k exactly: floor(4 + k) = 4 + k
    as well.  For s = 28 (k = -3, half an ulp 7.5e-9) the sum rounds one ulp up and the logarithm stays at or just above -3:
    level 1 either way."""
    b = boxes.to(F64).cpu()
    s = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).sqrt()
    lv = torch.floor(canonical_level + torch.log2(s / canonical_size + 1e-8))
    return lv.clamp(min_level, max_level).long() - min_level


def apply_deltas_ref(src, deltas, weights, clamp, sizes=None, img=None):
    """Box2BoxTransform.apply_deltas (modeling/box_regression.py:78-116) and, with `sizes` [n_images, 2] (h, w), Boxes.clip
    (structures/boxes.py:172-181) to the size of image img[i] (image 0 without `img`), in float64.  `clamp` is an operand the
    fp32 operation holds in fp32 (the reference clamps an fp32 tensor with it), so it is rounded to fp32 first.  torch.clamp
    keeps NaN, so a NaN delta gives NaN corners; the clip keeps NaN too.  Returns (unclipped [n, 4], clipped [n, 4] or None)."""
    s, d = src.to(F64).cpu(), deltas.to(F64).cpu()
    clamp = float(torch.tensor(clamp, dtype=torch.float32))
    w, h = s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
    cx, cy = s[:, 0] + 0.5 * w, s[:, 1] + 0.5 * h
    dx, dy = d[:, 0] / weights[0], d[:, 1] / weights[1]
    dw, dh = torch.clamp(d[:, 2] / weights[2], max=clamp), torch.clamp(d[:, 3] / weights[3], max=clamp)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    raw = torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1)
    if sizes is None:
        return raw, None
    sz = sizes.to(F64).cpu()
    sz = sz[img.cpu().long()] if img is not None else sz[:1].expand(raw.shape[0], 2)
    hi = torch.stack([sz[:, 1], sz[:, 0], sz[:, 1], sz[:, 0]], dim=1)
    return raw, torch.minimum(torch.clamp(raw, min=0), hi)


def _crop_axis(lo, hi, p, size):
    """One axis of the ROIAlign behind crop_and_resize: [p, size] float64, row b the summed bilinear weights on the `size` pixels of
    the g = ceil((hi - lo) / p) samples of bin b, and g.  aligned=True: the ROI is shifted by -0.5; sample i of bin b sits at
    lo - 0.5 + b bin + (i + 0.5) bin / g; a sample outside [-1, size] contributes nothing (but counts); otherwise it is clamped
    to [0, size - 1] and split between floor and floor + 1."""
    lo, hi = float(lo) - 0.5, float(hi) - 0.5
    bin_ = (hi - lo) / p
    g = int(math.ceil((hi - lo) / p))
    out = torch.zeros((p, size), dtype=F64)
    for b in range(p):
        for i in range(max(g, 0)):
            c = lo + b * bin_ + (i + 0.5) * bin_ / g
            if c < -1.0 or c > size:
                continue
            c = max(c, 0.0)
            low = int(c)
            if low >= size - 1:
                out[b, size - 1] += 1.0
            else:
                out[b, low] += 1.0 - (c - low)
                out[b, low + 1] += c - low
    return out, g


def mask_crop_ref(masks, rois, p):
    """BitMasks.crop_and_resize (structures/masks.py:191-218) before the decision, in float64: ROIAlign(p, scale 1, sampling
    ratio 0, aligned) of mask rois[r, 0] inside box rois[r, 1:5] = (x1, y1, x2, y2).  The sampling grid has ceil(roi side / p)
    points per bin and axis, the average divides by max(gh gw, 1) whether or not a sample fell outside, and an ROI without
    extent has no samples: 0.  Returns [R, p, p] float64 averages; the target is `>= 0.5`."""
    m = masks.to(F64).cpu()
    r_ = rois.to(F64).cpu()
    out = torch.zeros((r_.shape[0], p, p), dtype=F64)
    for r in range(r_.shape[0]):
        wy, gh = _crop_axis(r_[r, 2], r_[r, 4], p, m.shape[1])
        wx, gw = _crop_axis(r_[r, 1], r_[r, 3], p, m.shape[2])
        if gh > 0 and gw > 0:
            out[r] = wy @ m[int(r_[r, 0])] @ wx.t() / (gh * gw)
    return out


# one ground truth and candidates whose IoU with it is exactly 1/2, 3/10, 7/10, 1, 0, 2/10, 4/10, 6/10, 8/10 and 0 (touching)
EDGE_GT = torch.tensor([[0.0, 0.0, 10.0, 10.0]])
EDGE_CAND = torch.tensor([[0.0, 0.0, 10.0, 5.0], [0.0, 0.0, 10.0, 3.0], [0.0, 0.0, 10.0, 7.0], [0.0, 0.0, 10.0, 10.0], [20.0, 20.0, 30.0, 30.0],
                          [0.0, 0.0, 10.0, 2.0], [0.0, 0.0, 10.0, 4.0], [0.0, 0.0, 10.0, 6.0], [0.0, 0.0, 10.0, 8.0], [10.0, 0.0, 20.0, 10.0]])
BOX_BIG = [0.0, 0.0, 2047.0, 2047.0]   # overlaps every box of the integer cases: what a padding row must not be read as


def int_boxes(n, g, span=96, side=64, min_side=1):
    """n random boxes with integer corners in [0, span + side], sides min_side .. side: overlaps, equal IoUs and exact ties are
    common."""
    xy = torch.randint(0, span, (n, 2), generator=g)
    wh = torch.randint(min_side, side + 1, (n, 2), generator=g)
    return torch.cat([xy, xy + wh], dim=1).float()


def level_boundary_boxes():
    """Boxes whose sqrt(area) is exactly s in {28, 56, 112, 224, 448, 896} - square, s/2 x 2 s and s/4 x 4 s, e.g. 56 x 224 -, squares
    of side s (1 + 2^-10) and s (1 - 2^-10) (fp32 numbers; 2^-10 moves the logarithm by 1.4e-3, far beyond fp32 error), and two
    boxes without area.  Origins are small integers, so every corner is an fp32 number.  [44, 4] fp32."""
    rows = []
    for i, s in enumerate((28.0, 56.0, 112.0, 224.0, 448.0, 896.0)):
        x, y = 3.0 + i, 5.0 + 2 * i
        for w, h in ((s, s), (s / 2, 2 * s), (4 * s, s / 4), (s * (1 + 2.0 ** -10), s * (1 + 2.0 ** -10)),
                     (s * (1 - 2.0 ** -10), s * (1 - 2.0 ** -10)), (s * (1 + 2.0 ** -10), s), (s, s * (1 - 2.0 ** -10))):
            rows.append([x, y, x + w, y + h])
    rows += [[5.0, 5.0, 5.0, 9.0], [7.0, 7.0, 7.0, 7.0]]
    b = torch.tensor(rows, dtype=F64)
    assert torch.equal(b, b.float().to(F64))
    return b.float()


def _grid_boxes(n, x0=0, y0=400, per_row=30, pitch=20, side=10):
    """n disjoint side x side boxes on a grid (they do not even touch)."""
    i = torch.arange(n)
    x, y = x0 + (i % per_row) * pitch, y0 + (i // per_row) * pitch
    return torch.stack([x, y, x + side, y + side], dim=1).float()


def nms_ladder(n, lead=0):
    """`lead` isolated boxes, then a one-dimensional ladder of 10 x 10 boxes shifted by 3: neighbours have IoU 7/13 > 0.5, second
    neighbours 4/16 - every second box of the ladder survives at 0.5, and which parity does flips with `lead`."""
    b = torch.zeros((n, 4))
    for i in range(n):
        b[i] = torch.tensor([3.0 * i, 0.0, 3.0 * i + 10, 10.0]) if i >= lead else torch.tensor([20.0 * i, 100.0, 20.0 * i + 10, 110.0])
    return b


def _victims(x, y):
    """Eleven boxes that each overlap A = (x, y, x + 100, y + 100) with IoU > 0.5 and one another with IoU <= 0.5 (asserted by the
    host test): A grown by 90 to one side (IoU 100/190) four times, A grown by 20 all round (100^2 / 140^2), 51 % strips of A at
    its four sides and through its middle both ways."""
    a = [x, y, x + 100, y + 100]
    out = [[x - 90, y, x + 100, y + 100], [x, y, x + 190, y + 100], [x, y - 90, x + 100, y + 100], [x, y, x + 100, y + 190],
           [x - 20, y - 20, x + 120, y + 120],
           [x, y, x + 51, y + 100], [x + 49, y, x + 100, y + 100], [x, y, x + 100, y + 51], [x, y + 49, x + 100, y + 100],
           [x + 24, y, x + 75, y + 100], [x, y + 24, x + 100, y + 75]]
    return torch.tensor(a, dtype=torch.float32), torch.tensor(out, dtype=torch.float32)


def nms_lazy_column_case():
    """300 boxes, threshold 0.5, one group.  A background of disjoint boxes, and two plots:
    - position 3 holds A; its only victims sit at 130 .. 140 (eleven boxes that do not suppress one another) and at 200 (a copy
      of the box at 130): a box kept in block 0 whose suppression row matters in block 2 and block 3 only;
    - position 4 holds a strip that covers 56 % of a second box A' at position 5, so A' is suppressed; 150 .. 155 hold six boxes
      that A' would suppress and the strip does not: they must all survive.
    Returns (boxes [300, 4], expected suppressed positions)."""
    b = _grid_boxes(300)
    a, v = _victims(100, 100)
    b[3] = a
    b[130:141] = v
    b[200] = v[0]
    a2, v2 = _victims(500, 100)
    b[4] = torch.tensor([500.0, 122.0, 600.0, 178.0])
    b[5] = a2
    b[150:156] = v2[torch.tensor([0, 1, 2, 3, 5, 6])]
    return b, list(range(130, 141)) + [200, 5]


def nms_helper_stride_case():
    """400 boxes (seven blocks), threshold 0.5, all disjoint except that position 390 (block 6) overlaps the box at position 200
    and position 395 the box at position 5 (IoU 7/13 each).  Every earlier box is kept, so 200 is also the 201st entry of the
    kept list: while block 5 is resolved, the 192 helper threads gather the rows of the 320 boxes kept before it for block 6's
    column, and entry 200 is reached only by a thread's second stride.  (With n = 300 no helper ever takes a second stride: the
    last column is gathered when 192 boxes are kept.)  Returns (boxes [400, 4], suppressed positions)."""
    b = _grid_boxes(400)
    b[390] = b[200] + torch.tensor([3.0, 0.0, 3.0, 0.0])
    b[395] = b[5] + torch.tensor([3.0, 0.0, 3.0, 0.0])
    return b, [390, 395]


NMS_EDGE_PAIRS = {0.5: ((10, 5), (10, 6)), 0.7: ((10, 7), (10, 8)), 0.65: ((20, 13), (20, 14))}


def nms_threshold_pairs(thr):
    """Four boxes: a square of side s and an s x k part of it with IoU k / s EXACTLY the threshold (1/2, 7/10, 13/20: not suppressed,
    RN32(k / s) equals the fp32 threshold), then, 100 further right, the same square and a part one pixel taller (suppressed)."""
    (s, k), (_, k1) = NMS_EDGE_PAIRS[thr]
    return torch.tensor([[0, 0, s, s], [0, 0, s, k], [100, 0, 100 + s, s], [100, 0, 100 + s, k1]], dtype=torch.float32)


CROP_H, CROP_W, CROP_MASKS = 100, 104, 3


def mask_crop_exact_case(p, h=CROP_H, w=CROP_W, n_masks=CROP_MASKS, seed=0, per_side=None):
    """Exact inputs of the mask crop: random binary masks [n_masks, h, w] and ROIs [R, 5] (mask index, x1, y1, x2, y2) with sides in
    {p, 2 p, 3 p, 1.5 p} (1, 2, 3, 2 samples per bin and axis, spaced 1, 1, 1, 0.75) and corners that are multiples of 1/4.
    Every sample coordinate is then a multiple of 1/8 below 2^8, every bilinear weight one of 1/8, every product one of 1/64 and
    every bin sum one of 1/64 below 9: fp32 numbers in any order.  With integer corners the samples of the 2 p and 3 p ROIs sit ON
    pixel centres, so their bin averages are k/4 and k/9 (the tests assert that 1/4, 2/4, 3/4, 4/9 and 5/9 occur).
    Besides per_side inside ROIs of every side (the first half on integer corners) and 2 p x 3 p ones: ROIs hanging over each of
    the four borders, ROIs wholly outside (left / above, right / below), an ROI without extent and one without width."""
    g = torch.Generator().manual_seed(1000 * p + seed)
    if per_side is None:
        per_side = 40 if p == 1 else 10      # p = 1: one bin per ROI, so more ROIs for the same variety of averages
    masks = (torch.rand((n_masks, h, w), generator=g) < 0.5).to(torch.uint8)
    rois = []

    def rnd(limit, integer):
        v = float(torch.randint(0, max(int(limit), 0) + 1, (1,), generator=g))
        return v if integer else min(v + float(torch.randint(0, 4, (1,), generator=g)) / 4, float(limit))

    for sw_, sh_ in ((1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (1.5, 1.5), (2.0, 3.0), (1.5, 1.0)):
        rw, rh = sw_ * p, sh_ * p
        for i in range(per_side):
            integer = i < per_side // 2 and rw == int(rw) and rh == int(rh)
            x, y = rnd(w - rw, integer), rnd(h - rh, integer)
            rois.append([float(torch.randint(0, n_masks, (1,), generator=g)), x, y, x + rw, y + rh])
    s = 2.0 * p
    rois += [[0.0, -p - 0.25, 8.0, -p - 0.25 + s, 8.0 + s], [1.0, w - p + 0.25, 4.0, w - p + 0.25 + s, 4.0 + s],
             [float(n_masks - 1), 6.0, -p - 0.5, 6.0 + s, -p - 0.5 + s], [0.0, 2.0, h - p + 0.5, 2.0 + s, h - p + 0.5 + s],
             [1.0, -0.75, -0.75, -0.75 + 3 * p, -0.75 + 3 * p],
             [0.0, -3.0 * p - 5, 10.0, -p - 5.0, 10.0 + s], [1.0, 10.0, -3.0 * p - 5, 10.0 + s, -p - 5.0],
             [float(n_masks - 1), w + 3.0, h + 3.0, w + 3.0 + s, h + 3.0 + s],
             [0.0, 10.0, 10.0, 10.0, 10.0], [1.0, 10.0, 10.0, 10.0, 10.0 + s]]
    r = torch.tensor(rois, dtype=F64)
    assert torch.equal(r, r.float().to(F64)) and torch.equal(r * 4, torch.round(r * 4))
    return masks, r.float()


def mask_crop_batch_case(p=7):
    """35 images (the batched launcher takes 32 per launch: two chunks) in two sizes with two bitmaps each; images 0, 5, 31, 32 and
    34 have ROIs (the exact-input kind, a border overhang among them), the other thirty none.
    Returns (list of masks [2, h_i, w_i] uint8, rois [R, 5], roi_image [R] int32, sorted)."""
    masks, rois, img = [], [], []
    for i in range(35):
        h, w = ((40, 44), (33, 29))[i % 2]
        m, r = mask_crop_exact_case(p, h, w, 2, seed=100 + i, per_side=1)
        masks.append(m)
        if i in (0, 5, 31, 32, 34):
            rois.append(r)
            img += [i] * r.shape[0]
    return masks, torch.cat(rois), torch.tensor(img, dtype=torch.int32)


def mask_crop_random_case(seed=5, p=28, n=24, h=45, w=53):
    """Random inputs of the mask crop: four h x w bitmaps of salt-and-pepper noise (flat regions would put whole runs of bins on
    exactly 1/2 - two of four samples inside -, which is the exact-input case's business) and n ROIs with arbitrary fp32 corners,
    a few of them hanging over the borders."""
    g = torch.Generator().manual_seed(seed)
    masks = (torch.rand((4, h, w), generator=g) < 0.5).to(torch.uint8)
    x = torch.rand(n, generator=g) * (w + 4) - 4
    y = torch.rand(n, generator=g) * (h + 4) - 4
    bw = torch.minimum(2 + torch.rand(n, generator=g) * (w - 2), w + 4 - x)    # at most 4 pixels past any border: in the strip
    bh = torch.minimum(2 + torch.rand(n, generator=g) * (h - 2), h + 4 - y)    # beyond it every sample is 0 or a clamped copy
    idx = torch.randint(0, 4, (n,), generator=g).float()
    return masks, torch.stack([idx, x, y, x + bw, y + bh], dim=1).float()


def delta_random_case(n, seed, weights):
    """Random inputs of the delta decode: source boxes of 2 .. 300 pixels a side, deltas N(0, 1) x weights / 2 on the centre and
    N(0, 1) x weights on the sizes with some size deltas far above the clamp (x 3 and more of it) and some near -20 after the
    division by the weight; image index in 0 .. 2."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((n, 2), generator=g) * 600 - 50
    wh = 2 + torch.rand((n, 2), generator=g) * 298
    src = torch.cat([xy, xy + wh], dim=1).float()
    wt = torch.tensor(weights)
    d = torch.randn((n, 4), generator=g) * wt * torch.tensor([0.5, 0.5, 1.0, 1.0])
    big = torch.rand((n, 2), generator=g)
    d[:, 2:] = torch.where(big > 0.9, (4 + 10 * torch.rand((n, 2), generator=g)) * wt[2:], d[:, 2:])
    d[:, 2:] = torch.where(big < 0.1, (-20 + torch.randn((n, 2), generator=g)) * wt[2:], d[:, 2:])
    img = torch.randint(0, 3, (n,), generator=g).to(torch.int32)
    return src, d.float(), img


CASCADE_WEIGHTS = [(10.0, 10.0, 5.0, 5.0), (20.0, 20.0, 10.0, 10.0), (30.0, 30.0, 15.0, 15.0)]
SCALE_CLAMP = math.log(1000.0 / 16)
DELTA_SIZES = [[64.0, 80.0], [50.0, 77.0], [333.0, 500.0]]   # (h, w) of three images


# ----------------------------------------------------------------------------------------------------------------------------
# k-means (u2seg_amd/csrc/kmeans.hip): the M step's sums and the E step's arg-min
# ----------------------------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24       # unit roundoff of fp32


def gamma32(m):
    """gamma_m = m u / (1 - m u), u = 2^-24, elementwise in float64: fp32 summation of n terms in ANY order and association
    (atomics included) obeys |fl(sum) - sum| <= gamma_(n-1) sum |x_i| (Higham, Accuracy and Stability, section 4.2)."""
    m = torch.as_tensor(m, dtype=F64)
    return m * U24 / (1 - m * U24)


def kmeans_update_ref(x, labels, k):
    """The M step's raw material in float64: (sums [K, D] = sum of the rows of x by label, counts [K] int64,
    sum_abs [K, D] = sum of |x| by label).  A label outside [0, K) belongs to no cluster.  Sums start from +0 and rows are added to
    them (index_add_), so a cluster of -0.0 rows sums to +0 as any accumulator that starts from zero does."""
    x64 = x.to(F64)
    k, d = int(k), x.shape[1]
    ok = (labels >= 0) & (labels < k)
    idx, rows = labels[ok], x64[ok]
    sums = torch.zeros((k, d), dtype=F64, device=x.device).index_add_(0, idx, rows)
    sum_abs = torch.zeros((k, d), dtype=F64, device=x.device).index_add_(0, idx, rows.abs())
    return sums, torch.bincount(idx, minlength=k), sum_abs


def kmeans_argmin_ref(x, c, budget=1 << 26):
    """The E step in float64, difference form: d_ij = sum_d (x_id - c_jd)^2, label = torch.argmin's choice - a NaN distance beats
    every number, the first index wins among equals (spelled out as NaN -> -inf so that it holds on every device; a squared
    distance is never -inf itself).  Also the relative gap (second - best) / best between the two smallest FINITE distances of
    every point (inf where fewer than two are finite): points with a gap far above fp32 rounding have one defensible label.
    Row-chunked: at most `budget` float64 differences at a time.  Returns (labels int64 [N], gap float64 [N])."""
    x64, c64 = x.to(F64), c.to(F64)
    n, (k, d) = x.shape[0], c.shape
    labels = torch.empty(n, dtype=torch.int64, device=x.device)
    gap = torch.empty(n, dtype=F64, device=x.device)
    step = max(1, budget // max(1, k * d))
    for s in range(0, n, step):
        dist = ((x64[s: s + step, None, :] - c64[None, :, :]) ** 2).sum(-1)
        labels[s: s + step] = torch.argmin(torch.where(torch.isnan(dist), float("-inf"), dist), dim=1)
        fin = torch.where(torch.isfinite(dist), dist, float("inf"))
        if k >= 2:
            two = torch.topk(fin, 2, dim=1, largest=False).values
            rel = torch.where(two[:, 1] == two[:, 0], 0.0, (two[:, 1] - two[:, 0]) / two[:, 0])     # 0 / 0: a tie at distance 0
            gap[s: s + step] = torch.where(torch.isfinite(two[:, 1]), rel, float("inf"))
        else:
            gap[s: s + step] = float("inf")
    return labels, gap


KM_RUN_ENDS = [7, 8, 9, 16, 255, 256, 257, 264, 511, 512, 513, 520, 767, 768, 769, 1024, 1279, 1280, 1281]


def kmeans_labels(pattern, n, k, gen):
    """Label patterns of the M-step tests (int64 [N] on the CPU, every label in [0, K)):
      uniform  random;                      sorted  the same, ascending;
      rr       i % K: the label changes on every entry of the label-ordered list's walk and on each of the rows in flight;
      first / last   all 0 / all K - 1: one label over every work-group;
      runs     ascending runs that end at KM_RUN_ENDS - on multiples of 8 (the rows in flight) and of 256 (a work-group's entries)
               and one entry either side -, the last run takes the rest (labels past K - 1 fold onto K - 1);
      holes    random, with clusters 0, K - 1 and the block [K / 3, K / 2) left empty (needs K >= 8)."""
    if pattern == "uniform":
        return torch.randint(0, k, (n,), generator=gen)
    if pattern == "sorted":
        return torch.randint(0, k, (n,), generator=gen).sort().values
    if pattern == "rr":
        return torch.arange(n) % k
    if pattern == "first":
        return torch.zeros(n, dtype=torch.int64)
    if pattern == "last":
        return torch.full((n,), k - 1, dtype=torch.int64)
    if pattern == "runs":
        return torch.searchsorted(torch.tensor(KM_RUN_ENDS), torch.arange(n), right=True).clamp(max=k - 1)
    if pattern == "holes":
        assert k >= 8
        allowed = torch.tensor([j for j in range(1, k - 1) if not k // 3 <= j < k // 2])
        return allowed[torch.randint(0, allowed.numel(), (n,), generator=gen)]
    raise ValueError(pattern)


# ----------------------------------------------------------------------------------------------------------------------------
# nearest-neighbour search (u2seg_amd/csrc/knn_select.h, knn.hip, usl.hip): the lists, the select stage's key error, decidability
# ----------------------------------------------------------------------------------------------------------------------------
KN_SPARE = 4           # knn.hip KN_SPARE, usl.hip US_SPARE: candidates kept beyond the K (H) that are returned


def knn_dists(x_train, x_query, budget=1 << 25):
    """[Nq, Nt] float64: sum_d (x_query_id - x_train_jd)^2 in the difference form, at most `budget` differences at a time."""
    x64, y64 = x_query.to(F64), x_train.to(F64)
    nq, (nt, d) = x64.shape[0], y64.shape
    out = torch.empty((nq, nt), dtype=F64, device=x_query.device)
    step = max(1, budget // max(1, nt * d))
    for s in range(0, nq, step):
        out[s: s + step] = ((x64[s: s + step, None, :] - y64[None, :, :]) ** 2).sum(-1)
    return out


def knn_ref(x_train, x_query, k, budget=1 << 25):
    """Brute-force k nearest neighbours in float64: (d [Nq, k] float64 ascending, ind [Nq, k] int64, dist [Nq, Nt] float64 - the whole
    matrix, for knn_decidable).  A stable sort: among equal distances the smaller train index comes first; an infinite distance
    sorts behind every number and a NaN behind that (torch.sort), so a train row with a non-finite element is ranked last."""
    dist = knn_dists(x_train, x_query, budget)
    s = torch.sort(dist, dim=1, stable=True)
    return s.values[:, :k].contiguous(), s.indices[:, :k].contiguous(), dist


def knn_key_bound(x_train, x_query):
    """E_i [Nq] float64: a bound on |computed key - true key| of the select stage for query row i and EVERY train row j.

    The kernel ranks the train rows of query i by the key  kappa_ij = |y'_j|^2 - 2 x'_i . y'_j,  x' = x - m, y' = y - m, where m is
    the point the kernel translates by; kappa_ij = d_ij - |x'_i|^2, so the true keys order the rows as the true distances do,
    whatever m is.  In fp32, u = 2^-24, gamma_n = n u / (1 - n u) (gamma32), -ffp-contract=off:
      m        per column the sum of the FINITE train elements over Nt: a sum of at most Nt terms in some order (error
               <= gamma_(Nt-1) sum|y|) and one division, so |m - mean| <= delta := gamma_Nt sum|y| / Nt with mean = sum y / Nt, both
               sums over the finite elements.  m only has to be A point, but the magnitudes below are taken about it:
               |x' | <= a := |x - mean| + delta,  |y'| <= b := |y - mean| + delta  elementwise.
      staging  fl(x - m) = x'(1 + e), |e| <= u: one rounding per element of either operand.
      |y'_j|^2 squares (one rounding each) of the staged elements, summed in some order: D - 1 more roundings per term, with the two
               of the staging  |tn_j - |y'_j|^2| <= gamma_(D+2) b_j . b_j.
      x'.y'    an fma chain of length D on the MFMA, |fl(a.b) - a.b| <= gamma_D |a|.|b|, with the staging's two roundings
               |acc_ij - x'_i.y'_j| <= gamma_(D+2) a_i . b_j.
      key      fl(tn_j - 2 acc_ij): the doubling is exact, the subtraction rounds once, (1 + u)(...) - 1: with
               u + gamma_(D+2) + u gamma_(D+2) <= gamma_(D+3) (Higham, Lemma 3.3) and |kappa_ij| <= b_j.b_j + 2 a_i.b_j
                   |key_ij - kappa_ij| <= gamma_(D+3) (b_j . b_j + 2 a_i . b_j) =: E_ij,       E_i = max_j E_ij.
    The maximum runs over the train rows without a NaN or Inf element: the others are never ranked."""
    x64, y64 = x_query.to(F64), x_train.to(F64)
    nt, d = y64.shape
    fin = torch.where(torch.isfinite(y64), y64, 0.0)
    mean = fin.sum(0) / nt
    delta = float(gamma32(nt)) * fin.abs().sum(0) / nt
    y64 = y64[torch.isfinite(y64).all(1)]
    a, b = (x64 - mean).abs() + delta, (y64 - mean).abs() + delta
    per = (b * b).sum(1)[None, :] + 2 * (a @ b.T)
    return float(gamma32(d + 3)) * per.max(1).values


def knn_decidable(dist, k, e, spare=KN_SPARE):
    """[Nq] bool: at most k + spare train rows have a float64 distance <= d_(k) + 2 E_i, d_(k) the k-th smallest of the row.
    Then the k + spare smallest COMPUTED keys (ties by index) contain every row of the true top k: were a row t with d_t <= d_(k)
    missing, k + spare other rows would have computed keys <= its own, hence true keys <= kappa_t + 2 E_i, hence distances
    <= d_(k) + 2 E_i - k + spare + 1 rows with t itself.  Non-finite distances are never <= anything finite."""
    dk = torch.sort(dist, dim=1).values[:, k - 1]
    return (dist <= (dk + 2 * e)[:, None]).sum(1) <= k + spare


def lattice_rows(n, d, gen, amp=8):
    """[n, d] fp32 on the CPU: integer coordinates in [-amp, amp], every row followed by its negation and, for odd n, a last row of
    zeros - every column sums to exactly 0 in any order, so the select stage's translation is the identity and, coordinates being
    small integers, every key and every distance an integer far below 2^24: exact in fp32 whatever the order of summation."""
    half = torch.randint(-amp, amp + 1, (n // 2, d), generator=gen).float()
    rows = torch.stack([half, -half], dim=1).reshape(-1, d)
    return torch.cat([rows, torch.zeros((n % 2, d))]) if n % 2 else rows


def assert_lattice(x_train, x_query, amp=8):
    """The preconditions of the bit-for-bit kNN / USL cases, on finite elements: small integers, exact zero column sums."""
    for t in (x_train, x_query):
        f = t[torch.isfinite(t)]
        assert torch.equal(f, f.round()) and float(f.abs().max()) <= amp
    yt = torch.where(torch.isfinite(x_train), x_train, 0.0)
    assert not bool(yt.to(F64).sum(0).any()), "train columns must sum to exactly 0"
    assert 3 * x_train.shape[1] * (2 * amp) ** 2 < TWO24


def fp32_value(v):
    """The fp32 number next to the Python float v, as a Python float: what a C `float` argument receives."""
    return float(torch.tensor(v, dtype=torch.float32))


def usl_reg_ref(x, sel, labels, reg_in, h, alpha, momentum, one_minus_momentum, exclude, exact=False):
    """One update of USL's selection regularizer (u2_usl_regularizer, usl.hip) in float64 with a per-row error bound and the rows
    the bound holds for -> (want [N], bound [N], checked [N] bool, alt).  want = reg_in * momentum + S * one_minus_momentum with
    S = sum over the H nearest selected rows of 1 / v^alpha after the reference's mask (tests/usl_select_oracle.py: regularizer64);
    the two scalars are taken as given - hand the kernel the same fp32 values (fp32_value).  usl_reg_within applies the result.

    The bound, u = 2^-24, gamma_n = gamma32(n), g = gamma_(D+2) the refine stage's difference-form bound (0 with exact=True:
    lattice inputs, whose distances are integers below 2^24):
      which rows  When the K + 4 -> H + 4 candidates contain the true top H (knn_decidable with H for K), the kernel's c-th smallest
                  fp32 distance among them lies within g of the true c-th smallest d_(c), c <= H: an order statistic moves by no more
                  than its elements do.  So the kernel's sorted list is the reference's sorted list, term by term, up to g - whichever
                  rows stand behind the values.  A distance is 0 in fp32 exactly when it is 0 (no square underflows: asserted), so
                  the zero mask strikes the same terms.  With exact=True the kernel's order IS the stable float64 order and every
                  row is checked.
      the label   The row behind a value matters to the same-cluster mask alone: there the position lab = labels[i] must be in both
                  top-H sets or in neither, which fp32 guarantees when d_lab (1 + g) < d_(H+1) (1 - g) (in) or
                  d_lab (1 - g) > d_(H) (1 + g) (out), or H = S (in), or lab is no position (out); the argument above then holds for
                  the lists without lab.  Where lab is the H-th or the (H+1)-th nearest and those two are closer than that, fp32 may
                  rank either of them H-th: alt = (want_alt, bound_alt, rows) is the other outcome - the (H+1)-th in place of the
                  H-th, the mask on whichever of them is lab - and the kernel may give either.  That needs the (H-1)-th and the
                  (H+2)-th to be clear of both; a row where they are not, or where lab is unclear in another way, is unchecked.
      a term      1 / v (alpha 1: the distance's factor and one rounding), 1 / sqrt(v) (alpha 0.5: the factor - a square root halves
                  it, counted whole - and two roundings), 1 / (v v) (alpha 2: the factor twice, two roundings): a product of c
                  factors (1 + eta)^(+-1), |eta| <= g, and m factors (1 + eps)^(+-1), |eps| <= u, is within
                  r = s / (1 - s), s = c g + m u, of 1 (Higham, Lemma 3.1).  A masked term is 1e10 on both sides (an fp32 number).
      the sum     H terms in some order: gamma_(H-1) <= gamma_H of the sum of the computed terms, which are positive:
                  |S^ - S| <= e_S := (r + gamma_H (1 + r)) S.
      the blend   fl(fl(reg_in * momentum) + fl(S^ * one_minus_momentum)): three roundings,
                  bound = one_minus_momentum e_S + gamma_3 (|reg_in| momentum + one_minus_momentum (S + e_S))."""
    from tests.usl_select_oracle import regularizer64

    n, (s, d) = x.shape[0], sel.shape
    assert alpha in (1, 0.5, 2) and 1 <= h <= s and momentum >= 0 and one_minus_momentum >= 0
    g = 0.0 if exact else float(gamma32(d + 2))
    c, m = {1: (1, 1), 0.5: (1, 2), 2: (2, 2)}[alpha]
    r = (c * g + m * U24) / (1 - (c * g + m * U24))
    reg64 = reg_in.to(F64)

    def blend(new):
        e_s = (r + float(gamma32(h)) * (1 + r)) * new
        bound = one_minus_momentum * e_s + float(gamma32(3)) * (reg64.abs() * momentum + one_minus_momentum * (new + e_s))
        return reg64 * momentum + new * one_minus_momentum, bound

    want, bound = blend(regularizer64(x, sel, labels, torch.zeros(n, dtype=F64, device=x.device), h, alpha, 0.0, exclude))
    checked = torch.ones(n, dtype=torch.bool, device=x.device)
    alt = (want, bound, ~checked)
    if n and not exact:
        dist = knn_dists(sel, x)
        assert not bool(((dist > 0) & (dist < 1e-30)).any())
        checked = knn_decidable(dist, h, knn_key_bound(sel, x))
        if exclude and h < s:
            srt = torch.sort(dist, dim=1, stable=True)
            v, j = srt.values, srt.indices
            lab = labels.to(x.device).reshape(-1)
            position = (lab >= 0) & (lab < s)
            d_lab = torch.gather(dist, 1, lab.clamp(0, s - 1)[:, None])[:, 0]
            clear = (d_lab * (1 + g) < v[:, h] * (1 - g)) | (d_lab * (1 - g) > v[:, h - 1] * (1 + g)) | ~position
            at_edge = (j[:, h - 1] == lab) | (j[:, h] == lab)
            inner = v[:, h - 2] * (1 + g) < v[:, h - 1] * (1 - g) if h > 1 else torch.ones_like(clear)
            outer = v[:, h + 1] * (1 - g) > v[:, h] * (1 + g) if h + 1 < s else torch.ones_like(clear)
            swap = ~clear & at_edge & inner & outer
            vm = torch.where(j[:, : h + 1] == lab[:, None], 1e10, v[:, : h + 1])
            terms = 1 / vm if alpha == 1 else 1 / vm ** alpha
            alt = blend(terms[:, : h - 1].sum(1) + terms[:, h]) + (swap,)
            checked &= clear | swap
    return want, bound, checked, alt


def usl_reg_within(got, ref):
    """[N] bool: reg_out within usl_reg_ref's bound of the reference - or, on the rows of alt, of the other outcome."""
    want, bound, _, (want_alt, bound_alt, rows) = ref
    g = got.to(F64)
    return ((g - want).abs() <= bound) | (rows & ((g - want_alt).abs() <= bound_alt))


# ----------------------------------------------------------------------------------------------------------------------------
# k-means E step at its screening margins (tests/test_gpu_kmeans_assign_float64.py)
# ----------------------------------------------------------------------------------------------------------------------------
# Edges of the relative-gap bands, gap / (|x_i| max_j |c_j|).  1e-4 and 2e-2 are the margin_rel the launcher u2_kmeans_assign_shadow
# hands to the three-product pass and to the leading-piece pass; the shadow pass gets 3e-4 and adds the norms of what fp16 dropped
# and the index bits to it, so its margin lies between: 3e-3 is ten times its constant.
KM_BANDS = (1e-4, 3e-3, 2e-2)
KM_LADDER_RUNGS = (1, 3, 5, 7, 9, 11, 13, 16, 20)
KM_LADDER_M = (2, 5, 8, 11, 2, 5, 2, 5)     # one per pair of kmeans_ladder_pairs, in its order
KM_EDGE_ROWS = (0, 127, 128, 255, 256, -1)  # first / last point of a work-group of the exact kernel (128) and of the screens (256)


def kmeans_key_bound(x, c):
    """E_i [N] float64: a bound on |computed key - true key| of the exact E-step kernel (kmeans_assign_kernel) for point i and EVERY
    centroid j.  The kernel ranks the centroids of point i by the key  kappa_ij = |c_j|^2 - 2 x_i . c_j = d_ij - |x_i|^2,  which orders
    them as the distances do.  Nothing is translated there: this is knn_key_bound's derivation without m.  In fp32, u = 2^-24,
    gamma_n = n u / (1 - n u) (gamma32):
      cn_j   D squares (one rounding each) summed in some order (D - 1 more roundings on a term's way):
             |cn_j - |c_j|^2| <= gamma_D |c_j|.|c_j|;
      acc_ij an fma chain of length D on the MFMA:  |acc_ij - x_i.c_j| <= gamma_D |x_i|.|c_j|  (the dot product of the absolute values);
      key    fl(cn_j - 2 acc_ij): the doubling is exact, the subtraction rounds once; u + gamma_D + u gamma_D <= gamma_(D+1) (Higham,
             Lemma 3.3), and with knn_key_bound's two spare roundings
                 |key_ij - kappa_ij| <= gamma_(D+3) (|c_j|.|c_j| + 2 |x_i|.|c_j|) =: E_ij,      E_i = max_j E_ij.
    The maximum runs over the centroid rows without a NaN or Inf element.  A row of x with a NaN gets E_i = NaN.  No number here is
    measured."""
    ax = x.to(F64).abs()
    ac = c.to(F64)
    ac = ac[torch.isfinite(ac).all(1)].abs()
    per = (ac * ac).sum(1)[None, :] + 2 * (ax @ ac.T)
    return float(gamma32(x.shape[1] + 3)) * per.max(1).values


def kmeans_decision_ref(x, c, budget=1 << 25):
    """What the decision rule of the E step needs, from kmeans_argmin_ref's distance matrix (float64, difference form), row-chunked.
    Returns a dict of [N] tensors on x's device:
      ref     the float64 arg-min (NaN distance first, lowest index among equals);   d1  its distance;
      gap     d_(2) - d_(1), the ABSOLUTE float64 gap between the two smallest distances (inf for K = 1);
      e       kmeans_key_bound;   rel  gap / (|x_i| max_j |c_j|), norms in float64, the maximum over finite centroid rows;
      nan     the row of x holds a NaN;
      decidable   gap > 2 e (never for a NaN row);
      low     the lowest index j with d_ij <= d_(1) + 2 e;
      same    every centroid row within that band has the bits of row `low`."""
    x64, c64 = x.to(F64), c.to(F64)
    n, (k, d) = x.shape[0], c.shape
    dev = x.device
    e = kmeans_key_bound(x, c)
    fin = torch.isfinite(c64).all(1)
    cmax = c64[fin].norm(dim=1).max() if bool(fin.any()) else torch.zeros((), dtype=F64, device=dev)
    # canon[j]: the lowest index whose row has the bits of row j
    inv = torch.unique(c.contiguous().view(torch.int32), dim=0, return_inverse=True)[1]
    first = torch.full((int(inv.max()) + 1,), k, dtype=torch.int64, device=dev).scatter_reduce(0, inv, torch.arange(k, device=dev), "amin")
    canon = first[inv]
    out = {name: torch.empty(n, dtype=F64, device=dev) for name in ("d1", "gap")}
    out.update({name: torch.empty(n, dtype=torch.int64, device=dev) for name in ("ref", "low")})
    out["same"] = torch.empty(n, dtype=torch.bool, device=dev)
    idx = torch.arange(k, device=dev)
    step = max(1, budget // max(1, k * d))
    for s in range(0, n, step):
        sl = slice(s, s + step)
        dist = ((x64[sl, None, :] - c64[None, :, :]) ** 2).sum(-1)
        dist = torch.where(torch.isnan(dist), float("-inf"), dist)
        two = torch.topk(dist, min(2, k), dim=1, largest=False).values
        out["ref"][sl] = torch.argmin(dist, dim=1)
        out["d1"][sl] = two[:, 0]
        out["gap"][sl] = two[:, 1] - two[:, 0] if k >= 2 else float("inf")
        band = dist <= (two[:, 0] + 2 * e[sl])[:, None]
        band |= idx[None, :] == out["ref"][sl][:, None]                      # (a NaN bound compares false: the arg-min itself stays in)
        out["low"][sl] = torch.where(band, idx[None, :], k).min(1).values
        out["same"][sl] = torch.where(band, canon[None, :], -1).max(1).values == torch.where(band, canon[None, :], k).min(1).values
    out["gap"] = torch.where(torch.isnan(out["gap"]), 0.0, out["gap"])        # inf - inf, -inf - -inf: no gap to speak of
    out["e"] = e
    out["nan"] = torch.isnan(x).any(1)
    out["scale"] = x64.norm(dim=1) * cmax
    out["rel"] = out["gap"] / out["scale"]
    out["decidable"] = (out["gap"] > 2 * e) & ~out["nan"]
    return out


def kmeans_rule_ok(x, c, labels, ref):
    """[N] bool: the label obeys the decision rule, the same for every path and every point (ref = kmeans_decision_ref(x, c)):
      a row of x with a NaN     label 0 (torch.argmin on an all-NaN row; km_less);
      a decidable point         (gap > 2 E_i) the float64 arg-min: both computed keys are within E_i of the true ones, so the computed
                                order of the two nearest is the true one, and every other centroid is farther still;
      an undecidable point      the label l has d_il <= d_(1) + 2 E_i, and where all centroid rows within that band have the same bits
                                (equal keys, whatever the arithmetic) the lowest index of them.
    Rows of x with +-Inf are out of scope, as centroid rows with +-Inf are: the expanded form gives Inf - Inf there."""
    k = c.shape[0]
    inside = (labels >= 0) & (labels < k)
    lab = labels.clamp(0, k - 1)
    d_l = ((x.to(F64) - c.to(F64)[lab]) ** 2).sum(1)
    d_l = torch.where(torch.isnan(d_l), float("-inf"), d_l)
    loose = (d_l <= ref["d1"] + 2 * ref["e"]) & (~ref["same"] | (lab == ref["low"]))
    ok = torch.where(ref["nan"], lab == 0, torch.where(ref["decidable"], lab == ref["ref"], loose))
    return ok & inside


def kmeans_band(ref):
    """[N] int64: 0 undecidable (or a NaN row), 1 .. 4 the decidable point's relative-gap band (2 E_i / (|x_i| max|c|), 1e-4),
    [1e-4, 3e-3), [3e-3, 2e-2), >= 2e-2."""
    b = 1 + sum((ref["rel"] >= edge).long() for edge in KM_BANDS)
    return torch.where(ref["decidable"], b, torch.zeros_like(b))


def kmeans_rule_report(path, x, c, labels, ref):
    """None when every label obeys the rule, else the failure message: the path, the count of wrong decidable labels (and of
    undecidable ones outside their band), the first such row with its float64 gap, its E_i and its relative-gap band."""
    ok = kmeans_rule_ok(x, c, labels, ref)
    if bool(ok.all()):
        return None
    bad = ~ok
    wrong_dec = bad & ref["decidable"]
    i = int(torch.nonzero(wrong_dec if bool(wrong_dec.any()) else bad)[0, 0])
    return ("%s: %d decidable labels differ from the float64 arg-min, %d undecidable labels lie outside d_(1) + 2 E, %d NaN rows are not 0 "
            "(N = %d, K = %d, D = %d); first: row %d got %d, float64 arg-min %d, gap %.6e, E_i %.6e, relative gap %.3e, band %d" % (
                path, int(wrong_dec.sum()), int((bad & ~ref["decidable"] & ~ref["nan"]).sum()), int((bad & ref["nan"]).sum()),
                x.shape[0], c.shape[0], x.shape[1], i, int(labels[i]), int(ref["ref"][i]), float(ref["gap"][i]), float(ref["e"][i]),
                float(ref["rel"][i]), int(kmeans_band(ref)[i])))


def kmeans_ladder_pairs(k):
    """Centroid pairs (a, b) of the gap ladder - where two candidates meet in the arg-min - with their m, [(a, b, m)]:
    (0, 1), (15, 16): neighbours inside and across a 16-block;  (3, 19): the same lane of neighbouring 16-blocks;  (31, 32): across
    the exact kernel's 32-centroid tiles;  (K - 2, K - 1): the last two;  K > 320: (319, 320) and (5, 325) across the blocks of 320,
    and at K = 641 (7, K - 1), whose last block holds that one centroid.  Pairs that K has no room for, or has twice, fall away.
    c_b is made from c_a; where b already is another pair's b (K = 641: 640), the pair is made the other way round, c_a from c_b."""
    cand = [(0, 1), (15, 16), (3, 19), (31, 32), (k - 2, k - 1)]
    if k > 320:
        cand += [(319, 320), (5, 325)]
    if k == 641:
        cand.append((7, k - 1))
    out, seen, made = [], set(), set()
    for i, (a, b) in enumerate(cand):
        if not (0 <= a < k and 0 <= b < k and a != b) or (a, b) in seen:
            continue
        seen.add((a, b))
        if b in made:
            a, b = b, a
        assert b not in made and all(b not in p[:2] for p in out), (k, a, b)
        made.add(b)
        out.append((a, b, KM_LADDER_M[i]))
    return out


def kmeans_gap_ladder(k, d, n, offset=0.0, seed=0, device="cpu"):
    """Inputs of the E-step tests: (x [n, D] fp32, c [K, D] fp32, ref = kmeans_decision_ref(x, c), ladder [n] bool) on `device`.

    A background mixture as in the other k-means tests - centres 2 randn, points centre + 0.5 randn, centroids centre + 0.3 randn,
    everything + offset - and, for every pair (a, b, m) of kmeans_ladder_pairs,  c_b = c_a + 2^-m |c_a| u  (u a random unit vector)
    with the points  x = c_a + lambda (c_b - c_a) + eta,  eta orthogonal to c_b - c_a, |eta| = 0.05 |c_b - c_a|,  whose gap between a
    and b is |c_b - c_a|^2 |2 lambda - 1| whatever eta is.  lambda = 1/2 +- 2^-r for r in KM_LADDER_RUNGS and for the r that put the
    relative gap gap / (|x| max|c|) on the geometric middle of each band of KM_BANDS the pair can reach (2^-2m |c_a| / max|c| is its
    largest; the lowest band ends at 2 E / (|x| max|c|), taken at the pair's midpoint - a band that is empty there gets no rung).
    Repetitions (each with its own eta): two of the rungs of KM_LADDER_RUNGS; of the bands' rungs 120 / (2 x the number of m = 2 pairs,
    which alone reach the upper bands), so that every band gets 32 points from the ladder alone where it can: with a common offset
    of 25 the background lies in one band ([3e-3, 2e-2): neighbouring centroids are 8 D apart and |x| |c| is 630 D) and only the rungs
    on c_b's side, which is far from every other centroid, get past it; at K = 641 the pair behind centroid 640 loses rungs to
    centroid 7 next to it.
    Everything is built in float64 and rounded to fp32 once;
    the reference works from the rounded values.  Ladder rows take what n allows (all of them when n is large enough), the
    background the rest; decidable ladder rows from the narrowest bands sit at KM_EDGE_ROWS (those below n), the rest is shuffled."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * k + 31 * d + int(offset))
    rn = lambda *shape: torch.randn(shape, generator=g, dtype=F64)   # noqa: E731
    centres = 2 * rn(k, d)
    c = centres + 0.3 * rn(k, d) + offset
    pairs = kmeans_ladder_pairs(k)
    for a, b, m in pairs:
        u = rn(d)
        c[b] = c[a] + 2.0 ** -m * c[a].norm() * u / u.norm()
    c = c.float().to(F64)                                             # the centroids the points are placed between
    cmax = c.norm(dim=1).max()
    n_m2 = sum(1 for p in pairs if p[2] == 2)
    reps = -(-120 // (2 * n_m2)) if pairs else 0
    rows = []
    for a, b, m in pairs:
        w = c[b] - c[a]
        mid = c[a] + 0.5 * w
        scale = mid.norm() * cmax / (w @ w)                           # |2 lambda - 1| = relative gap x scale
        low = float(2 * kmeans_key_bound(mid[None], c)[0] / (mid.norm() * cmax))
        edges = [low * 1.02] + list(KM_BANDS) + [4 * KM_BANDS[-1]]
        banded = [0.5 * math.sqrt(lo * hi) * float(scale) for lo, hi in zip(edges[:-1], edges[1:]) if lo < hi]
        for o in 2 * [2.0 ** -r for r in KM_LADDER_RUNGS] + reps * [o for o in banded if o <= 0.5]:
            for sign in (1.0, -1.0):
                eta = rn(d)
                eta = eta - (eta @ w) / (w @ w) * w
                rows.append(c[a] + (0.5 + sign * o) * w + 0.05 * w.norm() * eta / eta.norm())
    lad = torch.stack(rows) if rows else torch.zeros((0, d), dtype=F64)
    lad = lad[torch.randperm(lad.shape[0], generator=g)[: (3 * n + 3) // 4]]     # at least a quarter of the rows is background
    nb = n - lad.shape[0]
    back = centres[torch.randint(0, k, (nb,), generator=g)] + 0.5 * rn(nb, d) + offset
    x = torch.cat([lad, back]).float()
    is_lad = torch.arange(n) < lad.shape[0]
    # the reference is a matter of each row alone: taken before the placement, which needs it, and permuted with the rows
    x, c32 = x.to(device), c.float().to(device)
    ref = kmeans_decision_ref(x, c32)
    band = kmeans_band(ref).cpu()
    by_band = [torch.nonzero((band == bnd) & is_lad)[:, 0].tolist() for bnd in (1, 2, 3, 4)]
    by_band = [rows_ for rows_ in by_band if rows_][:2]                # the two narrowest decidable bands the ladder has rows in
    edge_pos = sorted({e % n for e in KM_EDGE_ROWS if -n <= e < n})
    chosen = []
    for j in range(len(edge_pos) if by_band else 0):                   # alternately from the two
        rows_ = by_band[j % len(by_band)]
        if j // len(by_band) < len(rows_):
            chosen.append(rows_[j // len(by_band)])
    taken = set(chosen)
    rest = iter([i for i in torch.randperm(n, generator=g).tolist() if i not in taken])
    at = dict(zip(edge_pos, chosen))
    perm = torch.tensor([at[p] if p in at else next(rest) for p in range(n)], dtype=torch.int64)
    is_lad = is_lad[perm].to(device)
    perm = perm.to(device)
    return x[perm].contiguous(), c32, {name: v[perm] for name, v in ref.items()}, is_lad


def kmeans_ladder_conditions(ref, n):
    """What the ladder must offer before any kernel runs, on the reference alone -> (counts of bands 1 .. 4, undecidable share,
    band 1 is empty by construction).  Band 1, (2 E_i / (|x_i| max|c|), 1e-4), is empty where its lower end is no smaller than its
    upper one for EVERY point: 2 E_i / (|x_i| max|c|) >= 2 gamma_(D+3) max|c| / |x_i|, about 6 gamma_(D+3) on these mixtures, which
    passes 1e-4 between D = 256 and D = 768."""
    band = kmeans_band(ref)
    counts = [int((band == b).sum()) for b in (1, 2, 3, 4)]
    lower = 2 * ref["e"] / ref["scale"]
    empty = bool((lower[~ref["nan"]] >= KM_BANDS[0]).all())
    return counts, float((band == 0).sum()) / max(n, 1), empty


def kmeans_fp32_plain(x, c):
    """The E step as a plain fp32 program on whatever device: arg-min of |c_j|^2 - 2 x_i.c_j with torch.argmin's order (NaN first)."""
    key = (c * c).sum(1)[None, :] - 2 * (x @ c.T)
    return torch.argmin(torch.where(torch.isnan(key), float("-inf"), key), dim=1)


# The cases of tests/test_gpu_kmeans_assign_float64.py as (K, D, N, offset), here so that the CPU twin checks the ladder's conditions
# and the plain fp32 emulation on every one.  2817 = 256 * 11 + 1 = 128 * 22 + 1: a last work-group of one point on every path.
KM_N_STD = 11 * 256 + 1
KM_SCREEN_SHAPES = [(40, 64), (300, 256), (17, 768), (2, 32), (320, 64)]
KM_SCREENED_CASES = [(k, d, KM_N_STD, off) for k, d in KM_SCREEN_SHAPES for off in (0.0, 25.0)] + [(40, 64, 256, 0.0), (300, 256, 256, 25.0)]
KM_EXACT_CASES = [(40, 64, KM_N_STD, 0.0), (300, 256, KM_N_STD, 0.0), (300, 256, KM_N_STD, 25.0), (641, 64, KM_N_STD, 0.0),
                  (17, 768, KM_N_STD, 25.0), (40, 64, 255, 0.0), (40, 48, KM_N_STD, 0.0), (40, 16, KM_N_STD, 0.0), (1, 64, KM_N_STD, 0.0),
                  (40, 64, 1, 0.0), (40, 64, 127, 0.0), (40, 64, 129, 25.0)]
KM_TWO_LEVEL_CASES = KM_SCREENED_CASES + [(40, 64, 24 * 256 + 1, 0.0)]
KM_SHADOW_CASES = KM_SCREENED_CASES + [(40, 64, 66003, 0.0)]
KM_BLOCKS_CASES = [(k, 64, KM_N_STD, off) for k in (321, 641, 1280) for off in (0.0, 25.0)] + [(641, 256, KM_N_STD, 0.0)]
KM_ALL_CASES = sorted(set(KM_EXACT_CASES + KM_TWO_LEVEL_CASES + KM_SHADOW_CASES + KM_BLOCKS_CASES))


def kmeans_check_ladder(ref, n, d):
    """The conditions a full-size ladder case (N >= 2048, K >= 2) is asserted to meet on the reference alone: every band holds at
    least 32 decidable points - but for the lowest where it is empty by construction, which it is exactly from D = 768 on -
    and at most 0.4 of the points are undecidable.  Returns (counts of bands 1 .. 4, undecidable share)."""
    counts, undecidable, empty = kmeans_ladder_conditions(ref, n)
    assert empty == (d >= 768), (d, empty)
    assert all(cnt >= 32 for cnt in counts[1 if empty else 0:]) and undecidable <= 0.4, (counts, undecidable)
    assert not empty or counts[0] == 0
    return counts, undecidable


# ----------------------------------------------------------------------------------------------------------------------------
# row-wise top-k with a total order (u2seg_amd/csrc/select.hip; tests/test_gpu_topk_rows.py, tests/topk_cases.py)
# ----------------------------------------------------------------------------------------------------------------------------
def topk_view(vals, n, group=1, pitch=1):
    """The n elements of every row of vals [rows, ...] under the (group, pitch) view: element i at (i // group) * pitch + i % group."""
    flat = vals.reshape(vals.shape[0], -1)
    i = torch.arange(n)
    return flat[:, (i // group) * pitch + i % group]


def topk_rows_ref(vals, k, largest=True, mask=None, mask_value=1, group=1, pitch=1, n=None, idx_in=None, cnt=None, cnt_group=1,
                  idx_mod=1, idx_mul=0):
    """The contract of u2_topk_rows / u2_topk_rows_multi, in numpy on the CPU, one lexicographic sort per row.
    vals: [rows, ...] fp32 or bf16, read through the (group, pitch) view.  The participants of a row are the elements with
    mask == mask_value and, under cnt [rows, n // cnt_group], i % cnt_group < cnt[row][i // cnt_group].  Each is ranked by
    (value, reported index ascending): values compare as reals (float64 holds every fp32 / bf16 exactly), -0 equal to +0, every
    NaN of either sign the greatest value; `largest` reverses the value order only.  The reported index is idx_in[row][i]
    (else i) + (row % idx_mod) * idx_mul.  Returned values are canonical: +0.0 for either zero, the quiet NaN 0x7fc00000 for
    every NaN.  Past the count: index 0, value -inf (largest) or +inf.
    Returns (values fp32 [rows, k], indices int32 [rows, k], counts int32 [rows])."""
    import numpy as np

    rows = vals.shape[0]
    if n is None:
        n = vals.reshape(rows, -1).shape[1]
    v = topk_view(vals.cpu(), n, group, pitch).to(torch.float64).numpy()
    nan = np.isnan(v)
    v = np.where(nan, 0.0, v) + 0.0           # NaNs are ranked by their own key below; -0.0 + 0.0 = +0.0
    out_v = np.full((rows, k), -np.inf if largest else np.inf, dtype=np.float32)
    out_i = np.zeros((rows, k), dtype=np.int32)
    out_c = np.zeros((rows,), dtype=np.int32)
    pos = np.arange(n)
    for r in range(rows):
        part = np.ones(n, dtype=bool)
        if mask is not None:
            part &= mask[r].cpu().numpy() == mask_value
        if cnt is not None:
            part &= (pos % cnt_group) < cnt[r].cpu().numpy()[pos // cnt_group]
        rep = (idx_in[r].cpu().numpy().astype(np.int64) if idx_in is not None else pos) + (r % idx_mod) * idx_mul
        who = np.nonzero(part)[0]
        # np.lexsort: the last key is the primary one.  Ascending in (NaN last, value, index); descending flips the first two.
        if largest:
            order = np.lexsort((rep[who], -v[r, who], ~nan[r, who]))
        else:
            order = np.lexsort((rep[who], v[r, who], nan[r, who]))
        who = who[order][:k]
        c = len(who)
        out_c[r] = c
        out_i[r, :c] = rep[who]
        out_v[r, :c] = np.where(nan[r, who], np.float32(np.nan), v[r, who].astype(np.float32))
    res = torch.from_numpy(out_v)
    res.view(torch.int32)[torch.isnan(res)] = 0x7FC00000
    return res, torch.from_numpy(out_i), torch.from_numpy(out_c)


# ----------------------------------------------------------------------------------------------------------------------------
# head losses (u2seg_amd/csrc/losses.hip; tests/test_gpu_losses_float64.py, tests/loss_cases.py): plain torch in float64 on the
# bf16 / fp32 values the kernels read, from the formulas the header comment of losses.hip cites.  Each returns a dict: the loss
# sum, the gradient before scaling and the pieces the derived bounds are made of.  They run on the inputs' device.
# ----------------------------------------------------------------------------------------------------------------------------
def softmax_ce_ref(z, labels, nc):
    """cross_entropy(sum) over the first nc columns of z [R, LP] (fast_rcnn.py:344) and softmax - onehot."""
    zz = z[:, :nc].to(F64)
    mx = zz.amax(1, keepdim=True)
    lse = mx + torch.log(torch.exp(zz - mx).sum(1, keepdim=True))
    p = torch.exp(zz - lse)
    oh = TF.one_hot(labels, nc).to(F64)
    zt = zz.gather(1, labels[:, None])
    rows = lse - zt
    return dict(loss=rows.sum(), grad=p - oh, rows=rows, p=p, oh=oh, mx=mx, lse=lse, zt=zt, z=zz)


def semseg_ce_ref(logits, target, nc, ignore=255):
    """semantic_seg.py:255-267 with the sum in place of the mean: F.interpolate(x4, bilinear, align_corners=False) of the first nc
    channels of logits [B, h, w, LP], cross_entropy(sum, ignore_index), the gradient through autograd.  Keeps the graph of `up`
    (from the leaf `z` [B, nc, h, w]) so that a per-pixel bound can be sent through the transposed interpolation."""
    z = logits[..., :nc].to(F64).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    up = TF.interpolate(z, scale_factor=4, mode="bilinear", align_corners=False)
    t = target.long()
    ce = TF.cross_entropy(up, t, ignore_index=ignore, reduction="sum")
    (g,) = torch.autograd.grad(ce, z, retain_graph=True)
    valid = t != ignore
    return dict(loss=ce.detach(), grad=g.permute(0, 2, 3, 1), count=int(valid.sum()), z=z, up=up, target=t, valid=valid)


def mask_bce_ref(x, w, b, cls, tgt, z=None):
    """mask_head.py:258 + :33-112 with the sum in place of the mean: the gt class's channel of the 1x1 predictor (weights and bias
    rounded to bf16, the autocast conv's operands) and BCE-with-logits.  x [N, P, C] in pixel order, w [K, C], b [K], cls [N],
    tgt [N, P].  The loss and the gradients are taken at z [N, P] where given (the kernel's own rounded logit), else at the
    float64 logit.  logit_abs (the dot product's, without the bias), dW_abs, db_abs: the sums of magnitudes of the same terms."""
    k = w.shape[0]
    xx, t = x.to(F64), tgt.to(F64)
    wq, bq = bf16_round(w)[cls], bf16_round(b)[cls]                              # [N, C], [N]
    logit = torch.einsum("npc,nc->np", xx, wq) + bq[:, None]
    logit_abs = torch.einsum("npc,nc->np", xx.abs(), wq.abs())
    z = logit if z is None else z.to(F64)
    terms = z.clamp_min(0) - z * t + torch.log1p(torch.exp(-z.abs()))
    g = torch.sigmoid(z) - t
    put = lambda v: torch.zeros((k,) + v.shape[1:], dtype=F64, device=v.device).index_add_(0, cls, v)   # noqa: E731
    return dict(logit=logit, logit_abs=logit_abs, z=z, terms=terms, loss=terms.sum(), g=g, wq=wq, dx=g[:, :, None] * wq[:, None, :],
                dW=put(torch.einsum("np,npc->nc", g, xx)), dW_abs=put(torch.einsum("np,npc->nc", g.abs(), xx.abs())),
                db=put(g.sum(1)), db_abs=put(g.abs().sum(1)))


def rpn_level_ref(obj, dlt, labels, match, gt, anchors, a):
    """rpn.py:366-429 for one level, sums: BCE-with-logits over the anchors labelled 0 / 1, L1 between the deltas and
    get_deltas(anchor, matched gt; unit weights) over those labelled 1.  obj [B, HW, >= a], dlt [B, HW, >= 4 a] (the valid
    columns first), labels / match [B, HW * a] of the level, gt [B, G, 4], anchors [HW * a, 4]."""
    from tests.box_loss_refs import get_deltas

    bsz, hw = obj.shape[0], obj.shape[1]
    lab = labels.long().view(bsz, hw, a)
    mt = match.long().view(bsz, hw, a)
    zz = obj[..., :a].to(F64)
    valid, pos = lab >= 0, lab == 1
    t = lab.clamp_min(0).to(F64)
    zero = torch.zeros_like(zz)
    terms = torch.where(valid, zz.clamp_min(0) - zz * t + torch.log1p(torch.exp(-zz.abs())), zero)
    dobj = torch.where(valid, torch.sigmoid(zz) - t, zero)
    bi = torch.arange(bsz, device=obj.device)[:, None, None].expand(bsz, hw, a)
    an = anchors.to(F64).view(hw, a, 4)[None].expand(bsz, hw, a, 4)
    tg = get_deltas(an[pos], gt.to(F64)[bi[pos], mt[pos]], (1.0, 1.0, 1.0, 1.0))                       # [npos, 4]
    pr = dlt[..., : 4 * a].to(F64).view(bsz, hw, a, 4)
    df = pr[pos] - tg
    ddlt = torch.zeros_like(pr)
    ddlt[pos] = torch.sign(df)
    src = anchors.view(hw, a, 4)[None].expand(bsz, hw, a, 4)[pos]      # the positives' anchors and boxes as the kernel reads them
    return dict(loss_cls=terms.sum(), loss_loc=df.abs().sum(), terms=terms, dobj=dobj, ddlt=ddlt, df=df, tgt=tg, pred=pr[pos],
                pos=pos, valid=valid, src=src, dst=gt[bi[pos], mt[pos]], z=zz, t=t)


def box_l1_ref(pred, prop, gtb, labels, bg, weights):
    """fast_rcnn.py:424-463 with smooth_l1(beta = 0), class agnostic, the sum: L1 between pred[:, :4] and
    get_deltas(proposal, gt; weights) over the foreground rows (0 <= label < bg), and its sign."""
    from tests.box_loss_refs import get_deltas

    fg = (labels >= 0) & (labels < bg)
    tg = get_deltas(prop.to(F64), gtb.to(F64), weights)
    df = torch.where(fg[:, None], pred[:, :4].to(F64) - tg, torch.zeros_like(tg))
    return dict(loss=df.abs().sum(), grad=torch.sign(df), df=df, tgt=tg, fg=fg)
