"""Float64 reference helpers of tests/test_gpu_optim_resample_float64.py, in a plain module so that the CPU tests of
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
