// Per-tap weight gradient of the convolution family (gfx950, bf16 in / fp32 out), the end of the weight-gradient chain
// (conv_api.hip): every (n-tile, c-tile, filter tap) is a GEMM over the pixels of its own, split over pixel ranges.
//
//   wgrad: dW[n][tap][c] += sum_m dY[m][n] * X[src(m,tap)][c]    (fp32 atomics or partial tiles, split over pixels)
//
// Replaces the autograd weight gradient behind the calls listed in conv_igemm.hip for every shape that wgrad_stream.hip and
// wgrad_halo.hip do not take.
#include "common.h"
#include "conv_args.h"
#include "u2seg_hip.h"

using namespace u2conv;
namespace {

constexpr int WP = 32;  // pixels per reduction step

// The wgrad LDS image is [32 px][16 chunks of 16 bytes], chunk index XOR-swizzled by tr_swz<256>(pix) (conv_args.h).

template <bool GLDS, bool TR, int RING = 2>
__global__ __launch_bounds__(256, 4) void conv_wgrad_kernel(const WgradArgs a) {
  constexpr int TILE_BYTES = WP * 128 * 2;  // 8 KB per operand per stage
  constexpr int STAGE_BYTES = 2 * TILE_BYTES;
  static_assert(RING == 2 || (GLDS && TR), "the deeper rings exist for the LDS-DMA + transposing-read form only");
  __shared__ __attribute__((aligned(16))) unsigned char smem[RING * STAGE_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t = blockIdx.x, split = blockIdx.y;
  if (a.xcd_group) {
    // every (n-tile, c-tile, tap) of one pixel split streams the same pixels: keep them on one XCD so that its L2 serves
    // all but the first read (hardware sends work-group i to XCD i % 8)
    const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    split = logical / a.tiles;
    t = logical - split * a.tiles;
  }
  const int tile_c = t % a.tiles_c; t /= a.tiles_c;
  const int tile_n = t % a.tiles_n; t /= a.tiles_n;
  const int tap = t;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int n0 = tile_n * 128, c0 = tile_c * 128;
  const int mbeg = split * a.pix_per_wg;
  const int mend = min(a.M, mbeg + a.pix_per_wg);
  if (mbeg >= mend) return;
  const int nsteps = (mend - mbeg + WP - 1) / WP;
  const int hw = a.Hout * a.Wout;
  const bool direct = (a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad_h == 0 && a.pad_w == 0);

  // chunk assignment: instr i in {0,1}: linear chunk p = (i*4+w)*64 + lane; pix = p>>4, slot = p&15
  const int pix_in_instr = lane >> 4;
  const int slot = lane & 15;

  uint4 stage_regs[GLDS ? 1 : 4];
  // per-chunk pixel cursor, advanced by WP pixels per step with carries instead of divisions
  int cm[2], cimg[2], coy[2], cox[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pix = (i * 4 + w) * 4 + pix_in_instr;
    cm[i] = mbeg + pix;
    cimg[i] = cm[i] / hw;
    const int rem = cm[i] - cimg[i] * hw;
    coy[i] = rem / a.Wout;
    cox[i] = rem - coy[i] * a.Wout;
  }
  auto issue = [&](int step, int buf) {
    (void)step;
    unsigned char* ybase = smem + buf * STAGE_BYTES;
    unsigned char* xbase = ybase + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pix = (i * 4 + w) * 4 + pix_in_instr;
      const int cc = slot ^ tr_swz<256>(pix);
      const int m = cm[i];
      const bool mok = m < mend;
      const bf16_t* ysrc = (mok && n0 + cc * 8 < a.N) ? a.dy + (size_t)m * a.dy_ld + n0 + cc * 8 : a.zero;
      const bf16_t* xsrc = a.zero;
      if (mok && c0 + cc * 8 < a.C) {
        if (direct) {
          xsrc = a.x + (size_t)m * a.x_ld + c0 + cc * 8;
        } else {
          const int sy = coy[i] * a.stride - a.pad_h + kh;
          const int sx = cox[i] * a.stride - a.pad_w + kw;
          if (sy >= 0 && sy < a.Hin && sx >= 0 && sx < a.Win)
            xsrc = a.x + ((size_t)(cimg[i] * a.Hin + sy) * a.Win + sx) * a.x_ld + c0 + cc * 8;
        }
      }
      if constexpr (GLDS) {
        glds16(ysrc, ybase + (i * 4 + w) * 1024);
        glds16(xsrc, xbase + (i * 4 + w) * 1024);
      } else {
        stage_regs[2 * i] = *reinterpret_cast<const uint4*>(ysrc);
        stage_regs[2 * i + 1] = *reinterpret_cast<const uint4*>(xsrc);
      }
      cm[i] += WP;
      if (!direct) {
        if (a.Wout >= WP) {
          cox[i] += WP;
          while (cox[i] >= a.Wout) { cox[i] -= a.Wout; if (++coy[i] == a.Hout) { coy[i] = 0; ++cimg[i]; } }
        } else {
          cimg[i] = cm[i] / hw;
          const int rem = cm[i] - cimg[i] * hw;
          coy[i] = rem / a.Wout;
          cox[i] = rem - coy[i] * a.Wout;
        }
      }
    }
  };
  auto commit = [&](int buf) {
    if constexpr (!GLDS) {
      unsigned char* ybase = smem + buf * STAGE_BYTES;
      unsigned char* xbase = ybase + TILE_BYTES;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        *reinterpret_cast<uint4*>(ybase + (i * 4 + w) * 1024 + lane * 16) = stage_regs[2 * i];
        *reinterpret_cast<uint4*>(xbase + (i * 4 + w) * 1024 + lane * 16) = stage_regs[2 * i + 1];
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wr = w >> 1, wc = w & 1;
  const int fr = lane & 15, fg = lane >> 4;

  // Fragment for a 16-channel block starting at ch0: lane gets, for channel ch0+fr, the 8 pixels 8*fg .. 8*fg+7 of the
  // step.  LDS image: [pix][128 ch] bf16, 16-byte chunks XOR-swizzled by tr_swz<256>(pix).  All byte offsets are loop
  // invariant and computed once.
  // The 16-channel block index q only occupies bits 1-2 of the 16-byte chunk number (disjoint from the bits set by
  // wr and the lane), so offset(q) = offset(0) ^ (q << 5): two base offsets per operand instead of a table.
  constexpr int NOFF = TR ? 2 : 8;
  int yoff0[NOFF], xoff0[NOFF];
#pragma unroll
  for (int e = 0; e < NOFF; ++e) {
    // TR: ds_read_b64_tr_b16 - lane fr of a 16-lane group supplies the address of 4 contiguous bf16
    // (pixel p0 + fr/4, channels ch0 + (fr%4)*4 ..+3) and receives channel ch0+fr of pixels p0..p0+3.
    const int pix = TR ? fg * 8 + e * 4 + (fr >> 2) : fg * 8 + e;
    const int chl = TR ? (fr & 3) * 4 : fr;
    const int chy = wr * 64 + chl, chx = wc * 64 + chl;
    yoff0[e] = pix * 256 + (((chy >> 3) ^ tr_swz<256>(pix)) << 4) + (chy & 7) * 2;
    xoff0[e] = pix * 256 + (((chx >> 3) ^ tr_swz<256>(pix)) << 4) + (chx & 7) * 2;
  }
  // GLDS + TR: the transposing reads are inline asm.  Through the builtin the compiler assumes every LDS read may alias
  // the LDS-DMA writes in flight and drains them (vmcnt(0)) right after they are issued, i.e. the next step's loads
  // never overlap this step's MFMAs.  Ordering is explicit instead: vmcnt(0) + barrier before a step is read (the only
  // loads in flight at that point are that step's), lgkmcnt(0) after the reads.
  constexpr bool ASM_TR = GLDS && TR;
  const unsigned lds0 = (unsigned)(size_t)U2_LDS_PTR(smem);
  auto load_frag = [&](const unsigned char* base, const int* off0, int q) -> s16x8 {
    s16x8 r;
    if constexpr (ASM_TR) {
      Frag rr;
#pragma unroll
      for (int h = 0; h < 2; ++h) rr.u[h] = tr_read(lds0 + (unsigned)(base - smem) + (unsigned)(off0[h] ^ (q << 5)));
      r = rr.v;
    } else if constexpr (TR) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(base + (off0[h] ^ (q << 5))));
        r[h * 4 + 0] = v[0]; r[h * 4 + 1] = v[1]; r[h * 4 + 2] = v[2]; r[h * 4 + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = *reinterpret_cast<const short*>(base + (off0[e] ^ (q << 5)));
    }
    return r;
  };

  // a wave whose 64 x 64 sub-tile lies outside the valid N x C block (64-channel layers fill a quarter of the tile) only
  // helps with the staging: its MFMAs would multiply the zero page
  const bool wave_active = (n0 + wr * 64 < a.n_valid) && (c0 + wc * 64 < a.c_valid);
  auto compute = [&](int buf) {
    if (!wave_active) return;
    const unsigned char* ybase = smem + buf * STAGE_BYTES;
    const unsigned char* xbase = ybase + TILE_BYTES;
    s16x8 yf[4], xf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      yf[q] = load_frag(ybase, yoff0, q);
      xf[q] = load_frag(xbase, xoff0, q);
    }
    if constexpr (ASM_TR) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf[j], acc[i][j], 0, 0, 0);
  };

  if constexpr (GLDS && RING > 2) {
    // RING-deep LDS ring: the loads of steps st+1 .. st+RING-1 are in flight while step st is multiplied (a step is only 16
    // MFMAs per wave, ~0.1 us: with the two-buffer form every step waited out most of a memory round trip).  4 LDS-DMA
    // loads per thread per step, retired in order: counted vmcnt, raw barrier (__syncthreads would drain them).
#pragma unroll
    for (int s0 = 0; s0 < RING - 1; ++s0)
      if (s0 < nsteps) issue(s0, s0);
    int buf = 0;
    for (int st = 0; st < nsteps; ++st) {
      const int ahead = min(nsteps, st + RING - 1) - (st + 1);  // steps issued behind step st
      if (ahead >= 2) {
        if (RING > 3 && ahead >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else if (ahead == 1) {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (st + RING - 1 < nsteps) issue(st + RING - 1, buf == 0 ? RING - 1 : buf - 1);
      compute(buf);
      buf = (buf + 1 == RING) ? 0 : buf + 1;
    }
  } else if constexpr (GLDS) {
    issue(0, 0);
    for (int st = 0; st < nsteps; ++st) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (st + 1 < nsteps) issue(st + 1, (st + 1) & 1);
      compute(st & 1);
    }
  } else {
    for (int st = 0; st < nsteps; ++st) {
      issue(st, 0);
      __syncthreads();
      commit(0);
      __syncthreads();
      compute(0);
    }
  }

  // D[i = n][j = c]: lane holds column c = fr, rows n = fg*4 + r
  const int T = a.KH * a.KW;
  if (a.part) {  // 16 B per lane: rows fg * 4 .. + 3 of column c are consecutive in the [c][n] partial tile
    const int tlin = (tap * a.tiles_n + tile_n) * a.tiles_c + tile_c;
    float* pt = a.part + ((size_t)split * a.tiles + tlin) * (128 * 128);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<f32x4*>(pt + (wc * 64 + j * 16 + fr) * 128 + wr * 64 + i * 16 + fg * 4) = acc[i][j];
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + wc * 64 + j * 16 + fr;
      if (c >= a.c_valid) continue;
      float* dst = a.dw + (size_t)tap * a.dw_st + (size_t)c * a.dw_sc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wr * 64 + i * 16 + fg * 4 + r;
        if (n < a.n_valid) atomicAdd(dst + n * a.dw_sn, acc[i][j][r]);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// wgrad, 256(n) x 256(c) tile per tap, 8 waves of 64(n) x 128(c).  The 128 x 128 kernel re-streams its pixel range for every
// (n-tile, c-tile) pair - PMC: 829 MB fetched per launch against ~250 MB algorithmic - so for layers with >= 256 channels
// on both sides this halves (256 x 256 layers: both operands once per tap) the traffic that bounds it.  Each operand's
// [32 px][256 ch] step image is stored as two of the 128-channel images of the kernel above (same swizzle, same transposing
// reads); three-stage LDS ring, counted vmcnt, one raw barrier per step (one resident work-group per CU cannot hide a
// drained pipeline behind another group).
// ------------------------------------------------------------------------------------------------
constexpr int WG256_IMG = WP * 128 * 2;          // 8 KB: one [32 px][128 ch] image
constexpr int WG256_STAGE = 4 * WG256_IMG;       // dy lo / dy hi / x lo / x hi
// Fragment reads half a step ahead of their MFMAs in a four-stage ring: measured equal (profiles/r06_wgrad_halo_part.txt, last table).
// LDS ring depth: 3, 4 and 5 stages (96 ... 160 KB) measured equal (profiles/r06_wgrad_halo_part.txt, "LDS ring depth").
constexpr int WG256_STAGES = 3;

__global__ __launch_bounds__(512, 2) void conv_wgrad256_kernel(const WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t = blockIdx.x, split = blockIdx.y;
  if (a.xcd_group) {
    const int logical = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    split = logical / a.tiles;
    t = logical - split * a.tiles;
  }
  const int tile_c = t % a.tiles_c; t /= a.tiles_c;
  const int tile_n = t % a.tiles_n; t /= a.tiles_n;
  const int tap = t;
  const int kh = tap / a.KW, kw = tap - kh * a.KW;
  const int n0 = tile_n * 256, c0 = tile_c * 256;
  const int mbeg = split * a.pix_per_wg;
  const int mend = min(a.M, mbeg + a.pix_per_wg);
  if (mbeg >= mend) return;
  const int nsteps = (mend - mbeg + WP - 1) / WP;
  const int hw = a.Hout * a.Wout;
  const bool direct = (a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad_h == 0 && a.pad_w == 0);
  // a "fully connected" conv (one output position per image, no padding: fc1's 7 x 7): pixel m reads input row (m, kh, kw) - no
  // coordinates to carry (the general path below re-derives them with two integer divisions per step when Wout < 32)
  const bool fc = !direct && a.Hout == 1 && a.Wout == 1 && a.pad_h == 0 && a.pad_w == 0;
  const size_t fc_pitch = (size_t)a.Hin * a.Win * a.x_ld, fc_off = ((size_t)kh * a.Win + kw) * a.x_ld;

  // staging: wave w moves pixels 4w .. 4w+3 of the step (16 chunks each) of all four images
  const int pix = w * 4 + (lane >> 4);
  const int cc = (lane & 15) ^ tr_swz<256>(pix);
  int cm = mbeg + pix, cimg, coy, cox;
  {
    cimg = cm / hw;
    const int rem = cm - cimg * hw;
    coy = rem / a.Wout;
    cox = rem - coy * a.Wout;
  }
  auto issue = [&](int buf) {
    unsigned char* base = smem + buf * WG256_STAGE;
    const bool mok = cm < mend;
    const bf16_t* xrow = nullptr;
    if (mok) {
      if (direct) {
        xrow = a.x + (size_t)cm * a.x_ld;
      } else if (fc) {
        xrow = a.x + (size_t)cm * fc_pitch + fc_off;
      } else {
        const int sy = coy * a.stride - a.pad_h + kh;
        const int sx = cox * a.stride - a.pad_w + kw;
        if (sy >= 0 && sy < a.Hin && sx >= 0 && sx < a.Win) xrow = a.x + ((size_t)(cimg * a.Hin + sy) * a.Win + sx) * a.x_ld;
      }
    }
#pragma unroll
    for (int im = 0; im < 2; ++im) {
      const int nch = n0 + im * 128 + cc * 8, cch = c0 + im * 128 + cc * 8;
      const bf16_t* ysrc = (mok && nch < a.N) ? a.dy + (size_t)cm * a.dy_ld + nch : a.zero;
      const bf16_t* xsrc = (xrow && cch < a.C) ? xrow + cch : a.zero;
      glds16(ysrc, base + im * WG256_IMG + w * 1024);
      glds16(xsrc, base + (2 + im) * WG256_IMG + w * 1024);
    }
    cm += WP;
    if (!direct && !fc) {
      if (a.Wout >= WP) {
        cox += WP;
        while (cox >= a.Wout) { cox -= a.Wout; if (++coy == a.Hout) { coy = 0; ++cimg; } }
      } else {
        cimg = cm / hw;
        const int rem = cm - cimg * hw;
        coy = rem / a.Wout;
        cox = rem - coy * a.Wout;
      }
    }
  };

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wr = w >> 1, wc = w & 1;  // wr: 64-channel slice of dy (image wr >> 1, half wr & 1); wc: x image (128 channels)
  const int fr = lane & 15, fg = lane >> 4;
  // transposing-read offsets inside one image (see conv_wgrad_kernel); the 16-channel block q is offset ^ (q << 5)
  int yoff0[2], xoff0[2][2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int px = fg * 8 + e * 4 + (fr >> 2);
    const int chl = (fr & 3) * 4;
    const int chy = (wr & 1) * 64 + chl;
    yoff0[e] = (wr >> 1) * WG256_IMG + px * 256 + (((chy >> 3) ^ tr_swz<256>(px)) << 4) + (chy & 7) * 2;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int chx = hh * 64 + chl;
      xoff0[hh][e] = (2 + wc) * WG256_IMG + px * 256 + (((chx >> 3) ^ tr_swz<256>(px)) << 4) + (chx & 7) * 2;
    }
  }
  // The transposing reads are issued as inline asm: for the builtin the compiler assumes that an LDS read may alias the
  // LDS-DMA writes still in flight and drains them (s_waitcnt vmcnt(0)) before every step, which turns the ring into a
  // synchronous load.  Ordering is explicit instead: counted vmcnt + barrier before the reads, lgkmcnt(0) after them.
  const unsigned lds0 = (unsigned)(size_t)U2_LDS_PTR(smem);
  auto load_frag = [&](unsigned base, const int* off0, int q) -> s16x8 {
    Frag r;
#pragma unroll
    for (int h = 0; h < 2; ++h) r.u[h] = tr_read(base + (unsigned)(off0[h] ^ (q << 5)));
    return r.v;
  };
  auto compute = [&](int buf) {
    const unsigned base = lds0 + buf * WG256_STAGE;
    s16x8 yf[4], xf[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      yf[q] = load_frag(base, yoff0, q);
      xf[q] = load_frag(base, xoff0[0], q);
      xf[4 + q] = load_frag(base, xoff0[1], q);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i], xf[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // ring of WG256_STAGES stages: steps st+1 .. st+STAGES-1 are in flight while step st is multiplied (4 LDS-DMA loads per thread
  // per step); at the barrier of step st everything but the stages behind it has landed
  static_assert(WG256_STAGES == 3, "the counted waits below are written for one stage in flight behind the step");
#pragma unroll
  for (int s0 = 0; s0 < WG256_STAGES - 1; ++s0)
    if (s0 < nsteps) issue(s0);
  for (int st = 0; st < nsteps; ++st) {
    const int behind = min(WG256_STAGES - 2, nsteps - 1 - st);   // stages issued behind step st that may still be in flight
    if (behind == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (st + WG256_STAGES - 1 < nsteps) issue((st + WG256_STAGES - 1) % WG256_STAGES);
    compute(st % WG256_STAGES);
  }

  // D[i = n][j = c]: lane holds column c = fr, rows n = fg*4 + r
  if (a.part) {
    const int tlin = (tap * a.tiles_n + tile_n) * a.tiles_c + tile_c;
    float* pt = a.part + ((size_t)split * a.tiles + tlin) * (256 * 256);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<f32x4*>(pt + (wc * 128 + (j >> 2) * 64 + (j & 3) * 16 + fr) * 256 + wr * 64 + i * 16 + fg * 4) = acc[i][j];
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + wc * 128 + (j >> 2) * 64 + (j & 3) * 16 + fr;
      if (c >= a.c_valid) continue;
      float* dst = a.dw + (size_t)tap * a.dw_st + (size_t)c * a.dw_sc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wr * 64 + i * 16 + fg * 4 + r;
        if (n < a.n_valid) atomicAdd(dst + n * a.dw_sn, acc[i][j][r]);
      }
    }
}

// Sums the partial tiles of a weight-gradient launch over its pixel splits and adds the result into dw (single owner per
// element: plain read-modify-write).  TILE x TILE partials, [c][n] with n fastest; a work-group takes 8 columns c of one tile:
// 32 lanes x 16 B per column and split (coalesced), the sums go through LDS so that the dw accesses run along c (the contiguous
// direction of both gradient layouts).
template <int TILE>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int splits, int tiles, int per_group,
                                                           WgradArgs a) {
  constexpr int NQ = TILE / 4;            // 16-byte groups per column
  constexpr int CPW = 256 / NQ;           // columns per pass of the work-group (8 for 128, 4 for 256)
  constexpr int COLS = 8;                 // columns per work-group
  __shared__ float sm[COLS][TILE + 1];
  const int tlin = blockIdx.x, slab = blockIdx.y;
  int t = tlin;
  const int tile_c = t % a.tiles_c; t /= a.tiles_c;
  const int tile_n = t % a.tiles_n; t /= a.tiles_n;
  const int tap = t;
  const int tid = threadIdx.x;
  const int nq = tid % NQ, ci = tid / NQ;
#pragma unroll
  for (int cc = 0; cc < COLS / CPW; ++cc) {
    const int c_local = slab * COLS + cc * CPW + ci;
    const float* src = part + (size_t)tlin * (TILE * TILE) + c_local * TILE + nq * 4;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    // blockIdx.z = group of `per_group` consecutive splits (launches with few tiles and hundreds of splits: a work-group per
    // (tile, 8 columns) alone would be 32 work-groups reading 2 MB each); several groups meet in dw through atomics
    int sp = blockIdx.z * per_group;
    const int sp_end = min(splits, sp + per_group);
    const size_t sstride = (size_t)tiles * (TILE * TILE);
    // round 6: eight loads in flight per thread (the partials come back from the MALL at ~1 us per dependent round trip; with
    // pairs a work-group summing 16 splits spent eight round trips on 2 KB of data per thread)
    for (; sp + 7 < sp_end; sp += 8) {
      f32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (size_t)(sp + k) * sstride));
      s0 += (v[0] + v[2]) + (v[4] + v[6]);
      s1 += (v[1] + v[3]) + (v[5] + v[7]);
    }
    for (; sp + 1 < sp_end; sp += 2) {   // two independent chains: the loads of a pair are in flight together
      s0 += *reinterpret_cast<const f32x4*>(src + (size_t)sp * sstride);
      s1 += *reinterpret_cast<const f32x4*>(src + (size_t)(sp + 1) * sstride);
    }
    if (sp < sp_end) s0 += *reinterpret_cast<const f32x4*>(src + (size_t)sp * sstride);
    s0 += s1;
    float* row = sm[cc * CPW + ci] + nq * 4;
    row[0] = s0[0]; row[1] = s0[1]; row[2] = s0[2]; row[3] = s0[3];
  }
  __syncthreads();
  const int c_rel = tid & (COLS - 1);
  const int c = tile_c * TILE + slab * COLS + c_rel;
  if (c >= a.c_valid) return;
  float* dst = a.dw + (size_t)tap * a.dw_st + (size_t)c * a.dw_sc;
  for (int nl = tid / COLS; nl < TILE; nl += 256 / COLS) {
    const int n = tile_n * TILE + nl;
    if (n < a.n_valid) {
      if (gridDim.z == 1) dst[n * a.dw_sn] += sm[c_rel][nl];
      else atomicAdd(dst + n * a.dw_sn, sm[c_rel][nl]);
    }
  }
}

constexpr size_t WG_SCRATCH_LIMIT = (size_t)96 << 20;
float* wgrad_scratch(hipStream_t s, size_t need_bytes) {
  return (float*)u2conv::scratch_get(2, s, need_bytes, WG_SCRATCH_LIMIT, false);
}

}  // namespace

namespace u2conv {

// Serves every shape, so like launch_conv_igemm it answers with the C status of the call: 0, or the positive hipError_t of
// U2_CHECK_LAUNCH (the other weight-gradient families fail with -1000 - hipError_t; both values stay as they are).
int launch_wgrad_per_tap(WgradArgs& a, const WgradVariant& v, hipStream_t s) {
  const int KH = a.KH, KW = a.KW, N = a.N, C = a.C, Hout = a.Hout, Wout = a.Wout;
  // 256 x 256 tiles on the multi-tap layers: only on request (v.wide).  Measured 516 vs 805 TFLOP/s on the 200x336 3x3 256->256 layer: with
  // one resident work-group per CU the transposing reads of a step are not hidden behind anything, while four resident
  // 128 x 128 groups hide them behind each other, which outweighs the halved operand traffic.
  // 256 x 256 tiles (half the operand traffic per flop) win where nothing else hides the memory stream: 1x1 layers over the
  // stride-4 / stride-8 maps and the 7x7 "fully connected" fc1 (tests/native/selftest bench2w, profiles/r02_wgrad_variants.txt)
  // Round 4, with the partial-tile reduction in place of the 256 KB atomic epilogue (bench2w 0 256 2048, profiles/r04_wgrad_partials.txt):
  // the 256-wide tiles also win on the stride-16 1x1 layers (res4 256 <-> 1024: 71 -> 67-69 us on two boxes, the stride-2 512 -> 1024
  // 124 -> 112) - wherever both channel counts fill 256-wide tiles; with a 128-channel side (128 <-> 512, 256 -> 128) the result
  // flipped between two boxes (+-10 %), so those stay on the 128-wide tiles; below ~50 k pixels (res5, the FC layers) they lose.
  const bool wide_1x1 = KH * KW == 1 && a.M >= 50000 && N % 256 == 0 && C % 256 == 0;
  const bool wide_auto = v.wide != Choice::Never &&
                         (wide_1x1 || ((N % 256 == 0) && (C % 256 == 0) && KH * KW > 1 && a.M <= 16384 && Hout == 1 && Wout == 1));
  const bool wide = (v.wide == Choice::Force || wide_auto) && !v.reg_staging && !v.scalar_gather;
  const int tw = wide ? 256 : 128;
  a.tiles_n = (N + tw - 1) / tw;
  a.tiles_c = (C + tw - 1) / tw;
  const int tiles = a.tiles_n * a.tiles_c * KH * KW;
  // Pixel splits: fill the chip once (4 resident work-groups per CU = 1024 slots) but keep >= 2048 pixels per
  // work-group so that the 64 KB fp32-atomic epilogue stays a small fraction; tiny layers fall back to >= 512 groups.
  int slots = (wide ? 256 : 1024) >> v.fewer_splits;  // resident work-groups; U2_WG_FEWER_SPLITS: tuning knob
  int splits = slots / tiles;
  if (splits < 1) splits = 1;
  // (1024 and 512 pixels per work-group measured 25 % slower on the stride-16 / 32 layers: the epilogue grows with the splits)
  const int by_pixels = a.M / 2048 > 1 ? a.M / 2048 : 1;
  if (splits > by_pixels) splits = by_pixels;
  const int min_groups = wide ? 256 : 512;
  if (tiles * splits < min_groups) {
    int s2 = (min_groups + tiles - 1) / tiles;
    const int cap = a.M / 512 > 1 ? a.M / 512 : 1;
    if (s2 > cap) s2 = cap;
    if (s2 > splits) splits = s2;
  }
  int ppw = (a.M + splits - 1) / splits;
  ppw = ((ppw + WP - 1) / WP) * WP;
  splits = (a.M + ppw - 1) / ppw;
  a.pix_per_wg = ppw;
  a.tiles = tiles;
  // measured: +29% on res3 3x3, +6% on the 200x336 3x3 layers, -3..-10% on small-M layers and plain GEMMs
  a.xcd_group = (v.xcd == Choice::Force || (v.xcd != Choice::Never && KH * KW > 1 && a.M >= 200000)) ? 1 : 0;
  const dim3 grid = a.xcd_group ? dim3(tiles * splits) : dim3(tiles, splits);
  const dim3 block(256);
  // partial tiles + one reduction pass instead of the fp32-atomic epilogue (U2_WG_ATOMICS keeps the atomics); a single split
  // has nothing to reduce and little to gain
  a.part = nullptr;
  // Measured (tests/native/selftest bench2w 0 65536, round 4): the atomics of a long kernel hide behind the work-groups that are
  // still multiplying, so the pass only pays where the launch is short or has many tiles - 1x1 layers on the stride-8 ... 32 maps
  // (res4 78 -> 72 us, res5 67 -> 58, lat3 126 -> 113, res3 256->512 138 -> 114), mid-size 3x3 layers (+3...10 %); it loses on
  // the stride-4 1x1 layers with one or two tiles and 512 splits (64 MB of partials: 64->256 134 -> 156 us) and on the big 3x3
  // layers (-2...4 %).  U2_WG_PARTIALS_FORCE forces the pass wherever splits >= 2.
  const long long dw_elems = (long long)a.tiles_n * a.tiles_c * tw * tw;
  const bool part_auto = dw_elems >= 4LL * 128 * 128 && !(KH * KW > 1 && a.M >= 200000);
  if (!v.atomics && splits >= 2 && (part_auto || v.partials_force))
    a.part = wgrad_scratch(s, (size_t)tiles * splits * tw * tw * sizeof(float));
  auto reduce = [&]() -> int {
    if (!a.part) return 0;
    const int slabs = tw / 8;
    int groups = (512 + tiles * slabs - 1) / (tiles * slabs);   // >= ~512 work-groups in the reduction pass
    if (groups > splits / 4) groups = splits / 4 > 1 ? splits / 4 : 1;
    const int per_group = (splits + groups - 1) / groups;
    groups = (splits + per_group - 1) / per_group;
    if (wide) hipLaunchKernelGGL(wgrad_reduce_kernel<256>, dim3(tiles, slabs, groups), dim3(256), 0, s, a.part, splits, tiles, per_group, a);
    else hipLaunchKernelGGL(wgrad_reduce_kernel<128>, dim3(tiles, slabs, groups), dim3(256), 0, s, a.part, splits, tiles, per_group, a);
    U2_CHECK_LAUNCH();
    return 0;
  };
  const bool glds = !v.reg_staging, tr = !v.scalar_gather;
  g_last_conv_kernel = (wide ? U2_K_WGRAD256 : U2_K_WGRAD + (glds ? 2 : 0) + (tr ? 1 : 0)) + (a.xcd_group ? U2_K_WGRAD_XCD : 0);
  if (wide) {
    static PerDeviceOnce attr_set;
    if (auto once_guard = attr_set.first()) {
      (void)hipFuncSetAttribute((const void*)conv_wgrad256_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    hipLaunchKernelGGL(conv_wgrad256_kernel, grid, dim3(512), WG256_STAGES * WG256_STAGE, s, a);
    U2_CHECK_LAUNCH();
    return reduce();
  }
  const int ring = v.ring;  // LDS ring depth of the LDS-DMA form (0 = two buffers, 1 = 3, 2 = 4)
  if (glds && tr && ring == 1)      hipLaunchKernelGGL((conv_wgrad_kernel<true, true, 3>), grid, block, 0, s, a);
  else if (glds && tr && ring == 2) hipLaunchKernelGGL((conv_wgrad_kernel<true, true, 4>), grid, block, 0, s, a);
  else if (glds && tr)  hipLaunchKernelGGL((conv_wgrad_kernel<true, true>), grid, block, 0, s, a);
  else if (glds && !tr) hipLaunchKernelGGL((conv_wgrad_kernel<true, false>), grid, block, 0, s, a);
  else if (!glds && tr) hipLaunchKernelGGL((conv_wgrad_kernel<false, true>), grid, block, 0, s, a);
  else                  hipLaunchKernelGGL((conv_wgrad_kernel<false, false>), grid, block, 0, s, a);
  U2_CHECK_LAUNCH();
  return reduce();
}

}  // namespace u2conv
