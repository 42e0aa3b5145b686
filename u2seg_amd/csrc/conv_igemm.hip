// Implicit-GEMM convolution family on CDNA4 MFMA (gfx950), bf16 in / fp32 accumulate.
//
// Replaces the F.conv2d / F.linear / ConvTranspose2d calls behind
//   detectron2/layers/wrappers.py:127-134 (Conv2d.forward), roi_heads/box_head.py:94-97,
//   roi_heads/fast_rcnn.py:288-305, roi_heads/mask_head.py:287-290   (reference file:line)
// and their autograd backward (dgrad = the same gather with mul/div swapped and a flipped,
// transposed filter; wgrad = pixel-reduction GEMM with split-K + fp32 atomics).
//
// Data layout (HBM): activations NHWC bf16 ("pixel rows" of C channels, pitch in_ld), weights
// [N][KH*KW][C] bf16 (K contiguous per output channel), outputs [M][out_ld] bf16, M = B*Hout*Wout.
//
// Tile: 128 pixels x 128 output channels x BK reduction per workgroup of 4 waves (2x2, 64x64 per
// wave, 4x4 v_mfma_f32_16x16x32_bf16).  Operands reach LDS by global_load_lds (16 B per lane, the
// LDS image is lane-linear, the XOR bank swizzle is applied on the *source* chunk index and again
// on the fragment read).  Zero padding / row tails read a 16-byte zero page instead of branching.
// The MFMA is issued with the weight tile as the "A" operand and the pixel tile as "B", so every
// lane ends up with 4 consecutive channels of one pixel; the tile is then transposed through LDS
// and written with 16-byte coalesced stores (bias / accumulate / ReLU / BN column statistics fused).
//
// This file is the fallback family of the forward chain: the kernels that run when neither conv_stream.hip, conv_halo.hip nor
// conv_tile.hip takes the launch.  Entry points and dispatch: conv_api.hip; the per-tap weight gradient: conv_wgrad.hip.
#include "common.h"
#include "conv_args.h"
#include "u2seg_hip.h"

using namespace u2conv;
namespace {

template <int BK, bool GLDS, int TM, int TN, int NST>
__global__ __launch_bounds__((TM / 64) * (TN / 64) * 64, 2) void conv_igemm_kernel(const ConvArgs a) {
  constexpr int NW = (TM / 64) * (TN / 64);   // waves per work-group, one 64x64 sub-tile each
  constexpr int NT = NW * 64;
  constexpr int CPR = BK / 8;                 // 16-byte chunks per tile row
  constexpr int NCHP = (TM * CPR) / NT;       // chunks per thread, pixel operand
  constexpr int NCHW = (TN * CPR) / NT;       // chunks per thread, weight operand
  static_assert(NCHP >= 1 && NCHW >= 1, "tile too small for the thread count");
  constexpr int ROWS_PER_WAVE_INSTR = 64 / CPR;
  constexpr int PTILE_BYTES = TM * BK * 2;
  constexpr int WTILE_BYTES = TN * BK * 2;
  constexpr int STAGE_BYTES = PTILE_BYTES + WTILE_BYTES;
  constexpr int OPITCH = TN + 8;              // bf16 elements per row of the staged output tile
  constexpr int WM = TM / 64;                 // waves along the pixel dimension
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = a.tiles_m * a.tiles_n;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tile_m = tile / a.tiles_n;
  const int tile_n = tile - tile_m * a.tiles_n;
  const int m0 = tile_m * TM;
  const int n0 = tile_n * TN;

  // ---- per-thread chunk bookkeeping (rows are fixed across the K loop) ----
  int p_img[NCHP], p_by[NCHP], p_bx[NCHP];
  bool p_ok[NCHP];
  const bf16_t* w_row[NCHW];
  int cc;  // data chunk (8 channels) this lane fetches within a row; identical for all NCH rows
  {
    const int row_in_instr = lane / CPR;
    const int slot = lane % CPR;
    cc = slot ^ swz<BK>(row_in_instr);  // (instr,wave) offsets are multiples of the swizzle period
    const int hw = a.Hout * a.Wout;
#pragma unroll
    for (int i = 0; i < NCHP; ++i) {
      const int row = (i * NW + w) * ROWS_PER_WAVE_INSTR + row_in_instr;
      const int m = m0 + row;
      p_ok[i] = m < a.M;
      const int mm = p_ok[i] ? m : 0;
      const int img = mm / hw;
      const int rem = mm - img * hw;
      const int oy = rem / a.Wout;
      const int ox = rem - oy * a.Wout;
      p_img[i] = img;
      p_by[i] = oy * a.mul;
      p_bx[i] = ox * a.mul;
    }
#pragma unroll
    for (int i = 0; i < NCHW; ++i) {
      const int n = n0 + (i * NW + w) * ROWS_PER_WAVE_INSTR + row_in_instr;
      w_row[i] = (n < a.N) ? a.wt + (size_t)n * ((size_t)a.wt_taps * a.C) + cc * 8 : nullptr;
    }
  }

  const int kc_per_tap = a.C / BK;
  const int nk = a.ntaps * kc_per_tap;

  uint4 stage_regs[GLDS ? 1 : NCHP + NCHW];

  // Source pointers are (re)derived once per filter tap; inside a tap consecutive K tiles only advance by BK channels
  // (rows that read the zero page do not advance).  issue() is always called with kt = 0, 1, 2, ... in order.
  const bf16_t* p_src[NCHP];
  int p_inc[NCHP];
  const bf16_t* w_src[NCHW];
#pragma unroll
  for (int i = 0; i < NCHW; ++i) w_src[i] = w_row[i] ? w_row[i] : a.zero;
  int kc_in_tap = 0, tap_cur = 0, reg_kh = 0, reg_kw = 0;

  auto issue = [&](int kt, int buf) {
    (void)kt;
    if (kc_in_tap == 0) {
      int dy, dx, wtap;
      if (a.remap_out) {
        dy = a.tap_dy[tap_cur]; dx = a.tap_dx[tap_cur]; wtap = a.tap_w[tap_cur];
      } else {
        dy = reg_kh - a.pad_h; dx = reg_kw - a.pad_w; wtap = tap_cur;
        if (++reg_kw == a.KW) { reg_kw = 0; ++reg_kh; }
      }
#pragma unroll
      for (int i = 0; i < NCHP; ++i) {
        const int sy = p_by[i] + dy, sx = p_bx[i] + dx;
        const bool ok = p_ok[i] && sy >= 0 && sx >= 0 && sy < a.Hin && sx < a.Win;
        p_src[i] = ok ? a.in + ((size_t)(p_img[i] * a.Hin + sy) * a.Win + sx) * a.in_ld + cc * 8 : a.zero;
        p_inc[i] = ok ? BK : 0;
      }
#pragma unroll
      for (int i = 0; i < NCHW; ++i) w_src[i] = w_row[i] ? w_row[i] + (size_t)wtap * a.C : a.zero;
    }
    unsigned char* pbase = smem + buf * STAGE_BYTES;
    unsigned char* wbase = pbase + PTILE_BYTES;
#pragma unroll
    for (int i = 0; i < NCHP; ++i) {
      if constexpr (GLDS) glds16(p_src[i], pbase + (i * NW + w) * 1024);
      else stage_regs[i] = *reinterpret_cast<const uint4*>(p_src[i]);
      p_src[i] += p_inc[i];
    }
#pragma unroll
    for (int i = 0; i < NCHW; ++i) {
      if constexpr (GLDS) glds16(w_src[i], wbase + (i * NW + w) * 1024);
      else stage_regs[NCHP + i] = *reinterpret_cast<const uint4*>(w_src[i]);
      if (w_row[i]) w_src[i] += BK;
    }
    if (++kc_in_tap == kc_per_tap) { kc_in_tap = 0; ++tap_cur; }
  };
  auto commit = [&](int buf) {  // register-staged path only
    if constexpr (!GLDS) {
      unsigned char* pbase = smem + buf * STAGE_BYTES;
      unsigned char* wbase = pbase + PTILE_BYTES;
#pragma unroll
      for (int i = 0; i < NCHP; ++i)
        *reinterpret_cast<uint4*>(pbase + (i * NW + w) * 1024 + lane * 16) = stage_regs[i];
#pragma unroll
      for (int i = 0; i < NCHW; ++i)
        *reinterpret_cast<uint4*>(wbase + (i * NW + w) * 1024 + lane * 16) = stage_regs[NCHP + i];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wr = w / WM;  // which 64-channel slice of the tile
  const int wc = w % WM;  // which 64-pixel slice of the tile
  const int fr = lane & 15;
  const int fg = lane >> 4;

  auto compute = [&](int buf) {
    const unsigned char* pbase = smem + buf * STAGE_BYTES;
    const unsigned char* wbase = pbase + PTILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      s16x8 wf[4], pf[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int nrow = wr * 64 + t * 16 + fr;
        const int prow = wc * 64 + t * 16 + fr;
        const int kc = ks * 4 + fg;
        wf[t] = *reinterpret_cast<const s16x8*>(wbase + nrow * (BK * 2) + ((kc ^ swz<BK>(nrow)) << 4));
        pf[t] = *reinterpret_cast<const s16x8*>(pbase + prow * (BK * 2) + ((kc ^ swz<BK>(prow)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], pf[j], acc[i][j], 0, 0, 0);
    }
  };

  if constexpr (GLDS) {
    // NST-deep LDS ring: tile kt+NST-1 is in flight while tile kt is multiplied.  LDS-DMA completion is tracked
    // with counted vmcnt (each tile is LPT global_load_lds per thread, retired in order); a raw s_barrier (not
    // __syncthreads, which would drain vmcnt to 0) publishes tile kt and frees the slot of tile kt-1.
    constexpr int LPT = NCHP + NCHW;
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
      if (s0 < nk) issue(s0, s0);
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = min(nk, kt + NST - 1) - (kt + 1);
      if (NST > 3 && ahead >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPT) : "memory");
      else if (NST > 2 && ahead == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
      else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kt + NST - 1 < nk) issue(kt + NST - 1, (kt + NST - 1) % NST);
      compute(kt % NST);
    }
  } else {
    for (int kt = 0; kt < nk; ++kt) {
      issue(kt, 0);
      __syncthreads();
      commit(0);
      __syncthreads();
      compute(0);
    }
  }

  // ---- epilogue: accumulators -> LDS (bf16, [pixel][channel]) -> coalesced 16-byte stores ----
  __syncthreads();
  bf16_t* otile = reinterpret_cast<bf16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + TM * OPITCH * 2);  // [2][NW][TN] floats
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nl = wr * 64 + i * 16 + fg * 4;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (a.bias) {
      const int n = n0 + nl;
      b0 = (n + 0 < a.N) ? a.bias[n + 0] : 0.f;
      b1 = (n + 1 < a.N) ? a.bias[n + 1] : 0.f;
      b2 = (n + 2 < a.N) ? a.bias[n + 2] : 0.f;
      b3 = (n + 3 < a.N) ? a.bias[n + 3] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ml = wc * 64 + j * 16 + fr;
      float v0 = acc[i][j][0] + b0, v1 = acc[i][j][1] + b1, v2 = acc[i][j][2] + b2, v3 = acc[i][j][3] + b3;
      if (a.relu && !a.accumulate) {
        v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
      }
      uint2 pk;
      pk.x = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
      pk.y = (uint32_t)f2bf(v2) | ((uint32_t)f2bf(v3) << 16);
      *reinterpret_cast<uint2*>(otile + ml * OPITCH + nl) = pk;
    }
  }
  __syncthreads();

  constexpr int CPO = TN / 8;           // 16-byte chunks per output row
  constexpr int RPI = NT / CPO;         // rows covered per iteration
  const int cchunk = tid % CPO;
  const int rbase = tid / CPO;
  float s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; ss[e] = 0.f; }
  const bool vec_ok = ((a.out_ld & 7) == 0) && (n0 + cchunk * 8 + 8 <= a.N);
  const bool nt_out = !a.accumulate && (size_t)a.M * a.out_ld * 2 > ((size_t)160 << 20) && (a.abl & 8);
#pragma unroll
  for (int it = 0; it < TM / RPI; ++it) {
    const int row = it * RPI + rbase;
    const int m = m0 + row;
    if (m >= a.M) continue;
    uint4 v = *reinterpret_cast<const uint4*>(otile + row * OPITCH + cchunk * 8);
    bf16_t e8[8];
    *reinterpret_cast<uint4*>(e8) = v;
    size_t orow = (size_t)m;
    if (a.remap_out) {
      const int hw = a.Hout * a.Wout;
      const int img = m / hw;
      const int rem = m - img * hw;
      const int qy = rem / a.Wout;
      const int qx = rem - qy * a.Wout;
      orow = ((size_t)img * a.Hfull + qy * a.out_sy + a.out_y0) * a.Wfull + qx * a.out_sx + a.out_x0;
    }
    bf16_t* dst = a.out + orow * a.out_ld + n0 + cchunk * 8;
    if (a.accumulate) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (n0 + cchunk * 8 + e < a.N) {
          float f = bf2f(e8[e]) + bf2f(dst[e]);
          if (a.relu) f = fmaxf(f, 0.f);
          e8[e] = f2bf(f);
        }
      }
    }
    if (a.stats) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf2f(e8[e]);
        s[e] += f;
        ss[e] += f * f;
      }
    }
    if (vec_ok) {
      if (nt_out) {  // outputs far beyond the MALL size: do not let them evict what the next layer can still reuse
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
        const uint4 v = *reinterpret_cast<const uint4*>(e8);
        u32x4_t t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<u32x4_t*>(dst));
      } else {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(e8);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (n0 + cchunk * 8 + e < a.N) dst[e] = e8[e];
    }
  }
  if (a.stats) {
    // lanes sharing (lane % CPO) hold partial sums of the same 8 channels
#pragma unroll
    for (int e = 0; e < 8; ++e) {
#pragma unroll
      for (int o = CPO; o < 64; o <<= 1) {
        s[e] += __shfl_xor(s[e], o, 64);
        ss[e] += __shfl_xor(ss[e], o, 64);
      }
    }
    if (lane < CPO) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[(0 * NW + w) * TN + lane * 8 + e] = s[e];
        red[(1 * NW + w) * TN + lane * 8 + e] = ss[e];
      }
    }
    __syncthreads();
    if (tid < TN && n0 + tid < a.N) {
      float t0 = 0.f, t1 = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) {
        t0 += red[(0 * NW + ww) * TN + tid];
        t1 += red[(1 * NW + ww) * TN + tid];
      }
      atomicAdd(a.stats + n0 + tid, t0);
      atomicAdd(a.stats + a.N + n0 + tid, t1);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// 256 x 256 tile, 8 waves (4 along channels x 2 along pixels, 64 x 128 per wave), for the wide layers.
//
// Why a second structure: with 64 x 64 wave tiles a K step needs 16 ds_read_b128 per 32 MFMA and a barrier pair
// per K tile; here a wave needs 12 reads per 32 MFMA, the reduction advances in half K tiles (32 channels) through FOUR
// LDS buffers (global_load_lds runs four half tiles = two K tiles ahead, counted vmcnt(8), never drained in the loop),
// there is ONE raw barrier per half tile, and the fragments of the next phase are read from LDS before the MFMAs of
// the current one are issued (register double buffering), so LDS latency hides behind the wave's own MFMA clusters.
//
//   phase A(h): read W fragments (channels 32-63 of the wave) of half tile h; stage 2nd half of half tile h+3; 16 MFMA
//   phase B(h): vmcnt(8), barrier [publishes h+1, frees buffer h]; read W (channels 0-31) + 8 pixel fragments of h+1;
//               stage 1st half of half tile h+4 into the freed buffer; 16 MFMA
// ------------------------------------------------------------------------------------------------
constexpr int C256_THREADS = 512;
constexpr int C256_HALF_BYTES = 256 * 64;                       // one operand, one half K tile: 256 rows x 32 bf16
constexpr int C256_BUF_BYTES = 2 * C256_HALF_BYTES;             // pixels + weights
constexpr int C256_OPITCH = 256 + 8;
constexpr int C256_LDS_BYTES = 256 * C256_OPITCH * 2 + 2 * 8 * 256 * 4;  // epilogue staging + stats scratch (151 KB)
static_assert(C256_LDS_BYTES >= 4 * C256_BUF_BYTES, "ring must fit in the epilogue allocation");

template <bool STAGGER>
__global__ __launch_bounds__(C256_THREADS, 2) void conv_igemm256_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nwg = a.tiles_m * a.tiles_n;
  const int tile = xcd_remap(blockIdx.x, nwg);
  const int tile_m = tile / a.tiles_n;
  const int tile_n = tile - tile_m * a.tiles_n;
  const int m0 = tile_m * 256;
  const int n0 = tile_n * 256;

  // ---- staging bookkeeping: per half tile a thread moves 2 pixel chunks and 2 weight chunks (rows fixed) ----
  int p_img[2], p_by[2], p_bx[2];
  bool p_ok[2];
  const bf16_t* w_src[2];  // weights are [n][tap][C]: consecutive half tiles are consecutive 32-channel slabs, across taps too
  int w_inc[2];
  const int row_in = lane >> 2;
  const int cc = (lane & 3) ^ swz<32>(row_in);
  {
    const int hw = a.Hout * a.Wout;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (i * 8 + w) * 16 + row_in;
      const int m = m0 + row;
      p_ok[i] = m < a.M;
      const int mm = p_ok[i] ? m : 0;
      const int img = mm / hw;
      const int rem = mm - img * hw;
      const int oy = rem / a.Wout;
      p_img[i] = img;
      p_by[i] = oy * a.mul;
      p_bx[i] = (rem - oy * a.Wout) * a.mul;
      const int n = n0 + row;
      w_src[i] = (n < a.N) ? a.wt + (size_t)n * ((size_t)a.wt_taps * a.C) + cc * 8 : a.zero;
      w_inc[i] = (n < a.N) ? 32 : 0;
    }
  }
  const int kh_per_tap = a.C >> 5;      // half tiles (32 channels) per filter tap
  const int nkh = a.ntaps * kh_per_tap; // even (C % 64 == 0), >= 4
  const bf16_t* p_src[2];
  int p_inc[2];
  int kc_in_tap = 0, reg_kh = 0, reg_kw = 0;
  // Staging order is P(0) W(0) P(1) W(1) ...: the pixel half carries the (branchy, once per tap) pointer set-up and is
  // issued right after a barrier, where no LDS read is outstanding; the weight half is straight-line code.
  auto stage_pixels = [&](int hb) {
    if (kc_in_tap == 0) {
      const int dy = reg_kh - a.pad_h, dx = reg_kw - a.pad_w;
      if (++reg_kw == a.KW) { reg_kw = 0; ++reg_kh; }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int sy = p_by[i] + dy, sx = p_bx[i] + dx;
        const bool ok = p_ok[i] && sy >= 0 && sx >= 0 && sy < a.Hin && sx < a.Win;
        p_src[i] = ok ? a.in + ((size_t)(p_img[i] * a.Hin + sy) * a.Win + sx) * a.in_ld + cc * 8 : a.zero;
        p_inc[i] = ok ? 32 : 0;
      }
    }
    if (++kc_in_tap == kh_per_tap) kc_in_tap = 0;
    unsigned char* pbase = smem + hb * C256_BUF_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(p_src[i], pbase + (i * 8 + w) * 1024);
      p_src[i] += p_inc[i];
    }
  };
  auto stage_weights = [&](int hb) {
    unsigned char* wbase = smem + hb * C256_BUF_BYTES + C256_HALF_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(w_src[i], wbase + (i * 8 + w) * 1024);
      w_src[i] += w_inc[i];
    }
  };

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int wr = w >> 1;  // 64-channel slice
  const int wc = w & 1;   // 128-pixel slice
  const int fr = lane & 15;
  const int fg = lane >> 4;
  // the swizzle term has a period of 16 rows, so fragment t of a wave is fragment 0 + t * 1024 bytes (an immediate offset)
  const int wbase0 = C256_HALF_BYTES + (wr * 64 + fr) * 64 + ((fg ^ swz<32>(fr)) << 4);
  const int pbase0 = (wc * 128 + fr) * 64 + ((fg ^ swz<32>(fr)) << 4);
  auto ldw = [&](int hb, int t) { return *reinterpret_cast<const s16x8*>(smem + hb * C256_BUF_BYTES + wbase0 + t * 1024); };
  auto ldp = [&](int hb, int t) { return *reinterpret_cast<const s16x8*>(smem + hb * C256_BUF_BYTES + pbase0 + t * 1024); };

  s16x8 wfA[2], wfB[2], pf[8];
#define U2_C256_MFMA(I, WF, J)                                                                             \
  acc[I][J] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WF, pf[J], acc[I][J], 0, 0, 0)
#define U2_BAR()                                                                                           \
  do {                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    asm volatile("" ::: "memory");                                                                         \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
  } while (0)
  if constexpr (STAGGER) {
    // Two wave groups (waves 0-3 / 4-7: one wave of each per SIMD) run the same LOAD | MFMA | LOAD | MFMA sequence one
    // barrier apart, so that while one group issues LDS reads and LDS-DMA the other keeps the matrix pipe busy:
    //   L_A(h): read W frags (ch 0-31) + 8 pixel frags of half tile h; stage weights(h+2)
    //   M_A(h): 16 MFMA
    //   L_B(h): read W frags (ch 32-63); stage pixels(h+3)      [group 1: vmcnt for half tile h+1]
    //   M_B(h): 16 MFMA                                         [group 0: vmcnt for half tile h+1]
    // with a raw barrier after every part.  Half tile k's pixels are staged in L_B(k-3) and its weights in L_A(k-2),
    // into the buffer of half tile k-4, whose last reads (group 1's L_B(k-4)) retired two barriers earlier.
    const int grp = a.stagger_by_parity ? (w & 1) : (w >> 2);
    stage_pixels(0); stage_weights(0);
    stage_pixels(1); stage_weights(1);
    stage_pixels(2);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    U2_BAR();
    if (grp == 1) U2_BAR();  // the lag: group 1 starts one part later
#define U2_C256_HALF(H, SW, SP, VMC, NEXT)                                                                  \
  do {                                                                                                     \
    const int hb_ = (H) & 3;                                                                               \
    /* L_A */                                                                                              \
    wfA[0] = ldw(hb_, 0); wfA[1] = ldw(hb_, 1);                                                            \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) pf[j] = ldp(hb_, j);                                     \
    if (SW) stage_weights(((H) + 2) & 3);                                                                  \
    U2_BAR();                                                                                              \
    /* M_A */                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) { U2_C256_MFMA(0, wfA[0], j); U2_C256_MFMA(1, wfA[1], j); } \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    U2_BAR();                                                                                              \
    /* L_B */                                                                                              \
    wfB[0] = ldw(hb_, 2); wfB[1] = ldw(hb_, 3);                                                            \
    if (SP) stage_pixels(((H) + 3) & 3);                                                                   \
    if (NEXT && grp == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");                       \
    U2_BAR();                                                                                              \
    /* M_B */                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) { U2_C256_MFMA(2, wfB[0], j); U2_C256_MFMA(3, wfB[1], j); } \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    if (NEXT && grp == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");                       \
    U2_BAR();                                                                                              \
  } while (0)
    int h = 0;
    for (; h + 3 < nkh; ++h) U2_C256_HALF(h, true, true, 6, true);
    U2_C256_HALF(h, true, false, 4, true); ++h;    // h = nkh - 3: weights(nkh-1) are the last loads issued
    U2_C256_HALF(h, false, false, 0, true); ++h;   // h = nkh - 2
    U2_C256_HALF(h, false, false, 0, false);       // h = nkh - 1
#undef U2_C256_HALF
    if (grp == 0) U2_BAR();  // pairs with group 1's last barrier
  } else {
  // ---- prologue: P0 W0 P1 W1 P2 W2 P3 in flight (W3 follows in phase A of half tile 0), publish half tile 0 ----
  stage_pixels(0); stage_weights(0);
  stage_pixels(1); stage_weights(1);
  stage_pixels(2); stage_weights(2);
  stage_pixels(3);
  asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  wfA[0] = ldw(0, 0); wfA[1] = ldw(0, 1);
#pragma unroll
  for (int j = 0; j < 8; ++j) pf[j] = ldp(0, j);

  // One half tile.  SW / SP: stage weights(h+3) / pixels(h+4); VMC: loads that may stay in flight at the barrier;
  // NEXT: half tile h+1 exists.  LDS reads are placed so that nothing waits on a read issued less than ~8 MFMAs
  // earlier: phase A starts with MFMAs on fragments loaded in the middle of the previous phase B, reloads pixel
  // fragments 4-7 and the second weight pair after its first four MFMAs, and phase B reloads pixel fragments 0-3
  // (for the next half tile) between its two MFMA groups.
#define U2_C256_HALF(H, SW, SP, VMC, NEXT)                                                                  \
  do {                                                                                                     \
    const int hb_ = (H) & 3, nb_ = ((H) + 1) & 3;                                                          \
    /* phase A */                                                                                          \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    U2_C256_MFMA(0, wfA[0], 0); U2_C256_MFMA(1, wfA[1], 0); U2_C256_MFMA(0, wfA[0], 1); U2_C256_MFMA(1, wfA[1], 1); \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    pf[4] = ldp(hb_, 4); pf[5] = ldp(hb_, 5); pf[6] = ldp(hb_, 6); pf[7] = ldp(hb_, 7);                    \
    wfB[0] = ldw(hb_, 2); wfB[1] = ldw(hb_, 3);                                                            \
    if (SW) stage_weights(((H) + 3) & 3);                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    U2_C256_MFMA(0, wfA[0], 2); U2_C256_MFMA(1, wfA[1], 2); U2_C256_MFMA(0, wfA[0], 3); U2_C256_MFMA(1, wfA[1], 3); \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) { U2_C256_MFMA(0, wfA[0], j); U2_C256_MFMA(1, wfA[1], j); } \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    /* phase B */                                                                                          \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");                                             \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                     \
    __builtin_amdgcn_s_barrier();                                                                          \
    asm volatile("" ::: "memory");                                                                         \
    if (SP) stage_pixels(hb_);                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) { U2_C256_MFMA(2, wfB[0], j); U2_C256_MFMA(3, wfB[1], j); } \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    if (NEXT) {                                                                                            \
      wfA[0] = ldw(nb_, 0); wfA[1] = ldw(nb_, 1);                                                          \
      pf[0] = ldp(nb_, 0); pf[1] = ldp(nb_, 1); pf[2] = ldp(nb_, 2); pf[3] = ldp(nb_, 3);                  \
    }                                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                     \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int j = 4; j < 8; ++j) { U2_C256_MFMA(2, wfB[0], j); U2_C256_MFMA(3, wfB[1], j); } \
    __builtin_amdgcn_s_setprio(0);                                                                         \
  } while (0)

  int h = 0;
  for (; h + 4 < nkh; ++h) U2_C256_HALF(h, true, true, 8, true);
  U2_C256_HALF(h, true, false, 8, true); ++h;    // h = nkh - 4: weights(nkh-1) are the last loads issued
  U2_C256_HALF(h, false, false, 4, true); ++h;   // h = nkh - 3
  U2_C256_HALF(h, false, false, 0, true); ++h;   // h = nkh - 2
  U2_C256_HALF(h, false, false, 0, false);       // h = nkh - 1
#undef U2_C256_HALF
  }
#undef U2_C256_MFMA
#undef U2_BAR

  // ---- epilogue: accumulators -> LDS (bf16, [pixel][channel]) -> coalesced 16-byte stores ----
  __syncthreads();
  bf16_t* otile = reinterpret_cast<bf16_t*>(smem);
  float* red = reinterpret_cast<float*>(smem + 256 * C256_OPITCH * 2);  // [2][8][256] floats
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nl = wr * 64 + i * 16 + fg * 4;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (a.bias) {
      const int n = n0 + nl;
      b0 = (n + 0 < a.N) ? a.bias[n + 0] : 0.f;
      b1 = (n + 1 < a.N) ? a.bias[n + 1] : 0.f;
      b2 = (n + 2 < a.N) ? a.bias[n + 2] : 0.f;
      b3 = (n + 3 < a.N) ? a.bias[n + 3] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ml = wc * 128 + j * 16 + fr;
      float v0 = acc[i][j][0] + b0, v1 = acc[i][j][1] + b1, v2 = acc[i][j][2] + b2, v3 = acc[i][j][3] + b3;
      if (a.relu && !a.accumulate) {
        v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
      }
      uint2 pk;
      pk.x = (uint32_t)f2bf(v0) | ((uint32_t)f2bf(v1) << 16);
      pk.y = (uint32_t)f2bf(v2) | ((uint32_t)f2bf(v3) << 16);
      *reinterpret_cast<uint2*>(otile + ml * C256_OPITCH + nl) = pk;
    }
  }
  __syncthreads();
  const int cchunk = tid & 31;   // 32 chunks of 8 channels per output row
  const int rbase = tid >> 5;    // 16 rows per iteration
  float s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; ss[e] = 0.f; }
  const bool vec_ok = ((a.out_ld & 7) == 0) && (n0 + cchunk * 8 + 8 <= a.N);
  const bool nt_out = !a.accumulate && (size_t)a.M * a.out_ld * 2 > ((size_t)160 << 20) && (a.abl & 8);
  for (int it = 0; it < 16; ++it) {
    const int row = it * 16 + rbase;
    const int m = m0 + row;
    if (m >= a.M) continue;
    bf16_t e8[8];
    *reinterpret_cast<uint4*>(e8) = *reinterpret_cast<const uint4*>(otile + row * C256_OPITCH + cchunk * 8);
    bf16_t* dst = a.out + (size_t)m * a.out_ld + n0 + cchunk * 8;
    if (a.accumulate) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (n0 + cchunk * 8 + e < a.N) {
          float f = bf2f(e8[e]) + bf2f(dst[e]);
          if (a.relu) f = fmaxf(f, 0.f);
          e8[e] = f2bf(f);
        }
      }
    }
    if (a.stats) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf2f(e8[e]);
        s[e] += f;
        ss[e] += f * f;
      }
    }
    if (vec_ok) {
      if (nt_out) {  // outputs far beyond the MALL size: do not let them evict what the next layer can still reuse
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
        const uint4 v = *reinterpret_cast<const uint4*>(e8);
        u32x4_t t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<u32x4_t*>(dst));
      } else {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(e8);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (n0 + cchunk * 8 + e < a.N) dst[e] = e8[e];
    }
  }
  if (a.stats) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {  // lanes l and l ^ 32 hold the same 8 channels
      s[e] += __shfl_xor(s[e], 32, 64);
      ss[e] += __shfl_xor(ss[e], 32, 64);
    }
    if (lane < 32) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[(0 * 8 + w) * 256 + lane * 8 + e] = s[e];
        red[(1 * 8 + w) * 256 + lane * 8 + e] = ss[e];
      }
    }
    __syncthreads();
    if (tid < 256 && n0 + tid < a.N) {
      float t0 = 0.f, t1 = 0.f;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) {
        t0 += red[(0 * 8 + ww) * 256 + tid];
        t1 += red[(1 * 8 + ww) * 256 + tid];
      }
      atomicAdd(a.stats + n0 + tid, t0);
      atomicAdd(a.stats + a.N + n0 + tid, t1);
    }
  }
}

}  // namespace

namespace u2conv {

// The end of the forward chain (conv_api.hip): serves every shape, so it answers with the C status of the call instead of the
// launcher convention - 0, -3 when no configuration fits the LDS, or the positive hipError_t of U2_CHECK_LAUNCH (the other
// families' launch failures are -1000 - hipError_t; both values are part of the public contract and stay as they are).
int launch_conv_igemm(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s) {
  // wide layers: 256 x 256 tile, 8 waves, four-deep half-K-tile ring (v.wide)
  const bool wide_ok = !a.remap_out && C % 64 == 0 && a.ntaps * (C / 32) >= 4;
  // measured win: deep reductions (K >= 1024) with at least two full waves of 256 x 256 tiles; short-K 1x1 layers lose
  const bool wide_auto = N % 256 == 0 && a.ntaps * C >= 1024 && (long long)a.M * N >= 256LL * 256 * 512;
  if (wide_ok && v.wide != Choice::Never && (v.wide == Choice::Force || wide_auto)) {
    a.tiles_m = (a.M + 255) / 256;
    a.tiles_n = (N + 255) / 256;
    static PerDeviceOnce attr_set;
    if (auto once_guard = attr_set.first()) {
      (void)hipFuncSetAttribute((const void*)conv_igemm256_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      (void)hipFuncSetAttribute((const void*)conv_igemm256_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    a.stagger_by_parity = v.wide_stagger_parity ? 1 : 0;
    g_last_conv_kernel = U2_K_IGEMM256 + (v.wide_stagger ? U2_K_IGEMM256_STAGGER : 0);
    if (v.wide_stagger)  // staggered two-group schedule
      hipLaunchKernelGGL(conv_igemm256_kernel<true>, dim3(a.tiles_m * a.tiles_n), dim3(C256_THREADS), C256_LDS_BYTES, s, a);
    else
      hipLaunchKernelGGL(conv_igemm256_kernel<false>, dim3(a.tiles_m * a.tiles_n), dim3(C256_THREADS), C256_LDS_BYTES, s, a);
    U2_CHECK_LAUNCH();
    return 0;
  }
  const bool narrow = N <= 64;  // 256 x 64 tile
  const bool big = !narrow && v.tile_256x128;  // 256 x 128 tile, 8 waves
  const int TM = (narrow || big) ? 256 : 128, TN = narrow ? 64 : 128;
  a.tiles_m = (a.M + TM - 1) / TM;
  a.tiles_n = (N + TN - 1) / TN;
  const dim3 grid(a.tiles_m * a.tiles_n), block(big ? 512 : 256);
  const bool glds = !v.reg_staging;
  // Layers whose whole reduction is <= 256 deep (1x1 convs on <= 256 channels) are HBM-bound and never reach a steady
  // K loop: a small BK = 32 / 2-stage footprint (38 KB) keeps 4 work-groups per CU in flight instead of 2.
  const bool shallow = (long long)a.ntaps * C <= 256;  // K = 256: 440 vs 358 TFLOP/s on the 50x84 256->1024 layer
  const int bk = (C % 64 == 0 && !v.bk32 && !shallow) ? 64 : 32;
  int nst = v.ring;
  if (nst == 0) nst = (bk == 64 || shallow) ? 2 : 4;
  else nst += 1;  // 1 -> 2 stages, 2 -> 3, 3 -> 4
  if (!glds) nst = 2;
  size_t lds = (size_t)nst * (TM + TN) * bk * 2;
  const size_t epi = (size_t)TM * (TN + 8) * 2 + 2 * 8 * TN * 4;
  if (lds < epi) lds = epi;
  if (lds > 160 * 1024) return -3;
#define U2_LAUNCH_CONV(BK_, GL_, TM_, TN_, NST_)                                                                 \
  do {                                                                                                           \
    g_last_conv_kernel = U2_K_IGEMM + BK_ * 10000 + (TM_ / 64) * 1000 + (TN_ / 64) * 100 + NST_ * 10 + (GL_ ? 1 : 0); \
    static PerDeviceOnce attr_set;                                                                                \
    if (auto once_guard = attr_set.first()) {                                                                                             \
      (void)hipFuncSetAttribute((const void*)conv_igemm_kernel<BK_, GL_, TM_, TN_, NST_>,                        \
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);                         \
    }                                                                                                            \
    hipLaunchKernelGGL((conv_igemm_kernel<BK_, GL_, TM_, TN_, NST_>), grid, block, lds, s, a);                   \
  } while (0)
#define U2_PICK_NST(BK_, TM_, TN_)                                                                               \
  do {                                                                                                           \
    if (!glds) U2_LAUNCH_CONV(BK_, false, TM_, TN_, 2);                                                          \
    else if (nst == 2) U2_LAUNCH_CONV(BK_, true, TM_, TN_, 2);                                                   \
    else if (nst == 3) U2_LAUNCH_CONV(BK_, true, TM_, TN_, 3);                                                   \
    else U2_LAUNCH_CONV(BK_, true, TM_, TN_, 4);                                                                 \
  } while (0)
  if (narrow) {
    if (bk == 64) U2_PICK_NST(64, 256, 64); else U2_PICK_NST(32, 256, 64);
  } else if (big) {
    if (bk == 64) U2_PICK_NST(64, 256, 128); else U2_PICK_NST(32, 256, 128);
  } else {
    if (bk == 64) U2_PICK_NST(64, 128, 128); else U2_PICK_NST(32, 128, 128);
  }
#undef U2_PICK_NST
#undef U2_LAUNCH_CONV
  U2_CHECK_LAUNCH();
  return 0;
}

}  // namespace u2conv
