// The stem convolution and its weight gradient straight from the images (gfx950, bf16 operands / fp32 accumulation):
//
//   out[b][oy][ox][n] = sum over (kh, kw, c) of a[b][2 oy - 3 + kh][2 ox - 3 + kw][c] * W[n][kh][kw][c]
//   dW[n][kh][kw][c] += sum over pixels of dy[b][oy][ox][n] * a[...]
//
// with a = bf16((x - mean) / std) inside the image and zero in the padding and in the canvas beyond the image: (x - mean) / std,
// ImageList.from_tensors and the 7x7 / stride-2 / pad-3 conv1 of the stem (meta_arch/rcnn.py:223-234, backbone/resnet.py:355-357).
//
// Why: the im2col form (u2_stem_im2col_batch + u2_conv_igemm + u2_conv_wgrad) writes the [M][160] bf16 operand matrix to HBM and
// reads it twice - 1.4 GB written, 2.8 GB read per 16-image step for 51 MB of pixels - and keeps it alive from forward to backward.
// stem_im2col_kernel already holds the normalised window of a patch of 8 x 32 output pixels in LDS; here the MFMA operands are
// read from that window (stem_window.h) and the matrix never exists.
//
// The reduction runs in an order of its own.  The operand values are those of the matrix bit for bit; only the order in which
// fp32 partial products are added differs.  Internally K is ordered (c, kh, kw) with kw padded to 8: "group" g = c * 7 + kh is 8
// consecutive k, 21 groups padded to 24 = 192 = 6 MFMA steps of 32.  The 8 elements of a group for output pixel (ly, lx) are 8
// CONSECUTIVE bf16 of window row (c, 2 ly + kh) from column 2 lx on: one 16-byte run (4-byte aligned) where the (kh, kw, c) order
// needs 8 two-byte gathers through a table.  The eighth element (kw = 7) and the groups 21-23 meet zero weights; the window
// columns and rows they read hold finite values (stem_stage_window fills FW = 72 columns, zeros from column 69 on).
// Window rows are SW_P = 96 elements apart: 48 dwords = 16 mod 32 banks, so the two rows a 32-lane group reads (16 pixels of two
// consecutive groups g) fall on disjoint banks.
#include "common.h"
#include "conv_args.h"
#include "stem_window.h"
#include "u2seg_hip.h"

namespace {

constexpr int SW_P = 96, SW_FW = 72;
constexpr int SC_N = 64, SC_KP = 160, SC_GROUPS = 21;

// window offset of group g (elements); the padding groups read group 0's rows against zero weights
__device__ __forceinline__ int group_off(int g) { return g < SC_GROUPS ? ((g / 7) * ST_IH + g % 7) * SW_P : 0; }
// element (g, kw) of the internal order -> column of the [64][160] (kh, kw, c) layout, -1: padding
__device__ __forceinline__ int group_col(int g, int kw) { return (g < SC_GROUPS && kw < 7) ? ((g % 7) * 7 + kw) * 3 + g / 7 : -1; }

struct PatchPos { int bi, oy0, ox0; };
__device__ __forceinline__ PatchPos patch_pos(int p, int PX, int PY) {
  PatchPos q;
  q.bi = p / (PX * PY);
  const int r = p - q.bi * (PX * PY);
  q.oy0 = (r / PX) * ST_TH;
  q.ox0 = (r % PX) * ST_TW;
  return q;
}

// The window of the NEXT patch travels through registers: fetch() issues the loads in front of the current patch's MFMA phase,
// commit() normalises and writes them once every wave has left the window (stem_window.h: the staging of stem_im2col_kernel, in
// two halves).  A thread takes runs of 4 columns: run u = it 256 + tid is columns (u % 18) 4 .. + 3 of window row u / 18 (63 rows of
// 18 runs).  The thread index is made opaque on entry: the index arithmetic is a few instructions per run, and hoisted out of the
// patch loop it would occupy registers the accumulators need.
constexpr int SW_RUNS = SW_FW / 4, SW_NRUN = 3 * ST_IH * SW_RUNS, SW_IT = (SW_NRUN + 255) / 256;
template <typename T> struct WindowRegs {
  T raw[SW_IT][4];
  unsigned in;
  __device__ __forceinline__ void fetch(const StemImages& imgs, const PatchPos& q, int tid) {
    const T* __restrict__ img = reinterpret_cast<const T*>(imgs.img[q.bi]);
    const int h = imgs.h[q.bi], w = imgs.w[q.bi];
    asm volatile("" : "+v"(tid));
    in = 0u;
#pragma unroll
    for (int it = 0; it < SW_IT; ++it) {
      const int u = it * 256 + tid, row = u / SW_RUNS, x0 = (u - row * SW_RUNS) * 4, c = row / ST_IH;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const StemWindowElem e = stem_window_elem<SW_P>(c, row - c * ST_IH, x0 + k, h, w, q.oy0 * 2 - 3, q.ox0 * 2 - 3);
        const bool ok = e.in && u < SW_NRUN;
        raw[it][k] = img[ok ? e.src : 0];
        in |= ok ? 1u << (it * 4 + k) : 0u;
      }
    }
  }
  // `lut` (uint8 images): the 3 x 256 values stem_window_value can take, computed once per work-group (fill_lut) - a pixel then
  // costs one LDS read instead of an IEEE division
  __device__ __forceinline__ void commit(bf16_t* tile, const bf16_t* lut, const float (&mean)[3], const float (&stdv)[3],
                                         int tid) const {
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int it = 0; it < SW_IT; ++it) {
      const int u = it * 256 + tid, row = u / SW_RUNS, x0 = (u - row * SW_RUNS) * 4, c = row / ST_IH;
      if (u >= SW_NRUN) break;
      bf16_t v[4];
      if constexpr (sizeof(T) == 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ((in >> (it * 4 + k)) & 1u) ? lut[c * 256 + (int)raw[it][k]] : (bf16_t)0;
      } else {
        const float mu = c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2];
        const float sd = c == 0 ? stdv[0] : c == 1 ? stdv[1] : stdv[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = stem_window_value<T>(raw[it][k], (in >> (it * 4 + k)) & 1u, mu, sd);
      }
      // (c and the LDS place depend on the run alone; 8-byte aligned: SW_P and x0 are multiples of 4)
      const StemWindowElem e = stem_window_elem<SW_P>(c, row - c * ST_IH, x0, 1, 1, 0, 0);
      *reinterpret_cast<uint2*>(tile + e.lds) = make_uint2(v[0] | ((unsigned)v[1] << 16), v[2] | ((unsigned)v[3] << 16));
    }
  }
  static __device__ __forceinline__ void fill_lut(bf16_t* lut, const float (&mean)[3], const float (&stdv)[3], int tid) {
    if constexpr (sizeof(T) == 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) lut[c * 256 + tid] = stem_window_value<T>((T)tid, true, mean[c], stdv[c]);
    }
  }
};

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// ---- forward.  4 waves; wave w owns patch rows 2 w, 2 w + 1 = 4 fragments of 16 pixels, all 64 channels.  The weights are the
// MFMA A operand and stay in registers for the work-group's life (conv_stream.hip's row order: block i, row fr = channel
// (i >> 1) 32 + (fr >> 2) 8 + (i & 1) 4 + (fr & 3), so that a lane ends up with two runs of 8 consecutive channels of one pixel).
template <typename T>
__global__ __launch_bounds__(256, 2) void stem_conv_fwd_kernel(const StemImages imgs, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, const bf16_t* __restrict__ wk,
                                                               bf16_t* __restrict__ out, float* __restrict__ stats, int b0, int Ho,
                                                               int Wo, int PX, int PY, int npatch) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[3 * ST_IH * SW_P];
  __shared__ bf16_t lut[3 * 256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nwg = gridDim.x, wg = xcd_remap(blockIdx.x, nwg);
  const int p_beg = (int)((long long)npatch * wg / nwg), p_end = (int)((long long)npatch * (wg + 1) / nwg);
  if (p_beg >= p_end) return;

  s16x8 wr[6][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = (i >> 1) * 32 + (fr >> 2) * 8 + (i & 1) * 4 + (fr & 3);
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const int g = ks * 4 + fg;
      s16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = group_col(g, e);
        const bf16_t wv = wk[n * SC_KP + (col >= 0 ? col : 0)];
        v[e] = col >= 0 ? (short)wv : (short)0;
      }
      wr[ks][i] = v;
    }
  }
  const float mu[3] = {mean[0], mean[1], mean[2]}, sd[3] = {stdv[0], stdv[1], stdv[2]};
  int goff[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) goff[ks] = group_off(ks * 4 + fg);
  const int pix0 = (2 * 2 * w) * SW_P + 2 * fr;   // patch row 2 w; the second row adds 2 * SW_P, the second 16 pixels 32

  float st_s = 0.f, st_ss = 0.f;
  const int st_n = fg * 8 + (fr >> 3) * 32 + (fr & 7);

  WindowRegs<T> win;
  win.fetch(imgs, patch_pos(p_beg, PX, PY), tid);
  WindowRegs<T>::fill_lut(lut, mu, sd, tid);
  __syncthreads();
  win.commit(tile, lut, mu, sd, tid);
  for (int p = p_beg; p < p_end; ++p) {
    __syncthreads();
    if (p + 1 < p_end) win.fetch(imgs, patch_pos(p + 1, PX, PY), tid);
    const PatchPos q = patch_pos(p, PX, PY);
    // two passes of two fragments (one patch row each): 32 accumulators beside the 96 registers of weights
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const bf16_t* trow = tile + pix0 + half * 2 * SW_P;
      f32x4 acc[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) {
        s16x8 pf[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint32_t* src = reinterpret_cast<const uint32_t*>(trow + goff[ks] + j * 32);
          const u32x4_t v = {src[0], src[1], src[2], src[3]};
          pf[j] = *reinterpret_cast<const s16x8*>(&v);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[ks][i], pf[j], acc[i][j], 0, 0, 0);
      }
      // epilogue: D[row = channel][col = pixel fr]; the lane holds channels fg 8 .. + 7 and 32 + fg 8 .. + 7 of pixel fr
      f32x2_t s2[8], ss2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s2[e] = f32x2_t{0.f, 0.f}; ss2[e] = f32x2_t{0.f, 0.f}; }
      const int oy = q.oy0 + 2 * w + half;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ox = q.ox0 + j * 16 + fr;
        const bool row_ok = oy < Ho && ox < Wo;
        uint32_t pk[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pk[2 * i] = pack_bf16(acc[i][j][0], acc[i][j][1]);
          pk[2 * i + 1] = pack_bf16(acc[i][j][2], acc[i][j][3]);
        }
        if (row_ok) {
          if (stats) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const f32x2_t v = {__uint_as_float(pk[e] << 16), __uint_as_float(pk[e] & 0xffff0000u)};
              s2[e] += v;
              ss2[e] = __builtin_elementwise_fma(v, v, ss2[e]);
            }
          }
          const unsigned off = (((unsigned)(b0 + q.bi) * Ho + oy) * Wo + ox) * SC_N + fg * 8;   // < 2^31: checked by the launcher
          *reinterpret_cast<u32x4_t*>(out + off) = u32x4_t{pk[0], pk[1], pk[2], pk[3]};
          *reinterpret_cast<u32x4_t*>(out + off + 32) = u32x4_t{pk[4], pk[5], pk[6], pk[7]};
        }
      }
      if (stats) {
        float s[16], ss[16];
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[2 * e] = s2[e][0]; s[2 * e + 1] = s2[e][1]; ss[2 * e] = ss2[e][0]; ss[2 * e + 1] = ss2[e][1]; }
        st_s += row16_transpose_sum(s, fr);
        st_ss += row16_transpose_sum(ss, fr);
      }
    }
    __syncthreads();
    if (p + 1 < p_end) win.commit(tile, lut, mu, sd, tid);
  }
  if (stats) wg_flush_column_sums<4>(stats, SC_N, st_n, st_s, st_ss, w, lane, reinterpret_cast<unsigned char*>(tile));
}

// ---- weight gradient.  The reduction runs over pixels: 32 per MFMA = one patch row.  A operand dy^T (transposing reads of the
// patch's dy rows, staged in LDS as wgrad_stream.hip lays out a step: 128-byte rows, chunks XOR tr_swz<128>), B operand
// a[pixel][k]: lane (fr, fg) of k-block kb holds element (group 2 kb + (fr >> 3), kw = fr & 7) of pixels fg 8 .. + 7 of the row,
// 8 two-byte reads 4 bytes apart.  Wave w owns k-blocks w, w + 4, w + 8 (of 12) for all 64 channels: 48 accumulators that live
// as long as the work-group, flushed once with fp32 atomics into dw[64][160] (the other work-groups hold the other patches).
template <typename T>
__global__ __launch_bounds__(256, 2) void stem_conv_wgrad_kernel(const StemImages imgs, const float* __restrict__ mean,
                                                                 const float* __restrict__ stdv, const bf16_t* __restrict__ dy,
                                                                 float* __restrict__ dw, int b0, int Ho, int Wo, int PX, int PY,
                                                                 int npatch) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[3 * ST_IH * SW_P];
  __shared__ __attribute__((aligned(16))) unsigned char dyt[ST_TH * ST_TW * SC_N * 2];
  __shared__ bf16_t lut[3 * 256];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nwg = gridDim.x, wg = xcd_remap(blockIdx.x, nwg);
  const int p_beg = (int)((long long)npatch * wg / nwg), p_end = (int)((long long)npatch * (wg + 1) / nwg);
  if (p_beg >= p_end) return;

  const float mu[3] = {mean[0], mean[1], mean[2]}, sd[3] = {stdv[0], stdv[1], stdv[2]};
  int xbase[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) xbase[t] = group_off(2 * (w + 4 * t) + (fr >> 3)) + 16 * fg + (fr & 7);
  unsigned yoff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int pix = fg * 8 + h * 4 + (fr >> 2), chy = (fr & 3) * 4;
    yoff[h] = (unsigned)(pix * 128 + (((chy >> 3) ^ u2conv::tr_swz<128>(pix)) << 4) + (chy & 7) * 2);
  }
  // dy staging: chunk ci = q 256 + tid of the patch = channels (ci & 7) 8 .. + 7 of patch pixel ci >> 3
  uint4 dreg[8];
  auto dy_fetch = [&](const PatchPos& q) {
    int tid_ = tid;
    asm volatile("" : "+v"(tid_));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ci = k * 256 + tid_, pix = ci >> 3;
      const int oy = q.oy0 + (pix >> 5), ox = q.ox0 + (pix & 31);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (oy < Ho && ox < Wo) {
        const unsigned off = (((unsigned)(b0 + q.bi) * Ho + oy) * Wo + ox) * SC_N + (ci & 7) * 8;
        v = *reinterpret_cast<const uint4*>(dy + off);
      }
      dreg[k] = v;
    }
  };
  auto dy_commit = [&]() {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ci = k * 256 + tid, pix = ci >> 3;
      *reinterpret_cast<uint4*>(dyt + pix * 128 + (((ci & 7) ^ u2conv::tr_swz<128>(pix)) << 4)) = dreg[k];
    }
  };

  f32x4 acc[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  WindowRegs<T> win;
  {
    const PatchPos q = patch_pos(p_beg, PX, PY);
    win.fetch(imgs, q, tid);
    dy_fetch(q);
    WindowRegs<T>::fill_lut(lut, mu, sd, tid);
    __syncthreads();
    win.commit(tile, lut, mu, sd, tid);
    dy_commit();
  }
  const unsigned dy0 = (unsigned)(size_t)U2_LDS_PTR(dyt);
  for (int p = p_beg; p < p_end; ++p) {
    __syncthreads();
    if (p + 1 < p_end) {
      const PatchPos q = patch_pos(p + 1, PX, PY);
      win.fetch(imgs, q, tid);
      dy_fetch(q);
    }
#pragma unroll 2
    for (int ly = 0; ly < ST_TH; ++ly) {
      u2conv::Frag yf[4], xf[3];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) yf[i].u[h] = u2conv::tr_read(dy0 + (unsigned)(ly * 4096) + (yoff[h] ^ (unsigned)(i << 5)));
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const bf16_t* src = tile + xbase[t] + ly * 2 * SW_P;
        s16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (short)src[2 * j];
        xf[t].v = v;
      }
      // the transposing reads are inline asm: their wait is ours, and the empty statements tie the registers to it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(yf[i].u[0]), "+v"(yf[i].u[1])::"memory");
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf[i].v, xf[t].v, acc[i][t], 0, 0, 0);
    }
    __syncthreads();
    if (p + 1 < p_end) {
      win.commit(tile, lut, mu, sd, tid);
      dy_commit();
    }
  }

  // flush: D[row = channel 16 i + fg 4 + r][col = k fr of block kb]
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int col = group_col(2 * (w + 4 * t) + (fr >> 3), fr & 7);
    if (col < 0) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(dw + (16 * i + fg * 4 + r) * SC_KP + col, acc[i][t][r]);
  }
}

// 0: served; 1: not served, nothing launched; < 0: bad arguments
int stem_direct_check(const int* hs, const int* ws, int n_imgs, int Hpad, int Wpad, int N, int KP, const void* act) {
  if (n_imgs < 1 || Hpad < 1 || Wpad < 1 || ((uintptr_t)act & 15)) return -1;
  bool empty = false;
  for (int i = 0; i < n_imgs; ++i) {
    if (hs[i] < 0 || ws[i] < 0) return -1;
    empty = empty || hs[i] == 0 || ws[i] == 0;   // (the staging reads pixel 0 of an image for the places outside it)
  }
  if (N != SC_N || KP != SC_KP || empty) return 1;
  const int Ho = (Hpad + 6 - 7) / 2 + 1, Wo = (Wpad + 6 - 7) / 2 + 1;
  // the kernels address the activation with 32-bit byte offsets
  if ((unsigned long long)n_imgs * Ho * Wo * SC_N * 2ull >= 0xffffffffull) return 1;
  return 0;
}

// persistent grid: two work-groups per CU
unsigned stem_grid(int npatch) { return (unsigned)(npatch < 512 ? npatch : 512); }

}  // namespace

extern "C" int u2_stem_conv_fwd(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_uint8, const float* mean,
                                const float* stdv, const void* wk, void* out, float* stats, int Hpad, int Wpad, int N, int KP,
                                void* stream) {
  const int rc = stem_direct_check(hs, ws, n_imgs, Hpad, Wpad, N, KP, out);
  if (rc) return rc;
  const int Ho = (Hpad + 6 - 7) / 2 + 1, Wo = (Wpad + 6 - 7) / 2 + 1;
  const int PX = (Wo + ST_TW - 1) / ST_TW, PY = (Ho + ST_TH - 1) / ST_TH;
  for (int b0 = 0; b0 < n_imgs; b0 += 32) {
    const int nb = n_imgs - b0 < 32 ? n_imgs - b0 : 32;
    StemImages si;
    for (int i = 0; i < nb; ++i) { si.img[i] = imgs[b0 + i]; si.h[i] = hs[b0 + i]; si.w[i] = ws[b0 + i]; }
    const int npatch = nb * PX * PY;
    if (is_uint8)
      hipLaunchKernelGGL(stem_conv_fwd_kernel<uint8_t>, dim3(stem_grid(npatch)), dim3(256), 0, (hipStream_t)stream, si, mean, stdv,
                         (const bf16_t*)wk, (bf16_t*)out, stats, b0, Ho, Wo, PX, PY, npatch);
    else
      hipLaunchKernelGGL(stem_conv_fwd_kernel<float>, dim3(stem_grid(npatch)), dim3(256), 0, (hipStream_t)stream, si, mean, stdv,
                         (const bf16_t*)wk, (bf16_t*)out, stats, b0, Ho, Wo, PX, PY, npatch);
    U2_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int u2_stem_conv_wgrad(const void* const* imgs, const int* hs, const int* ws, int n_imgs, int is_uint8,
                                  const float* mean, const float* stdv, const void* dy, float* dw, int Hpad, int Wpad, int N, int KP,
                                  void* stream) {
  const int rc = stem_direct_check(hs, ws, n_imgs, Hpad, Wpad, N, KP, dy);
  if (rc) return rc;
  const int Ho = (Hpad + 6 - 7) / 2 + 1, Wo = (Wpad + 6 - 7) / 2 + 1;
  const int PX = (Wo + ST_TW - 1) / ST_TW, PY = (Ho + ST_TH - 1) / ST_TH;
  for (int b0 = 0; b0 < n_imgs; b0 += 32) {
    const int nb = n_imgs - b0 < 32 ? n_imgs - b0 : 32;
    StemImages si;
    for (int i = 0; i < nb; ++i) { si.img[i] = imgs[b0 + i]; si.h[i] = hs[b0 + i]; si.w[i] = ws[b0 + i]; }
    const int npatch = nb * PX * PY;
    if (is_uint8)
      hipLaunchKernelGGL(stem_conv_wgrad_kernel<uint8_t>, dim3(stem_grid(npatch)), dim3(256), 0, (hipStream_t)stream, si, mean, stdv,
                         (const bf16_t*)dy, dw, b0, Ho, Wo, PX, PY, npatch);
    else
      hipLaunchKernelGGL(stem_conv_wgrad_kernel<float>, dim3(stem_grid(npatch)), dim3(256), 0, (hipStream_t)stream, si, mean, stdv,
                         (const bf16_t*)dy, dw, b0, Ho, Wo, PX, PY, npatch);
    U2_CHECK_LAUNCH();
  }
  return 0;
}
