// Training through a FrozenBatchNorm2d (gfx950): the norm's fixed affine map y * s + t folded into the convolution in front of it.
// Contract: include/u2seg_hip.h, design: DESIGN.md section 24.
//
//   u2_frozen_fold            W'[n][c][t] = bf16(w[n][c][t] * s[n]) written in the two layouts the conv kernels read - the forward /
//                             weight-gradient layout [N][T][Cp] and the data-gradient layout [Cp][T][Npad] with the taps reversed -
//                             for a whole table of layers in one launch.
//   u2_frozen_wgrad_scale_add grad[n][c][t] += s[n] * scratch[n][t][c]: the transpose of the fold, from the kernel-layout weight
//                             gradient of W' into the parameter's own gradient storage.
//
// Both move weight-sized arrays (a ResNet-50 holds 23.5 M conv weights: 94 MB read, 94 MB written per fold) through an LDS
// transpose, so that the fp32 side is read / written in whole 256-byte rows and the bf16 side in 128-byte row segments, two per
// wave instruction where the layout allows pairs (the data-gradient layout, 1x1 filters).  No atomics; every
// product is one fp32 multiply with its own rounding (-ffp-contract=off), then one rounding to bf16.
#include "common.h"
#include "u2seg_hip.h"

namespace {

// One work-group per (64 output channels) x (64 contiguous (c, t) columns of the [N][Cin * T] source).
__global__ __launch_bounds__(256) void frozen_fold_kernel(const U2FrozenFoldDesc* __restrict__ table, int n_entries) {
  __shared__ float tile[64 * 65];
  const int b = blockIdx.x;
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {  // last entry with block_begin <= b
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].block_begin <= b) lo = mid; else hi = mid - 1;
  }
  const U2FrozenFoldDesc d = table[lo];
  const float* __restrict__ w = d.w;
  const float* __restrict__ s = d.s;
  bf16_t* __restrict__ fwd = (bf16_t*)d.fwd;
  bf16_t* __restrict__ dgrad = (bf16_t*)d.dgrad;
  const int N = d.N, T = d.T, Cp = d.Cp, Npad = d.Npad;
  const int J = d.Cin * T;
  const int jchunks = (J + 63) >> 6;
  const int lb = b - d.block_begin;
  const int nb = lb / jchunks, j0 = (lb - nb * jchunks) * 64, n0 = nb * 64;
  // (a table whose block counts disagree with the launcher's rule, or odd widths the pair stores cannot serve: nothing is written)
  if (n0 >= Npad || ((Npad | Cp) & 1)) return;
  const int jn = min(64, J - j0);
  const int tid = threadIdx.x;
  for (int i = tid; i < 64 * 64; i += 256) {
    const int r = i >> 6, j = i & 63;
    float v = 0.f;   // output channels N..Npad-1 of the data-gradient layout are written as zeros
    if (n0 + r < N && j < jn) v = w[(size_t)(n0 + r) * J + j0 + j] * s[n0 + r];
    tile[r * 65 + j] = v;
  }
  __syncthreads();
  // forward layout [N][T][Cp]: element (n, c, t) -> (n * T + t) * Cp + c; j (= c * T + t) runs fastest
  if (fwd && T == 1) {
    // 1x1 filters: j is the input channel - pairs of channels per lane, a wave stores two 128-byte row segments
    for (int i = tid; i < 64 * 32; i += 256) {
      const int r = i >> 5, j = (i & 31) * 2;
      if (n0 + r >= N || j >= jn) continue;
      bf16_t* dst = fwd + (size_t)(n0 + r) * Cp + j0 + j;   // Cp, j0 and j are even: 4-byte aligned
      if (j + 1 < jn) *reinterpret_cast<uint32_t*>(dst) = pack_bf16(tile[r * 65 + j], tile[r * 65 + j + 1]);
      else *dst = f2bf(tile[r * 65 + j]);
    }
  } else if (fwd) {
    for (int i = tid; i < 64 * 64; i += 256) {
      const int r = i >> 6, j = i & 63;
      if (n0 + r >= N || j >= jn) continue;
      const int jj = j0 + j, c = jj / T, t = jj - c * T;
      fwd[((size_t)(n0 + r) * T + t) * Cp + c] = f2bf(tile[r * 65 + j]);
    }
  }
  // data-gradient layout [Cp][T][Npad], taps reversed: element (n, c, t) -> (c * T + T - 1 - t) * Npad + n; n runs fastest
  if (dgrad) {
    const int nw = min(64, Npad - n0);   // Npad and n0 are multiples of 32: pairs of output channels never straddle the end
    for (int i = tid; i < 64 * 32; i += 256) {
      const int j = i >> 5, r = (i & 31) * 2;
      if (r >= nw || j >= jn) continue;
      const int jj = j0 + j, c = jj / T, t = jj - c * T;
      *reinterpret_cast<uint32_t*>(dgrad + ((size_t)c * T + (T - 1 - t)) * Npad + n0 + r) =
          pack_bf16(tile[r * 65 + j], tile[(r + 1) * 65 + j]);
    }
  }
}

// grad[n][c][t] += s[n] * scratch[n][t][c]: one work-group per output channel n; the [T][Cp] slab goes through LDS so that both the
// read (c fastest) and the read-modify-write of the [Cin][T] row (t fastest) are contiguous (u2_wgrad_permute_add with a factor)
__global__ __launch_bounds__(256) void frozen_wgrad_scale_add_kernel(const float* __restrict__ scratch, const float* __restrict__ s,
                                                                      float* __restrict__ grad, int Cin, int T, int Cp) {
  extern __shared__ float slab[];  // [T][Cp + 1]
  const int n = blockIdx.x;
  const float* src = scratch + (size_t)n * T * Cp;
  const int pitch = Cp + 1;
  for (int i = threadIdx.x; i < T * Cp; i += 256) slab[(i / Cp) * pitch + (i % Cp)] = src[i];
  __syncthreads();
  const float sn = s[n];
  float* dst = grad + (size_t)n * Cin * T;
  for (int i = threadIdx.x; i < Cin * T; i += 256) {
    const int c = i / T, t = i - c * T;
    const float scaled = sn * slab[t * pitch + c];   // dw = s * dW', rounded to fp32 before it is added
    dst[i] += scaled;
  }
}

}  // namespace

extern "C" int u2_frozen_fold(const U2FrozenFoldDesc* table, int n_entries, int total_blocks, void* stream) {
  if (n_entries <= 0 || total_blocks <= 0) return 0;
  if (!table) return -1;
  hipLaunchKernelGGL(frozen_fold_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table, n_entries);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_frozen_wgrad_scale_add(const float* scratch, const float* s, float* grad, int N, int Cin, int T, int Cp,
                                         void* stream) {
  if (N <= 0 || Cin <= 0 || T <= 0 || Cin > Cp || !scratch || !s || !grad) return -1;
  const size_t lds = (size_t)T * (Cp + 1) * sizeof(float);
  if (lds > 64 * 1024) return -2;  // 49 taps x 256 channels and beyond: no such layer stands in front of a FrozenBN here
  hipLaunchKernelGGL(frozen_wgrad_scale_add_kernel, dim3(N), dim3(256), lds, (hipStream_t)stream, scratch, s, grad, Cin, T, Cp);
  U2_CHECK_LAUNCH();
  return 0;
}
