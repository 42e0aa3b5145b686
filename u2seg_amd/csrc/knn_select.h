// Candidate stage of the brute-force nearest-neighbour search, shared by knn.hip (u2_knn, K <= 28) and usl.hip (the USL
// selection regularizer, H <= 64).  See knn.hip for the method:
//   select  for 128 query rows per workgroup, stream every train row through LDS; dot products on the exact-fp32 MFMA
//           (v_mfma_f32_32x32x2_f32, an fma chain in k order); rank key |y_j|^2 - 2 x_i.y_j on rows translated by the train
//           set's column mean; survivors of a per-row threshold go through a per-row LDS queue into a per-row sorted list of
//           KK <= KMAX candidates, written to cand[Nq][KK] (INT_MAX where a row has fewer than KK train rows).
// Template parameters: KMAX, the list capacity (LDS pitch KMAX + 1), and TILES, the 32-row train tiles per pass (even).
// u2_knn uses <32, 10>; a longer list needs fewer tiles per pass to stay within the 160 KB of LDS.
#pragma once
#include <limits.h>

#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int KN_ROWS = 128;   // query rows per workgroup (32 per wave)
constexpr int KN_BD = 16;      // dims per staged chunk
constexpr int KN_PITCH = 17;   // padded LDS row pitch (floats)
constexpr int KN_MEAN_SLICES = 64;

template <int TILES>
constexpr int kn_stage_floats() { return (KN_ROWS + TILES * 32) * KN_PITCH; }  // one staging buffer (query + train chunk)

template <int KMAX, int TILES>
constexpr size_t kn_lds_bytes() {
  return 4 * (2 * (size_t)kn_stage_floats<TILES>()  // two staging buffers
              + 2 * KN_ROWS * (KMAX + 1)            // topv, topj
              + 2 * KN_ROWS * 32                    // qv, qj
              + 2 * KN_ROWS);                       // qcnt, thr
}

// partial[s][d] = sum over the rows of slice s of the finite y[.][d]  (fixed order: deterministic).  A NaN or Inf element is
// left out: the translation point is arbitrary (distances do not depend on it), and a mean poisoned by one bad train row
// would turn every key of every row into NaN.  Left out, only the bad row's own key is NaN or +Inf, which never passes the
// threshold: the row is never ranked, as torch.sort and Kmin_argKmin never rank it.
__global__ __launch_bounds__(256) void knn_colsum_kernel(const float* __restrict__ y, float* __restrict__ partial, int D, int N) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const int per = (N + KN_MEAN_SLICES - 1) / KN_MEAN_SLICES;
  const int r0 = blockIdx.y * per, r1 = min(N, r0 + per);
  float s = 0.f;
  if (d < D)
    for (int r = r0 + w; r < r1; r += 4) { const float v = y[(size_t)r * D + d]; if (isfinite(v)) s += v; }
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && d < D) partial[(size_t)blockIdx.y * D + d] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ void knn_colmean_kernel(const float* __restrict__ partial, float* __restrict__ mu, int D, int N) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  float s = 0.f;
  for (int i = 0; i < KN_MEAN_SLICES; ++i) s += partial[(size_t)i * D + d];
  mu[d] = s / (float)N;
}

__global__ __launch_bounds__(256) void knn_rownorm_kernel(const float* __restrict__ y, const float* __restrict__ mu,
                                                          float* __restrict__ yn, int D, int N) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= N) return;
  float s = 0.f;
  for (int d = threadIdx.x & 63; d < D; d += 64) { const float v = y[(size_t)j * D + d] - mu[d]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) yn[j] = s;
}

__device__ __forceinline__ bool kn_less(float v, int j, float bv, int bj) { return v < bv || (v == bv && j < bj); }

template <int KMAX, int TILES>
__global__ __launch_bounds__(256, 1) void knn_select_kernel(const float* __restrict__ xq, const float* __restrict__ xt,
                                                            const float* __restrict__ tn, const float* __restrict__ mu,
                                                            int* __restrict__ cand, int Nq, int Nt, int D, int KK) {
  static_assert(TILES % 2 == 0, "train rows are staged as TILES / 2 float4 per thread");
  constexpr int KN_TILES = TILES;
  constexpr int KN_LP = KMAX + 1;  // padded pitch of the per-row lists
  constexpr int KN_STAGE = kn_stage_floats<TILES>();
  constexpr int NCR = TILES / 2;   // staged train float4 per thread and chunk
  extern __shared__ float kn_lds[];
  float* stage = kn_lds;  // [2][xs: KN_ROWS x KN_PITCH | cs: TILES * 32 x KN_PITCH]
  float* topv = stage + 2 * KN_STAGE;
  int* topj = reinterpret_cast<int*>(topv + KN_ROWS * KN_LP);
  float* qv = reinterpret_cast<float*>(topj + KN_ROWS * KN_LP);
  int* qj = reinterpret_cast<int*>(qv + KN_ROWS * 32);
  int* qcnt = qj + KN_ROWS * 32;
  float* thr = reinterpret_cast<float*>(qcnt + KN_ROWS);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int p0 = blockIdx.x * KN_ROWS;
  const int li = lane & 31, lk = lane >> 5;

  for (int i = tid; i < KN_ROWS * KN_LP; i += 256) { topv[i] = INFINITY; topj[i] = INT_MAX; }
  if (tid < KN_ROWS) { qcnt[tid] = 0; thr[tid] = INFINITY; }
  float thr_reg[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) thr_reg[r] = INFINITY;

  for (int k0 = 0; k0 < Nt; k0 += KN_TILES * 32) {
    const int ntile = min(KN_TILES, (Nt - k0 + 31) / 32);
    f32x16 acc[KN_TILES];
#pragma unroll
    for (int t = 0; t < KN_TILES; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // Staging registers for one 16-dim chunk: 128 query rows + TILES * 32 train rows x 4 float4 per row over 256 threads.
    // Rows past the end are clamped to the last row instead of predicated (they are never ranked): the loads stay
    // straight-line code, so the compiler can count them (s_waitcnt vmcnt(N)) instead of draining everything at a join.
    struct Chunk { float4 xr[2], cr[NCR], m; };
    const int c4 = tid & 3;  // every float4 index f = q * 256 + tid below has f % 4 == tid % 4
    const float* xrow[2];
    const float* crow[NCR];
#pragma unroll
    for (int q = 0; q < 2; ++q) xrow[q] = xq + (size_t)min(p0 + ((q * 256 + tid) >> 2), Nq - 1) * D + c4 * 4;
#pragma unroll
    for (int q = 0; q < NCR; ++q) crow[q] = xt + (size_t)min(k0 + ((q * 256 + tid) >> 2), Nt - 1) * D + c4 * 4;
    auto gload = [&](Chunk& R, int d0) {
      R.m = *reinterpret_cast<const float4*>(mu + d0 + c4 * 4);
#pragma unroll
      for (int q = 0; q < 2; ++q) R.xr[q] = *reinterpret_cast<const float4*>(xrow[q] + d0);
#pragma unroll
      for (int q = 0; q < NCR; ++q) R.cr[q] = *reinterpret_cast<const float4*>(crow[q] + d0);
    };
    auto lstore = [&](const Chunk& R, int buf) {
      float* xs = stage + buf * KN_STAGE;
      float* cs = xs + KN_ROWS * KN_PITCH;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int f = q * 256 + tid;
        float* dst = xs + (f >> 2) * KN_PITCH + (f & 3) * 4;  // translated by the column mean here, not at load time:
        dst[0] = R.xr[q].x - R.m.x; dst[1] = R.xr[q].y - R.m.y;  // the loads stay in flight across the MFMA sequence
        dst[2] = R.xr[q].z - R.m.z; dst[3] = R.xr[q].w - R.m.w;
      }
#pragma unroll
      for (int q = 0; q < NCR; ++q) {
        const int f = q * 256 + tid;
        float* dst = cs + (f >> 2) * KN_PITCH + (f & 3) * 4;
        dst[0] = R.cr[q].x - R.m.x; dst[1] = R.cr[q].y - R.m.y; dst[2] = R.cr[q].z - R.m.z; dst[3] = R.cr[q].w - R.m.w;
      }
    };

    // One barrier per 16-dim chunk and a global prefetch one full chunk ahead: late in the MFMA sequence of chunk c the
    // registers holding chunk c + 1 (requested at the same point of chunk c - 1) move into the other LDS buffer (its
    // readers finished before the previous barrier) and are immediately re-used to request chunk c + 2.  The LDS operands
    // of step ks + 1 are read while the TILES MFMAs of step ks run; full passes (all train tiles present) carry no per-tile
    // branch.
    auto dloop = [&](auto full) {
      constexpr bool FULL = decltype(full)::value;
      Chunk R;
      gload(R, 0);
      lstore(R, 0);
      if (KN_BD < D) gload(R, KN_BD);
      __syncthreads();
      int buf = 0;
      for (int d0 = 0; d0 < D; d0 += KN_BD, buf ^= 1) {
        const bool more = d0 + KN_BD < D;
        const float* xa = stage + buf * KN_STAGE + (w * 32 + li) * KN_PITCH + lk;
        const float* cb = stage + buf * KN_STAGE + KN_ROWS * KN_PITCH + li * KN_PITCH + lk;
        float a = xa[0], b[KN_TILES];
#pragma unroll
        for (int t = 0; t < KN_TILES; ++t) b[t] = (FULL || t < ntile) ? cb[t * 32 * KN_PITCH] : 0.f;
#pragma unroll
        for (int ks = 0; ks < KN_BD / 2; ++ks) {
          float an = 0.f, bn[KN_TILES];
          if (ks + 1 < KN_BD / 2) {
            an = xa[(ks + 1) * 2];
#pragma unroll
            for (int t = 0; t < KN_TILES; ++t) bn[t] = (FULL || t < ntile) ? cb[t * 32 * KN_PITCH + (ks + 1) * 2] : 0.f;
          }
          if (ks == KN_BD / 2 - 3 && more) {
            lstore(R, buf ^ 1);
            if (d0 + 2 * KN_BD < D) gload(R, d0 + 2 * KN_BD);
          }
#pragma unroll
          for (int t = 0; t < KN_TILES; ++t)
            if (FULL || t < ntile) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[t], acc[t], 0, 0, 0);
          if (ks + 1 < KN_BD / 2) {
            a = an;
#pragma unroll
            for (int t = 0; t < KN_TILES; ++t) b[t] = bn[t];
          }
        }
        __syncthreads();
      }
    };
    if (ntile == KN_TILES) dloop(std::true_type{}); else dloop(std::false_type{});
    // D[i = query][j = train]: lane holds column j = li of tile t, rows (r&3) + 8*(r>>2) + 4*lk of its wave's 32
#pragma unroll
    for (int t = 0; t < KN_TILES; ++t) {
      if (t < ntile) {
        const int j = k0 + t * 32 + li;
        const float tj = (j < Nt) ? tn[j] : 0.f;
        int any = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = tj - 2.f * acc[t][r];
          if (j < Nt && v < thr_reg[r]) {
            const int row = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            const int slot = atomicAdd(&qcnt[row], 1);  // at most 32 per row and tile: one per column
            qv[row * 32 + slot] = v;
            qj[row * 32 + slot] = j;
            any = 1;
          }
        }
        if (__syncthreads_or(any)) {
          if (tid < KN_ROWS) {
            const int n = qcnt[tid];
            float* tv = topv + tid * KN_LP;
            int* tj2 = topj + tid * KN_LP;
            float th = tv[KK - 1];
            int thj = tj2[KK - 1];
            for (int c = 0; c < n; ++c) {
              const float v = qv[tid * 32 + c];
              const int jj = qj[tid * 32 + c];
              if (!kn_less(v, jj, th, thj)) continue;
              int pos = KK - 1;
              while (pos > 0) {
                const float pv = tv[pos - 1];
                const int pj = tj2[pos - 1];
                if (!kn_less(v, jj, pv, pj)) break;
                tv[pos] = pv;
                tj2[pos] = pj;
                --pos;
              }
              tv[pos] = v;
              tj2[pos] = jj;
              th = tv[KK - 1];
              thj = tj2[KK - 1];
            }
            qcnt[tid] = 0;
            thr[tid] = th;
          }
          __syncthreads();
#pragma unroll
          for (int r = 0; r < 16; ++r) thr_reg[r] = thr[w * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
        }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < KN_ROWS * KK; i += 256) {
    const int row = i / KK, k = i % KK;
    if (p0 + row < Nq) cand[(size_t)(p0 + row) * KK + k] = topj[row * KN_LP + k];
  }
}

}  // namespace
