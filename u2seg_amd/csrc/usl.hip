// Selection regularizer of USL's regularised representative selection (one iteration's update of `reg`).
//
// Replaces the update step of get_selection_with_reg_imagenet in
// u2seg/Instance_Clustering/shared/utils/nn_utils_imagenet.py:147-212 (pykeops):
//   v[i][0..H)  = the H smallest sum_d (x_id - sel_jd)^2 over the S selected rows j, ascending (ties: smaller j first)
//   mask        exclude_same_cluster: v = 1e10 where the POSITION j equals label[i] (the reference compares positions in
//               the selection with cluster ids); otherwise v = 1e10 where v == 0.  A remaining 0 is the reference's
//               AssertionError: counted in *zero_count (rows), the caller raises.
//   new[i]      sum_k 1 / v[i][k]            (alpha == 1)
//               sum_k 1 / v[i][k] ** alpha   (otherwise; ** 0.5 is sqrt and ** 2 a product, as torch evaluates them)
//   reg_out[i]  reg_in[i] * momentum + new[i] * one_minus_momentum   (separate fp32 products and sum, no fma)
//
// Two kernels, the method of knn.hip:
//   select  knn_select_kernel<68, 8> (knn_select.h): 128 rows per workgroup against every selected row on the exact-fp32
//           MFMA in the mean-translated expanded form, a sorted list of KK = H + 4 candidates per row (8 train tiles per
//           pass instead of knn's 10, so that lists of up to 68 fit in LDS next to the staging buffers).
//   refine  one wave per row: the difference-form distance of each candidate (lanes over d, a fixed butterfly), rank by
//           (distance, position), then the mask, the power sum over the first H and the momentum blend.  Only reg_out and
//           the zero count leave the kernel; the candidate lists are workspace.
// The 4 spare candidates absorb the rounding difference between the two formulations at the H-th / (H+1)-th boundary.
// A selected row with a NaN or Inf element is left out of the column mean and never becomes a candidate (knn_select.h).
#include "knn_select.h"
#include "u2seg_hip.h"

namespace {

constexpr int US_TILES = 8;
constexpr int US_KMAX = 68;
constexpr int US_SPARE = 4;
constexpr int US_HMAX = US_KMAX - US_SPARE;  // 64
constexpr size_t US_LDS_BYTES = kn_lds_bytes<US_KMAX, US_TILES>();
static_assert(US_LDS_BYTES <= 160 * 1024, "the select kernel's LDS exceeds a CU's 160 KB");

__global__ __launch_bounds__(256) void usl_refine_kernel(const float* __restrict__ x, const float* __restrict__ sel,
                                                         const int* __restrict__ cand, const long long* __restrict__ labels,
                                                         const float* __restrict__ reg_in, float* __restrict__ reg_out,
                                                         int* __restrict__ zero_count, int N, int D, int KK, int H, float alpha,
                                                         float momentum, float one_minus_momentum, int exclude) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* xi = x + (size_t)row * D;
  const int* cr = cand + (size_t)row * KK;
  // candidate k ends in lane k (slot 0) or lane k - 64 (slot 1); the wave sums each candidate's distance with coalesced
  // 16-byte loads: every lane adds its float4 chunks of d in order, then a fixed butterfly (deterministic)
  float d0 = INFINITY, d1 = INFINITY;
  int j0 = INT_MAX, j1 = INT_MAX;
  for (int k = 0; k < KK; ++k) {
    const int j = cr[k];
    float s = INFINITY;
    if (j != INT_MAX) {
      const float* yj = sel + (size_t)j * D;
      s = 0.f;
      for (int d = lane * 4; d < D; d += 256) {
        const float4 a = *reinterpret_cast<const float4*>(xi + d);
        const float4 b = *reinterpret_cast<const float4*>(yj + d);
        float t;
        t = a.x - b.x; s += t * t;
        t = a.y - b.y; s += t * t;
        t = a.z - b.z; s += t * t;
        t = a.w - b.w; s += t * t;
      }
      s = wave_sum(s);
    }
    if (lane == (k & 63)) {
      if (k < 64) { d0 = s; j0 = j; } else { d1 = s; j1 = j; }
    }
  }
  int r0 = 0, r1 = 0;
  for (int k = 0; k < KK; ++k) {
    const float od = k < 64 ? __shfl(d0, k, 64) : __shfl(d1, k - 64, 64);
    const int oj = k < 64 ? __shfl(j0, k, 64) : __shfl(j1, k - 64, 64);
    r0 += kn_less(od, oj, d0, j0) ? 1 : 0;
    r1 += kn_less(od, oj, d1, j1) ? 1 : 0;
  }
  const long long lab = labels[row];
  int zero = 0;
  auto term = [&](float v, int j, int r) -> float {
    if (r >= H || j == INT_MAX) return 0.f;
    if (exclude) {
      if ((long long)j == lab) v = 1e10f;
    } else if (v == 0.f) {
      v = 1e10f;
    }
    zero |= v == 0.f;
    if (alpha == 1.f) return 1.f / v;
    const float p = alpha == 0.5f ? sqrtf(v) : (alpha == 2.f ? v * v : powf(v, alpha));
    return 1.f / p;
  };
  const float s = wave_sum(term(d0, j0, r0) + term(d1, j1, r1));
  const bool any_zero = __any(zero);
  if (lane == 0) {
    reg_out[row] = reg_in[row] * momentum + s * one_minus_momentum;
    if (any_zero) atomicAdd(zero_count, 1);
  }
}

__host__ inline long long us_round4(long long n) { return (n + 3) & ~3LL; }

}  // namespace

extern "C" int u2_usl_reg_workspace_ints(int N, int S, int D, int H, long long* n_ints) {
  if (H < 1 || H > US_HMAX || N < 0 || S < 1 || D < 1 || !n_ints) return -1;
  const int KK = H + US_SPARE;
  // |sel_j - mu|^2 (fp32), candidate lists (int32), column mean and its partial sums (fp32); each part 16-byte aligned
  *n_ints = us_round4(S) + us_round4((long long)N * KK) + (long long)(KN_MEAN_SLICES + 1) * D;
  return 0;
}

extern "C" int u2_usl_regularizer(const float* x, const float* sel, const long long* labels, const float* reg_in, float* reg_out,
                                  int* zero_count, void* workspace, int N, int S, int D, int H, float alpha, float momentum,
                                  float one_minus_momentum, int exclude_same_cluster, void* stream) {
  if (H < 1 || H > US_HMAX || D < KN_BD || D % KN_BD != 0 || N < 0 || !workspace || !zero_count) return -1;
  if (S < H) return -2;
  if (N == 0) return 0;
  const int KK = H + US_SPARE;
  hipStream_t s = (hipStream_t)stream;
  float* tn = reinterpret_cast<float*>(workspace);
  int* cand = reinterpret_cast<int*>(workspace) + us_round4(S);
  float* mu = reinterpret_cast<float*>(cand + us_round4((long long)N * KK));  // read as float4
  float* partial = mu + D;
  hipLaunchKernelGGL(knn_colsum_kernel, dim3((D + 63) / 64, KN_MEAN_SLICES), dim3(256), 0, s, sel, partial, D, S);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_colmean_kernel, dim3((D + 255) / 256), dim3(256), 0, s, partial, mu, D, S);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_rownorm_kernel, dim3((S + 3) / 4), dim3(256), 0, s, sel, mu, tn, D, S);
  U2_CHECK_LAUNCH();
  hipError_t e = hipFuncSetAttribute((const void*)knn_select_kernel<US_KMAX, US_TILES>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)US_LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((knn_select_kernel<US_KMAX, US_TILES>), dim3((N + KN_ROWS - 1) / KN_ROWS), dim3(256), US_LDS_BYTES, s, x,
                     sel, tn, mu, cand, N, S, D, KK);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(usl_refine_kernel, dim3((N + 3) / 4), dim3(256), 0, s, x, sel, cand, labels, reg_in, reg_out, zero_count, N,
                     D, KK, H, alpha, momentum, one_minus_momentum, exclude_same_cluster);
  U2_CHECK_LAUNCH();
  return 0;
}
