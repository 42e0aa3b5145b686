// Brute-force k nearest neighbours over fp32 embeddings (first-order density estimate before k-means).
//
// Replaces kNN / partitioned_kNN in u2seg/Instance_Clustering/shared/utils/nn_utils.py:204-299:
//   D_ij = sum_d (x_test_id - x_train_jd)^2;  d_knn, ind_knn = D_ij.Kmin_argKmin(K, dim=1)       (:210-218, pykeops)
//   the reference tiles both sides in partitions of 130 000 rows to fit its GPU and merges the per-partition lists by
//   an argsort (:226-266); the merged result is the global K smallest per row (its own verify branch asserts that,
//   :268-287).  With 288 GB of HBM the whole train set stays resident and one pass produces the global lists.
//
// Two kernels:
//   select  for 128 query rows per workgroup, stream every train row through LDS; dot products on the exact-fp32 MFMA
//           (v_mfma_f32_32x32x2_f32, an fma chain in k order); rank key |y_j|^2 - 2 x_i.y_j (|x_i|^2 is constant per
//           row), evaluated on rows translated by the train set's column mean (distances do not change, the cancellation
//           in the expanded form shrinks from |x|^2 to the spread of the data; the translation happens while staging).
//           A per-row threshold (current KK-th smallest) filters the tile; survivors go through a per-row LDS queue into
//           a per-row sorted list of KK = K + 4 candidates.
//   refine  one wave per query row: recomputes sum_d (x - y)^2 for the KK candidates in the reference's difference form
//           (no cancellation; the row's own distance is exactly 0), ranks them by (distance, index) and writes the first K.
// The 4 spare candidates absorb the rounding difference between the two formulations at the K-th / (K+1)-th boundary.
// Non-finite rows: a train row with a NaN or Inf element is left out of the column mean (knn_colsum_kernel), its own key is
// NaN or +Inf and never passes the threshold, so it is in nobody's list; a query row with one is skipped by the refine
// kernel.  d_knn / ind_knn are written for ranked neighbours only: every other slot keeps what the caller put there.
// The select kernel lives in knn_select.h (instantiated here as <32, 10>); usl.hip uses a longer list of the same kernel.
#include "knn_select.h"
#include "u2seg_hip.h"

namespace {

constexpr int KN_TILES = 10;   // 32-row train tiles per pass (320 train rows)
constexpr int KN_KMAX = 32;    // candidate list capacity
constexpr int KN_SPARE = 4;
constexpr size_t KN_LDS_BYTES = kn_lds_bytes<KN_KMAX, KN_TILES>();

// One wave per query row: exact difference-form distances of its KK candidates, rank by (distance, index), keep K.
__global__ __launch_bounds__(256) void knn_refine_kernel(const float* __restrict__ xq, const float* __restrict__ xt,
                                                         const int* __restrict__ cand, float* __restrict__ d_knn,
                                                         long long* __restrict__ ind_knn, int Nq, int D, int KK, int K) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= Nq) return;
  const float* xi = xq + (size_t)row * D;
  // A query row with a NaN or Inf element has no ranked neighbour: its slots are left as the caller filled them.  (NaN keys
  // never pass the select stage's threshold, but an Inf element gives keys of -Inf wherever the train element is larger than
  // the mean, and those do.)
  bool finite = true;
  for (int d = lane; d < D; d += 64) finite &= isfinite(xi[d]);
  if (!__all(finite)) return;
  float my_d = INFINITY;
  int my_j = INT_MAX;
  for (int k = 0; k < KK; ++k) {
    const int j = cand[(size_t)row * KK + k];
    float s = INFINITY;
    if (j != INT_MAX) {
      const float* yj = xt + (size_t)j * D;
      s = 0.f;
      for (int d = lane; d < D; d += 64) { const float df = xi[d] - yj[d]; s += df * df; }
      s = wave_sum(s);
    }
    if (lane == k) { my_d = s; my_j = j; }
  }
  int rank = 0;
  for (int k = 0; k < KK; ++k) {
    const float od = __shfl(my_d, k, 64);
    const int oj = __shfl(my_j, k, 64);
    rank += kn_less(od, oj, my_d, my_j) ? 1 : 0;
  }
  if (lane < KK && rank < K && my_j != INT_MAX) {
    d_knn[(size_t)row * K + rank] = my_d;
    ind_knn[(size_t)row * K + rank] = (long long)my_j;
  }
}

}  // namespace

extern "C" int u2_knn_workspace_ints(int Nq, int Nt, int D, int K, long long* n_ints) {
  if (K < 1 || K + KN_SPARE > KN_KMAX || D < 1 || !n_ints) return -1;
  const int KK = K + KN_SPARE;
  // |y_j - mu|^2 (fp32), candidate lists (int32), column mean and its partial sums (fp32)
  *n_ints = (long long)Nt + (long long)Nq * KK + (long long)(KN_MEAN_SLICES + 1) * D;
  return 0;
}

extern "C" int u2_knn(const float* x_query, const float* x_train, void* workspace, float* d_knn, long long* ind_knn, int Nq,
                      int Nt, int D, int K, void* stream) {
  if (K < 1 || K + KN_SPARE > KN_KMAX || D < KN_BD || D % KN_BD != 0 || !workspace) return -1;
  if (Nt < K) return -2;  // the reference assumes every partition holds at least K rows (nn_utils.py:236)
  if (Nq <= 0) return 0;
  const int KK = K + KN_SPARE;
  hipStream_t s = (hipStream_t)stream;
  float* tn = reinterpret_cast<float*>(workspace);
  int* cand = reinterpret_cast<int*>(workspace) + Nt;
  float* mu = reinterpret_cast<float*>(cand + (size_t)Nq * KK);
  float* partial = mu + D;
  hipLaunchKernelGGL(knn_colsum_kernel, dim3((D + 63) / 64, KN_MEAN_SLICES), dim3(256), 0, s, x_train, partial, D, Nt);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_colmean_kernel, dim3((D + 255) / 256), dim3(256), 0, s, partial, mu, D, Nt);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_rownorm_kernel, dim3((Nt + 3) / 4), dim3(256), 0, s, x_train, mu, tn, D, Nt);
  U2_CHECK_LAUNCH();
  hipError_t e = hipFuncSetAttribute((const void*)knn_select_kernel<KN_KMAX, KN_TILES>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)KN_LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((knn_select_kernel<KN_KMAX, KN_TILES>), dim3((Nq + KN_ROWS - 1) / KN_ROWS), dim3(256), KN_LDS_BYTES, s,
                     x_query, x_train, tn, mu, cand, Nq, Nt, D, KK);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(knn_refine_kernel, dim3((Nq + 3) / 4), dim3(256), 0, s, x_query, x_train, cand, d_knn, ind_knn, Nq, D, KK,
                     K);
  U2_CHECK_LAUNCH();
  return 0;
}
