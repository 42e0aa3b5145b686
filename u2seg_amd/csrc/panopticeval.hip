// Panoptic quality on the device (gfx950): the joint histogram of (ground-truth segment, predicted segment) over the pixels of
// an image, which is all that PQ takes from the pixels.  Contract: include/u2seg_hip.h, design: DESIGN.md section 12.
//
// An image is read as one flat run of H * W pixels (4 bytes of predicted id + 3 bytes of png colour, or 4 bytes of
// ground-truth id), so the width plays no part in the addressing: with 16-byte aligned bases a piece of 16 pixels is 64 + 48
// aligned bytes whatever W is, and only the image's last, partial piece is read pixel by pixel.  Everything is integer work: no
// result depends on the order of an addition.
#include "common.h"
#include "u2seg_hip.h"

namespace {

constexpr int PQ_THREADS = 256;
constexpr int PQ_RUN = 16;                       // consecutive pixels a thread owns per tile
constexpr int PQ_TILE = PQ_THREADS * PQ_RUN;     // pixels a work-group handles per step
constexpr int PQ_MAXIMG = 32;                    // 32 x 56 bytes of kernel arguments
constexpr int PQ_MAXSTRIPES = 64;                // work-groups per image at most
constexpr int PQ_TILES_PER_WG = 4;               // ... and at least this many tiles each, so that folding a table pays
constexpr int PQ_LDS_TABLE = 1024;               // ground-truth ids searched in LDS (a longer table is searched in global memory)
constexpr int PQ_LDS_COUNTS = 15 * 1024;         // table entries accumulated in LDS: 60 KB + 4 KB of ids = 64 KB, two work-groups per CU
struct PairCountBatch { U2PanopticPairImage im[PQ_MAXIMG]; };

// row of a ground-truth id: 0 = void, 1 + its index in the ascending table, G + 1 = not listed
template <class T>
__device__ __forceinline__ int pq_row(T tab, int G, int id) {
  if (id == 0) return 0;
  int lo = 0, hi = G;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (tab[m] < id) lo = m + 1; else hi = m;
  }
  return (lo < G && tab[lo] == id) ? lo + 1 : G + 1;
}

// counts and the out-of-range counters of a group of images; grid (stripes, images)
__global__ __launch_bounds__(PQ_THREADS) void pair_clear_kernel(const PairCountBatch batch, int* __restrict__ out_of_range) {
  const U2PanopticPairImage im = batch.im[blockIdx.y];
  const long long n = (long long)(im.G + 2) * im.P;
  for (long long i = (long long)blockIdx.x * PQ_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PQ_THREADS) im.counts[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_of_range[blockIdx.y] = 0;
}

// grid (stripes, images); dynamic LDS: [ids of the table | counts] of the image of the group that needs most.
// Panoptic maps are large uniform regions: a thread walks PQ_RUN consecutive pixels and keeps (row, table entry, run length) in
// registers, so it sends one atomic per change of pair and searches the id table once per change of ground-truth id.
__global__ __launch_bounds__(PQ_THREADS) void pair_counts_kernel(const PairCountBatch batch, int* __restrict__ out_of_range) {
  extern __shared__ int pq_lds[];
  const U2PanopticPairImage im = batch.im[blockIdx.y];
  const long long hw = (long long)im.H * im.W;
  const long long ntiles = (hw + PQ_TILE - 1) / PQ_TILE;
  if ((long long)blockIdx.x >= ntiles) return;  // the whole work-group: before any barrier
  const int G = im.G, P = im.P, tid = (int)threadIdx.x;
  const long long n = (long long)(G + 2) * P;
  const bool tab_lds = G <= PQ_LDS_TABLE, cnt_lds = n <= PQ_LDS_COUNTS;
  int* const tab = pq_lds;
  int* const cnt = pq_lds + (tab_lds ? G : 0);
  if (tab_lds)
    for (int i = tid; i < G; i += PQ_THREADS) tab[i] = im.gt_table[i];
  if (cnt_lds)
    for (int i = tid; i < (int)n; i += PQ_THREADS) cnt[i] = 0;
  __syncthreads();

  int last_id = 0, row = 0, key = -1, run = 0, bad = 0;
  auto flush = [&]() {
    if (key >= 0) {
      if (cnt_lds) atomicAdd(&cnt[key], run); else atomicAdd(&im.counts[key], run);
    }
  };
  auto pixel = [&](int id, int p) {
    if (id != last_id) {
      last_id = id;
      row = tab_lds ? pq_row(tab, G, id) : pq_row(im.gt_table, G, id);
    }
    const bool ok = (unsigned)p < (unsigned)P;  // checked before anything is indexed with p
    bad += ok ? 0 : 1;
    const int k = ok ? row * P + p : -1;
    if (k != key) {
      flush();
      key = k;
      run = 0;
    }
    ++run;
  };

  const uint8_t* gt8 = reinterpret_cast<const uint8_t*>(im.gt);
  const int* gt32 = reinterpret_cast<const int*>(im.gt);
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long p0 = tile * PQ_TILE + (long long)tid * PQ_RUN;
    if (p0 + PQ_RUN <= hw) {  // a whole piece: 16-byte loads, all of them inside the image
      unsigned pr[PQ_RUN], id[PQ_RUN];
#pragma unroll
      for (int e = 0; e < PQ_RUN / 4; ++e) {
        const uint4 v = *reinterpret_cast<const uint4*>(im.pred + p0 + 4 * e);
        pr[4 * e] = v.x; pr[4 * e + 1] = v.y; pr[4 * e + 2] = v.z; pr[4 * e + 3] = v.w;
      }
      if (im.gt_is_ids) {
#pragma unroll
        for (int e = 0; e < PQ_RUN / 4; ++e) {
          const uint4 v = *reinterpret_cast<const uint4*>(gt32 + p0 + 4 * e);
          id[4 * e] = v.x; id[4 * e + 1] = v.y; id[4 * e + 2] = v.z; id[4 * e + 3] = v.w;
        }
      } else {
        unsigned w[PQ_RUN * 3 / 4 + 1];
#pragma unroll
        for (int e = 0; e < PQ_RUN * 3 / 16; ++e) {
          const uint4 v = *reinterpret_cast<const uint4*>(gt8 + 3 * p0 + 16 * e);
          w[4 * e] = v.x; w[4 * e + 1] = v.y; w[4 * e + 2] = v.z; w[4 * e + 3] = v.w;
        }
        w[PQ_RUN * 3 / 4] = 0u;
#pragma unroll
        for (int e = 0; e < PQ_RUN; ++e) {  // bytes 3 e .. 3 e + 2, little endian = R + 256 G + 65536 B
          const int s = (24 * e) & 31, j = (24 * e) >> 5;
          const unsigned v = s <= 8 ? (w[j] >> s) : ((w[j] >> s) | (w[j + 1] << (32 - s)));
          id[e] = v & 0xffffffu;
        }
      }
#pragma unroll
      for (int e = 0; e < PQ_RUN; ++e) pixel((int)id[e], (int)pr[e]);
    } else {  // the image's last piece: pixel by pixel, nothing past the end is read
      for (long long p = p0; p < hw; ++p) {
        const int v = im.gt_is_ids ? gt32[p]
                                   : (int)((unsigned)gt8[3 * p] | ((unsigned)gt8[3 * p + 1] << 8) | ((unsigned)gt8[3 * p + 2] << 16));
        pixel(v, im.pred[p]);
      }
    }
  }
  flush();
  bad = wave_isum(bad);
  if ((tid & 63) == 0 && bad) atomicAdd(&out_of_range[blockIdx.y], bad);
  if (cnt_lds) {
    __syncthreads();
    for (int i = tid; i < (int)n; i += PQ_THREADS) {
      const int v = cnt[i];
      if (v) atomicAdd(&im.counts[i], v);
    }
  }
}

}  // namespace

extern "C" int u2_panoptic_pair_lds_ints(void) { return PQ_LDS_COUNTS; }

extern "C" int u2_panoptic_pair_counts(const U2PanopticPairImage* images, int n_images, int* out_of_range, void* stream) {
  if (n_images <= 0) return 0;
  if (!images || !out_of_range) return -1;
  for (int i = 0; i < n_images; ++i) {
    const U2PanopticPairImage& m = images[i];
    if (m.H < 0 || m.W < 0 || m.G < 0 || m.P < 1 || !m.counts || (m.G > 0 && !m.gt_table)) return -1;
    const long long hw = (long long)m.H * m.W;
    if (hw >= (1LL << 31) || (long long)(m.G + 2) * m.P >= (1LL << 31)) return -1;
    if (hw > 0 && (!m.pred || !m.gt || ((uintptr_t)m.pred & 15) || ((uintptr_t)m.gt & 15))) return -1;
  }
  const hipStream_t s = (hipStream_t)stream;
  for (int i0 = 0; i0 < n_images; i0 += PQ_MAXIMG) {
    PairCountBatch b;
    const int nb = n_images - i0 < PQ_MAXIMG ? n_images - i0 : PQ_MAXIMG;
    long long max_tiles = 0, max_n = 0;
    int lds_ints = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i] = images[i0 + i];
      const long long tiles = ((long long)b.im[i].H * b.im[i].W + PQ_TILE - 1) / PQ_TILE;
      const long long n = (long long)(b.im[i].G + 2) * b.im[i].P;
      const int need = (b.im[i].G <= PQ_LDS_TABLE ? b.im[i].G : 0) + (n <= PQ_LDS_COUNTS ? (int)n : 0);
      if (tiles > max_tiles) max_tiles = tiles;
      if (n > max_n) max_n = n;
      if (need > lds_ints) lds_ints = need;
    }
    long long cs = (max_n + 4 * PQ_THREADS - 1) / (4 * PQ_THREADS);
    cs = cs < 1 ? 1 : (cs > 256 ? 256 : cs);
    hipLaunchKernelGGL(pair_clear_kernel, dim3((unsigned)cs, nb), dim3(PQ_THREADS), 0, s, b, out_of_range + i0);
    U2_CHECK_LAUNCH();
    if (max_tiles == 0) continue;
    long long stripes = (max_tiles + PQ_TILES_PER_WG - 1) / PQ_TILES_PER_WG;
    stripes = stripes > PQ_MAXSTRIPES ? PQ_MAXSTRIPES : stripes;
    hipLaunchKernelGGL(pair_counts_kernel, dim3((unsigned)stripes, nb), dim3(PQ_THREADS), (size_t)lds_ints * sizeof(int), s, b,
                       out_of_range + i0);
    U2_CHECK_LAUNCH();
  }
  return 0;
}
