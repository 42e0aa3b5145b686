// Boundary IoU of the semantic evaluation on the device (gfx950): the confusion matrix of the boundary maps of prediction and
// ground truth, and the plain confusion matrix from the same read.  Contract: include/u2seg_hip.h, design: DESIGN.md section 16.
//
// boundary(m) = m - erode(m), erode(m) = minimum over the (2 d + 1) x (2 d + 1) window with everything outside the image 0.
// Fused path (d <= SB_DMAX): a work-group owns a 64 x 64 tile.  It loads the tile of both maps plus a halo of d into LDS as
// packed bytes (zeros outside the image, the LUT applied to the prediction on the way), takes the row minimum, then the column
// minimum, subtracts, and counts both pairs of every pixel in LDS counters, which it folds into the matrices with 64-bit integer
// atomics.  General path (any d): a row-minimum pass into a scratch buffer and a column-minimum pass that counts.
// Everything is integer work: no result depends on the order of an addition.
#include "common.h"
#include "u2seg_hip.h"

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_TILE = 64;                        // output pixels per tile side
constexpr int SB_DMAX = 32;                        // largest halo of the fused path (800 x 1333 needs 31)
constexpr int SB_REG = SB_TILE + 2 * SB_DMAX;      // rows / bytes per row of the largest region
constexpr int SB_RAW_PITCH = 48;                   // dwords per region row: 32 + 16, so that the two rows a half-wave reads in the
                                                   // row pass sit on disjoint banks
constexpr int SB_MIN_PITCH = 20;                   // dwords per row of the row minima: 16 + 4, rows 4 apart on disjoint banks
constexpr int SB_MAXN = 32;
constexpr int SB_RAW_WORDS = SB_REG * SB_RAW_PITCH, SB_MIN_WORDS = SB_REG * SB_MIN_PITCH;
constexpr size_t SB_LDS_BYTES = (size_t)(2 * SB_RAW_WORDS + 2 * SB_MIN_WORDS + 2 * SB_MAXN * SB_MAXN + 64) * 4;
constexpr unsigned SB_EVEN = 0x00ff00ffu;

typedef unsigned short sb_u16x2 __attribute__((ext_vector_type(2)));
// minimum of the two 16-bit halves (v_pk_min_u16); with SB_EVEN-masked operands: of bytes 0 and 2
__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b) {
  const sb_u16x2 r = __builtin_elementwise_min(*reinterpret_cast<const sb_u16x2*>(&a), *reinterpret_cast<const sb_u16x2*>(&b));
  return *reinterpret_cast<const unsigned*>(&r);
}
__device__ __forceinline__ unsigned umin3(unsigned a, unsigned b, unsigned c) { return min(min(a, b), c); }

// Bytes a .. a + 3 of the flat map p[0, n) as one word; a is the index of (row, col) with the row inside the image.  Whole
// dwords are read only where both lie inside the buffer, at their natural alignment (rows are w bytes: a is unaligned for most
// w); the buffer's first and last bytes are read one by one.  With lut: every byte mapped.  Then the bytes whose column is
// outside [0, w) - they belong to the neighbouring rows - become 0.
__device__ __forceinline__ unsigned sb_load4(const uint8_t* __restrict__ p, long long n, long long a, int col, int w,
                                             const uint8_t* lut) {
  if (col + 3 < 0 || col >= w) return 0u;
  const uintptr_t base = (uintptr_t)p, addr = (uintptr_t)((long long)base + a), lo = addr & ~(uintptr_t)3;
  unsigned v = 0u;
  if (a >= 0 && lo >= base && lo + 8 <= base + (uintptr_t)n) {
    const unsigned w0 = *reinterpret_cast<const unsigned*>(lo), w1 = *reinterpret_cast<const unsigned*>(lo + 4);
    v = __builtin_amdgcn_alignbyte(w1, w0, (unsigned)(addr & 3));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i = a + k;
      if (i >= 0 && i < n) v |= (unsigned)p[i] << (8 * k);
    }
  }
  if (lut)
    v = (unsigned)lut[v & 255u] | ((unsigned)lut[(v >> 8) & 255u] << 8) | ((unsigned)lut[(v >> 16) & 255u] << 16) |
        ((unsigned)lut[v >> 24] << 24);
  if (col < 0) v &= 0xffffffffu << (8 * -col);               // col in -3 .. -1
  if (col + 3 >= w) v &= (1u << (8 * (w - col))) - 1u;        // w - col in 1 .. 3
  return v;
}

// A thread's run of equal keys: one LDS atomic per change of key instead of one per pixel (label maps are large uniform areas,
// and the boundary pair of every interior pixel is (0, 0)).
struct SbRun {
  int key = -1, run = 0;
  __device__ __forceinline__ void flush(unsigned* cnt) {
    if (key >= 0) atomicAdd(&cnt[key], (unsigned)run);
  }
  __device__ __forceinline__ void add(unsigned* cnt, int k) {
    if (k != key) {
      flush(cnt);
      key = k;
      run = 0;
    }
    ++run;
  }
};

// grid (tiles along x, tiles along y); dynamic LDS: [region of pred | region of gt | row minima of pred | of gt | counters | lut]
__global__ __launch_bounds__(SB_THREADS) void boundary_fused_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                     const uint8_t* __restrict__ lut, int h, int w, int d, int n,
                                                                     unsigned long long* __restrict__ conf,
                                                                     unsigned long long* __restrict__ bconf) {
  extern __shared__ unsigned sb_lds[];
  unsigned* const raw = sb_lds;                                  // [2][SB_REG][SB_RAW_PITCH]
  unsigned* const hmn = sb_lds + 2 * SB_RAW_WORDS;               // [2][SB_REG][SB_MIN_PITCH]
  unsigned* const cnt = hmn + 2 * SB_MIN_WORDS;                  // [2][n * n]: plain, boundary
  uint8_t* const lut_s = reinterpret_cast<uint8_t*>(cnt + 2 * SB_MAXN * SB_MAXN);
  const int tid = (int)threadIdx.x, nn = n * n;
  const int x0 = (int)blockIdx.x * SB_TILE, y0 = (int)blockIdx.y * SB_TILE;
  const int L = 2 * d + 1;                                       // window
  const int R = SB_TILE + 2 * d;                                 // region rows, and bytes per region row
  const int CD = (R + 3) >> 2;                                   // dwords per region row
  const long long hw = (long long)h * w;

  for (int i = tid; i < 2 * nn; i += SB_THREADS) cnt[i] = 0u;
  if (lut) lut_s[tid] = lut[tid];                                // SB_THREADS == 256 entries
  __syncthreads();

  // ---- load: region (y0 - d, x0 - d) .. of both maps, zeros outside the image
  for (int it = tid; it < 2 * R * CD; it += SB_THREADS) {
    const int m = it >= R * CD, rem = it - m * R * CD, r = rem / CD, c = rem - r * CD;
    const int y = y0 - d + r, col = x0 - d + 4 * c;
    unsigned v = 0u;
    if (y >= 0 && y < h) v = sb_load4(m ? gt : pred, hw, (long long)y * w + col, col, w, (m || !lut) ? nullptr : lut_s);
    raw[m * SB_RAW_WORDS + r * SB_RAW_PITCH + c] = v;
  }
  __syncthreads();

  // ---- row minimum: item = (map, region row r, group g of 4 output columns); out[i] = min of the row's bytes 4 g + i .. + L - 1.
  // Of the bytes k = 0 .. L + 2 behind 4 g, 3 .. L - 1 are in all four windows (whole dwords of them: two packed minima per
  // dword), 0 .. 2 only in the first ones and L .. L + 2 only in the last ones.
  for (int it = tid; it < 2 * R * 16; it += SB_THREADS) {
    const int m = it >= R * 16, rem = it - m * R * 16, r = rem >> 4, g = rem & 15;
    const unsigned* row = raw + m * SB_RAW_WORDS + r * SB_RAW_PITCH + g;
    unsigned a0 = 255u, a1 = 255u, a2 = 255u, b0 = 255u, b1 = 255u, b2 = 255u, cm = 255u;
    auto put = [&](int k, unsigned v) {
      if (k < 3) {
        if (k == 0) a0 = v; else if (k == 1) a1 = v; else a2 = v;
      } else if (k < L) {
        cm = min(cm, v);
      } else if (k < L + 3) {
        if (k == L) b0 = v; else if (k == L + 1) b1 = v; else b2 = v;
      }
    };
    auto bytes = [&](int j) {
      const unsigned v = row[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) put(4 * j + b, (v >> (8 * b)) & 255u);
    };
    bytes(0);
    const int full = L >> 2, nd = (L + 6) >> 2;                  // dwords 1 .. full - 1 hold only common bytes; nd dwords in all
    unsigned ce = SB_EVEN, co = SB_EVEN;
    for (int j = 1; j < full; ++j) {
      const unsigned v = row[j];
      ce = pk_min(ce, v & SB_EVEN);
      co = pk_min(co, (v >> 8) & SB_EVEN);
    }
    for (int j = full < 1 ? 1 : full; j < nd; ++j) bytes(j);
    ce = pk_min(ce, co);
    cm = umin3(cm, ce & 0xffffu, ce >> 16);
    const unsigned o0 = min(cm, umin3(a0, a1, a2)), o1 = min(cm, umin3(a1, a2, b0)), o2 = min(cm, umin3(a2, b0, b1)),
                   o3 = min(cm, umin3(b0, b1, b2));
    hmn[m * SB_MIN_WORDS + r * SB_MIN_PITCH + g] = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
  }
  __syncthreads();

  // ---- column minimum, boundary and counts: a thread owns 4 columns (one dword) x 4 rows; the same split of the L + 3 rows
  // behind its first one, every minimum on even and odd bytes of the dword at once
  {
    const int g = tid & 15, rg = tid >> 4, cb = d + 4 * g;       // cb: byte of the thread's first pixel in a region row
    unsigned bnd[2][4], ctr[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const unsigned* col = hmn + m * SB_MIN_WORDS + (4 * rg) * SB_MIN_PITCH + g;
      unsigned e[6], o[6];                                       // rows 0 .. 2 and L .. L + 2
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const unsigned v = col[(k < 3 ? k : L + k - 3) * SB_MIN_PITCH];
        e[k] = v & SB_EVEN;
        o[k] = (v >> 8) & SB_EVEN;
      }
      unsigned ce = SB_EVEN, co = SB_EVEN;
      for (int k = 3; k < L; ++k) {
        const unsigned v = col[k * SB_MIN_PITCH];
        ce = pk_min(ce, v & SB_EVEN);
        co = pk_min(co, (v >> 8) & SB_EVEN);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {                              // window of output row i: rows i .. 2, the common ones, L .. L + i - 1
        unsigned me = ce, mo = co;
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if ((k < 3 && k >= i) || (k >= 3 && k - 3 < i)) {
            me = pk_min(me, e[k]);
            mo = pk_min(mo, o[k]);
          }
        const unsigned* rrow = raw + m * SB_RAW_WORDS + (d + 4 * rg + i) * SB_RAW_PITCH + (cb >> 2);
        ctr[m][i] = __builtin_amdgcn_alignbyte(rrow[1], rrow[0], (unsigned)(cb & 3));
        bnd[m][i] = ctr[m][i] - (me | (mo << 8));                // eroded <= centre in every byte: no borrow
      }
    }
    SbRun plain, edge;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = y0 + 4 * rg + i;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int x = x0 + 4 * g + b;
        const unsigned p = (ctr[0][i] >> (8 * b)) & 255u, q = (ctr[1][i] >> (8 * b)) & 255u;
        if (y < h && x < w && p < (unsigned)n && q < (unsigned)n) {
          if (conf) plain.add(cnt, (int)(p * n + q));
          edge.add(cnt + nn, (int)(((bnd[0][i] >> (8 * b)) & 255u) * n + ((bnd[1][i] >> (8 * b)) & 255u)));
        }
      }
    }
    plain.flush(cnt);
    edge.flush(cnt + nn);
  }
  __syncthreads();
  for (int i = tid; i < nn; i += SB_THREADS) {
    const unsigned c = cnt[i], e = cnt[nn + i];
    if (c) atomicAdd(&conf[i], (unsigned long long)c);           // c > 0 only with conf
    if (e) atomicAdd(&bconf[i], (unsigned long long)e);
  }
}

// ---- general path: one pixel per thread and step, 2 d + 1 reads each; a window that leaves the image has minimum 0
__global__ __launch_bounds__(SB_THREADS) void boundary_rowmin_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                      const uint8_t* __restrict__ lut, int h, int w, int d,
                                                                      uint8_t* __restrict__ scratch /*[2][h][w]*/) {
  __shared__ uint8_t lut_s[256];
  lut_s[threadIdx.x] = lut ? lut[threadIdx.x] : (uint8_t)threadIdx.x;
  __syncthreads();
  const long long hw = (long long)h * w;
  for (long long i = (long long)blockIdx.x * SB_THREADS + threadIdx.x; i < hw; i += (long long)gridDim.x * SB_THREADS) {
    const int x = (int)(i % w);
    unsigned mp = 0u, mg = 0u;
    if (x >= d && x < w - d) {                                   // x - d >= 0 and x + d <= w - 1, without forming x + d
      mp = mg = 255u;
      for (long long k = i - d; k <= i + d; ++k) {
        mp = min(mp, (unsigned)lut_s[pred[k]]);
        mg = min(mg, (unsigned)gt[k]);
      }
    }
    scratch[i] = (uint8_t)mp;
    scratch[hw + i] = (uint8_t)mg;
  }
}

__global__ __launch_bounds__(SB_THREADS) void boundary_colmin_count_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                                            const uint8_t* __restrict__ lut,
                                                                            const uint8_t* __restrict__ scratch, int h, int w, int d,
                                                                            int n, unsigned long long* __restrict__ conf,
                                                                            unsigned long long* __restrict__ bconf) {
  __shared__ uint8_t lut_s[256];
  __shared__ unsigned cnt[2 * SB_MAXN * SB_MAXN];
  const int tid = (int)threadIdx.x, nn = n * n;
  lut_s[tid] = lut ? lut[tid] : (uint8_t)tid;
  for (int i = tid; i < 2 * nn; i += SB_THREADS) cnt[i] = 0u;
  __syncthreads();
  const long long hw = (long long)h * w;
  for (long long i = (long long)blockIdx.x * SB_THREADS + tid; i < hw; i += (long long)gridDim.x * SB_THREADS) {
    const int y = (int)(i / w);
    unsigned mp = 0u, mg = 0u;
    if (y >= d && y < h - d) {
      mp = mg = 255u;
      for (long long k = i - (long long)d * w; k <= i + (long long)d * w; k += w) {
        mp = min(mp, (unsigned)scratch[k]);
        mg = min(mg, (unsigned)scratch[hw + k]);
      }
    }
    const unsigned p = lut_s[pred[i]], q = gt[i];
    if (p < (unsigned)n && q < (unsigned)n) {
      if (conf) atomicAdd(&cnt[p * n + q], 1u);
      atomicAdd(&cnt[nn + (p - mp) * n + (q - mg)], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < nn; i += SB_THREADS) {
    const unsigned c = cnt[i], e = cnt[nn + i];
    if (c) atomicAdd(&conf[i], (unsigned long long)c);
    if (e) atomicAdd(&bconf[i], (unsigned long long)e);
  }
}

}  // namespace

extern "C" int u2_semseg_boundary_fused_cap(void) { return SB_DMAX; }

extern "C" long long u2_semseg_boundary_scratch_bytes(int h, int w, int d) {
  if (h < 1 || w < 1 || d < 1) return -1;
  return d <= SB_DMAX ? 0 : 2LL * h * w;
}

extern "C" int u2_semseg_boundary_confusion(const void* pred, const void* gt, const void* lut, int h, int w, int d, int n,
                                            long long* conf, long long* bconf, void* scratch, long long scratch_bytes,
                                            void* stream) {
  if (n < 1 || n > SB_MAXN || d < 1 || h < 1 || w < 1 || !pred || !gt || !bconf) return -1;
  const long long hw = (long long)h * w;
  if (hw >= (1LL << 31) || (h + SB_TILE - 1) / SB_TILE > 65535) return -1;
  const hipStream_t s = (hipStream_t)stream;
  const uint8_t *p = (const uint8_t*)pred, *g = (const uint8_t*)gt, *l = (const uint8_t*)lut;
  unsigned long long *c = (unsigned long long*)conf, *b = (unsigned long long*)bconf;
  if (d <= SB_DMAX) {
    static PerDeviceOnce attr_set;
    if (auto once_guard = attr_set.first()) {
      (void)hipFuncSetAttribute((const void*)boundary_fused_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_LDS_BYTES);
    }
    const dim3 grid((unsigned)((w + SB_TILE - 1) / SB_TILE), (unsigned)((h + SB_TILE - 1) / SB_TILE));
    hipLaunchKernelGGL(boundary_fused_kernel, grid, dim3(SB_THREADS), SB_LDS_BYTES, s, p, g, l, h, w, d, n, c, b);
    U2_CHECK_LAUNCH();
    return 0;
  }
  if (!scratch || scratch_bytes < 2 * hw) return -1;
  long long blocks = (hw + SB_THREADS - 1) / SB_THREADS;
  blocks = blocks > 2048 ? 2048 : blocks;
  hipLaunchKernelGGL(boundary_rowmin_kernel, dim3((unsigned)blocks), dim3(SB_THREADS), 0, s, p, g, l, h, w, d, (uint8_t*)scratch);
  U2_CHECK_LAUNCH();
  hipLaunchKernelGGL(boundary_colmin_count_kernel, dim3((unsigned)blocks), dim3(SB_THREADS), 0, s, p, g, l, (const uint8_t*)scratch, h,
                     w, d, n, c, b);
  U2_CHECK_LAUNCH();
  return 0;
}
