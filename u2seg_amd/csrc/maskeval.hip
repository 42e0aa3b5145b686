// Mask evaluation on the device (gfx950): bit planes of the pasted canvases, COCO run-length strings, ground-truth planes
// from uncompressed counts and pairwise intersections.  Contracts: include/u2seg_hip.h, design: DESIGN.md section 11.
//
// Plane layout (column-major like COCO's RLE scan): a mask of H x W is W columns of wpc = ceil(H / 64) 64-bit words, bit b of
// word j of column x = pixel (y = 64 j + b, x); the padding bits of a column's last word are zero.  Everything here is integer
// work: no result depends on the order of a reduction.
#include <limits.h>
#include "common.h"
#include "u2seg_hip.h"

typedef unsigned long long u64;

constexpr int ME_MAXIMG = 64;
struct MaskBatch { U2MaskImage im[ME_MAXIMG]; };
struct PairBatch { U2PairImage im[ME_MAXIMG]; };

// ---- canvases -> planes ------------------------------------------------------------------------------------------------
// One work-group per (strip of 256 columns, mask); it walks the mask's 64-row bands.  A band's rows are fetched as aligned
// 16-byte pieces (a row starts at any byte: W is arbitrary) and stored in LDS at the same alignment, so row r sits shifted by
// (address of its first byte) & 15; then thread x reads its column down the band and forms the word.
constexpr int PK_COLS = 256, PK_CHUNKS = PK_COLS / 16 + 2, PK_PITCH = PK_CHUNKS * 16;
// grid (strips of the widest image, masks of the largest image, images)
__global__ __launch_bounds__(256) void mask_pack_kernel(const MaskBatch batch, const uint8_t* __restrict__ in, u64* __restrict__ planes) {
  const U2MaskImage im = batch.im[blockIdx.z];
  const int k = blockIdx.y, x0 = (int)blockIdx.x * PK_COLS;
  if (k >= im.n || x0 >= im.W) return;
  const int H = im.H, W = im.W, wpc = (H + 63) >> 6;
  const int cw = min(PK_COLS, W - x0);
  const long long total = (long long)im.n * H * W;  // bytes of this image's canvases
  const uint8_t* src = in + im.in_offset;           // 16-byte aligned
  __shared__ __attribute__((aligned(16))) uint8_t tile[64 * PK_PITCH];
  const int tx = (int)threadIdx.x;
  u64* dst = planes + im.plane_offset + ((long long)k * W + x0 + tx) * wpc;
  for (int j = 0; j < wpc; ++j) {
    const int y0 = j * 64, rows = min(64, H - y0);
    const long long band = ((long long)k * H + y0) * W + x0;  // byte of pixel (y0, x0)
    for (int t = tx; t < rows * PK_CHUNKS; t += 256) {
      const int r = t / PK_CHUNKS, c = t % PK_CHUNKS;
      const long long g0 = band + (long long)r * W;
      const long long a = (g0 & ~15LL) + 16LL * c;
      if (a >= g0 + cw) continue;
      uint4 v;
      if (a + 16 <= total) {
        v = *reinterpret_cast<const uint4*>(src + a);
      } else {  // the last piece of the image's canvases: byte by byte, nothing past the end is read
        unsigned w4[4] = {0u, 0u, 0u, 0u};
        for (int e = 0; e < 16; ++e)
          if (a + e < total) w4[e >> 2] |= (unsigned)src[a + e] << (8 * (e & 3));
        v = make_uint4(w4[0], w4[1], w4[2], w4[3]);
      }
      *reinterpret_cast<uint4*>(tile + r * PK_PITCH + 16 * c) = v;
    }
    __syncthreads();
    if (tx < cw) {
      u64 word = 0;
      for (int r = 0; r < rows; ++r) {
        const int s = (int)((band + (long long)r * W) & 15);
        word |= (u64)(tile[r * PK_PITCH + s + tx] != 0) << r;
      }
      dst[j] = word;
    }
    __syncthreads();
  }
}

// area and tight box of every mask from its plane; grid (masks of the largest image, images)
__global__ __launch_bounds__(256) void mask_stats_kernel(const MaskBatch batch, const u64* __restrict__ planes, int* __restrict__ area,
                                                         int* __restrict__ box) {
  const U2MaskImage im = batch.im[blockIdx.y];
  const int k = blockIdx.x;
  if (k >= im.n) return;
  const int H = im.H, W = im.W, wpc = (H + 63) >> 6;
  const long long nw = (long long)W * wpc;
  const u64* p = planes + im.plane_offset + (long long)k * nw;
  int a = 0, xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  for (long long i = threadIdx.x; i < nw; i += 256) {
    const u64 w = p[i];
    if (!w) continue;
    const int x = (int)(i / wpc), j = (int)(i % wpc);
    a += __popcll(w);
    xmin = min(xmin, x);
    xmax = max(xmax, x);
    ymin = min(ymin, 64 * j + (int)__builtin_ctzll(w));
    ymax = max(ymax, 64 * j + 63 - (int)__builtin_clzll(w));
  }
  __shared__ int red[5][4];
  a = wave_isum(a); xmin = wave_imin(xmin); ymin = wave_imin(ymin); xmax = wave_imax(xmax); ymax = wave_imax(ymax);
  const int wv = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wv] = a; red[1][wv] = xmin; red[2][wv] = ymin; red[3][wv] = xmax; red[4][wv] = ymax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    xmin = min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3]));
    ymin = min(min(red[2][0], red[2][1]), min(red[2][2], red[2][3]));
    xmax = max(max(red[3][0], red[3][1]), max(red[3][2], red[3][3]));
    ymax = max(max(red[4][0], red[4][1]), max(red[4][2], red[4][3]));
    const long long m = (long long)im.first + k;
    area[m] = a;
    const bool any = a > 0;
    box[m * 4 + 0] = any ? xmin : 0;
    box[m * 4 + 1] = any ? ymin : 0;
    box[m * 4 + 2] = any ? xmax - xmin + 1 : 0;
    box[m * 4 + 3] = any ? ymax - ymin + 1 : 0;
  }
}

// ---- planes -> run-length strings ---------------------------------------------------------------------------------------
// A run starts where a pixel differs from the pixel before it in the column-major scan (the pixel before (0, 0) counts as 0):
// the transitions of column x are plane ^ (plane shifted up by one pixel), the carry coming from the word below or from pixel
// H - 1 of column x - 1.  f(p) is called with the scan positions p = x H + y of column x's transitions in ascending order.
template <class F>
__device__ __forceinline__ void for_each_transition(const u64* __restrict__ mask, int x, int H, int wpc, F f) {
  const u64* col = mask + (long long)x * wpc;
  u64 carry = x > 0 ? (col[-1] >> ((H - 1) & 63)) & 1ull : 0ull;
  for (int j = 0; j < wpc; ++j) {
    const u64 v = col[j];
    u64 t = v ^ ((v << 1) | carry);
    carry = v >> 63;
    if (j == wpc - 1 && (H & 63)) t &= (1ull << (H & 63)) - 1ull;
    while (t) {
      const int b = (int)__builtin_ctzll(t);
      t &= t - 1ull;
      f(x * H + 64 * j + b);
    }
  }
}

// per column: the number of transitions and the positions of its last three (newest first); grid as mask_pack_kernel
__global__ __launch_bounds__(256) void rle_count_kernel(const MaskBatch batch, const u64* __restrict__ planes, int* __restrict__ colcnt,
                                                        int* __restrict__ last3) {
  const U2MaskImage im = batch.im[blockIdx.z];
  const int k = blockIdx.y, x = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= im.n || x >= im.W) return;
  const int H = im.H, W = im.W, wpc = (H + 63) >> 6;
  const u64* mask = planes + im.plane_offset + (long long)k * W * wpc;
  int n = 0, l0 = 0, l1 = 0, l2 = 0;
  for_each_transition(mask, x, H, wpc, [&](int p) { l2 = l1; l1 = l0; l0 = p; ++n; });
  const long long col = im.col_offset + (long long)k * W + x;
  colcnt[col] = n;
  last3[col * 3 + 0] = l0;
  last3[col * 3 + 1] = l1;
  last3[col * 3 + 2] = l2;
}

// One count of the string: 5-bit groups low first, 0x20 = more follows, bit 0x10 of the last group is the sign, + 48.
template <bool EMIT>
__device__ __forceinline__ int rle_put(long long v, uint8_t* out, long long at, long long cap) {
  int n = 0;
  bool more;
  do {
    const int g = (int)(v & 31);
    v >>= 5;
    more = (g & 16) ? (v != -1) : (v != 0);
    if (EMIT && at + n < cap) out[at + n] = (uint8_t)((g | (more ? 32 : 0)) + 48);
    ++n;
  } while (more);
  return n;
}

// EMIT = false: collen[col] = characters that column col's transitions contribute (the mask's last column also owns the final
// count).  EMIT = true: writes them at strcum[col - 1] of the arena.  The three transitions before the column's first one are
// found through lastne (last column <= c of the flat column list that has a transition, -1: none): at most three hops.
template <bool EMIT>
__global__ __launch_bounds__(256) void rle_string_kernel(const MaskBatch batch, const u64* __restrict__ planes,
                                                         const int* __restrict__ colcnt, const int* __restrict__ last3,
                                                         const long long* __restrict__ cntcum, const long long* __restrict__ lastne,
                                                         int* __restrict__ collen, const long long* __restrict__ strcum,
                                                         uint8_t* __restrict__ arena, long long arena_bytes) {
  const U2MaskImage im = batch.im[blockIdx.z];
  const int k = blockIdx.y, x = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= im.n || x >= im.W) return;
  const int H = im.H, W = im.W, wpc = (H + 63) >> 6;
  const u64* mask = planes + im.plane_offset + (long long)k * W * wpc;
  const long long cb = im.col_offset + (long long)k * W, col = cb + x;
  const int mine = colcnt[col];
  if (mine == 0 && x != W - 1) {
    if (!EMIT) collen[col] = 0;
    return;
  }
  int q[3] = {0, 0, 0}, got = 0;
  long long c = x > 0 ? lastne[col - 1] : -1;
  while (got < 3 && c >= cb) {
    const int n = min(colcnt[c], 3);
    for (int e = 0; e < n && got < 3; ++e) q[got++] = last3[c * 3 + e];
    c = c > cb ? lastne[c - 1] : -1;
  }
  long long i = (cntcum[col] - mine) - (cntcum[cb] - colcnt[cb]);  // index of this column's first count in the mask's list
  long long plast = q[0], c1 = (long long)q[0] - q[1], c2 = (long long)q[1] - q[2];
  long long at = EMIT ? (col > 0 ? strcum[col - 1] : 0) : 0;
  int len = 0;
  auto put = [&](long long cnt) {
    const int n = rle_put<EMIT>(cnt - (i > 2 ? c2 : 0), arena, at, arena_bytes);
    at += n;
    len += n;
    c2 = c1;
    c1 = cnt;
    ++i;
  };
  for_each_transition(mask, x, H, wpc, [&](int p) {
    put((long long)p - plast);
    plast = p;
  });
  if (x == W - 1) put((long long)H * W - plast);
  if (!EMIT) collen[col] = len;
}

// ---- uncompressed counts -> planes ----------------------------------------------------------------------------------------
// cum = inclusive prefix sums of the flat counts list, offs [M + 1] = first count of every mask.  One thread per plane word:
// binary search for the run that holds the word's first pixel, then a walk over the runs that touch the word.  Every word is
// written once, padding bits included: no pre-zeroing and no atomics.  grid (word blocks of the largest mask, masks, images)
__global__ __launch_bounds__(256) void planes_from_counts_kernel(const MaskBatch batch, const long long* __restrict__ cum,
                                                                 const long long* __restrict__ offs, u64* __restrict__ planes) {
  const U2MaskImage im = batch.im[blockIdx.z];
  const int k = blockIdx.y;
  if (k >= im.n) return;
  const int H = im.H, W = im.W, wpc = (H + 63) >> 6;
  const long long nw = (long long)W * wpc, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw) return;
  const int x = (int)(i / wpc), j = (int)(i % wpc);
  const long long lo = offs[im.first + k], hi = offs[im.first + k + 1];
  const long long base = lo > 0 ? cum[lo - 1] : 0;
  const long long p0 = (long long)x * H + 64 * j, p1 = p0 + min(64, H - 64 * j);
  long long a = lo, b = hi;  // first run in [lo, hi) that ends after p0
  while (a < b) {
    const long long m = (a + b) >> 1;
    if (cum[m] - base > p0) b = m; else a = m + 1;
  }
  u64 word = 0;
  long long pos = p0;
  for (long long r = a; r < hi && pos < p1; ++r) {
    const long long e = min(cum[r] - base, p1);
    if (((r - lo) & 1) && e > pos) {
      const int n = (int)(e - pos), s = (int)(pos - p0);
      word |= (n >= 64 ? ~0ull : ((1ull << n) - 1ull)) << s;
    }
    pos = max(pos, e);
  }
  planes[im.plane_offset + (long long)k * nw + i] = word;
}

// ---- pairwise intersections -----------------------------------------------------------------------------------------------
// inter[d][g] = popcount(dt[d] & gt[g]); grid (detections of the largest image, blocks of 8 ground truths, images).  With the
// detections' tight boxes only the columns inside the box are read (the rest of a detection's plane is zero).
constexpr int PR_G = 8;
__global__ __launch_bounds__(256) void pair_counts_kernel(const PairBatch batch, const u64* __restrict__ dt, const u64* __restrict__ gt,
                                                          const int* __restrict__ dt_box, int* __restrict__ inter) {
  const U2PairImage im = batch.im[blockIdx.z];
  const int d = blockIdx.x, g0 = (int)blockIdx.y * PR_G;
  if (d >= im.D || g0 >= im.G) return;
  const int wpc = (im.H + 63) >> 6, ng = min(PR_G, im.G - g0);
  const long long nw = (long long)im.W * wpc;
  long long w0 = 0, w1 = nw;
  if (dt_box) {
    const int* b = dt_box + ((long long)im.dt_first + d) * 4;
    const int bx = max(b[0], 0), bw = max(min(b[2], im.W - bx), 0);
    w0 = (long long)bx * wpc;
    w1 = w0 + (long long)bw * wpc;
  }
  const u64* pd = dt + im.dt_offset + (long long)d * nw;
  const u64* pg = gt + im.gt_offset + (long long)g0 * nw;
  int acc[PR_G];
#pragma unroll
  for (int e = 0; e < PR_G; ++e) acc[e] = 0;
  for (long long i = w0 + threadIdx.x; i < w1; i += 256) {
    const u64 v = pd[i];
    if (!v) continue;
#pragma unroll
    for (int e = 0; e < PR_G; ++e)
      if (e < ng) acc[e] += __popcll(v & pg[(long long)e * nw + i]);
  }
  __shared__ int red[4][PR_G];
#pragma unroll
  for (int e = 0; e < PR_G; ++e) {
    const int s = wave_isum(acc[e]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][e] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < ng)
    inter[im.out_offset + (long long)d * im.G + g0 + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static bool mask_images_ok(const U2MaskImage* images, int num_images) {
  if (!images) return false;
  for (int i = 0; i < num_images; ++i) {
    const U2MaskImage& m = images[i];
    if (m.first < 0 || m.n < 0 || m.H < 0 || m.W < 0 || m.in_offset < 0 || m.plane_offset < 0 || m.col_offset < 0) return false;
    if ((long long)m.H * m.W >= (1LL << 31) || m.n > 65535) return false;
  }
  return true;
}

// calls launch(batch, images in it, widest image, most masks, most plane words) for every group of ME_MAXIMG images
template <class L>
static int for_each_mask_batch(const U2MaskImage* images, int num_images, L launch) {
  for (int i0 = 0; i0 < num_images; i0 += ME_MAXIMG) {
    MaskBatch b;
    const int nb = num_images - i0 < ME_MAXIMG ? num_images - i0 : ME_MAXIMG;
    int max_w = 0, max_n = 0;
    long long max_words = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i] = images[i0 + i];
      if (b.im[i].n == 0 || b.im[i].H == 0 || b.im[i].W == 0) { b.im[i].n = 0; continue; }
      if (b.im[i].W > max_w) max_w = b.im[i].W;
      if (b.im[i].n > max_n) max_n = b.im[i].n;
      const long long nw = (long long)b.im[i].W * ((b.im[i].H + 63) >> 6);
      if (nw > max_words) max_words = nw;
    }
    if (max_n == 0) continue;
    launch(b, nb, max_w, max_n, max_words);
    U2_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int u2_mask_pack_planes(const void* canvases, void* planes, int* area, int* box, const U2MaskImage* images,
                                   int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!mask_images_ok(images, num_images) || ((uintptr_t)canvases & 15) || ((uintptr_t)planes & 7)) return -1;
  for (int i = 0; i < num_images; ++i)
    if (images[i].in_offset & 15) return -1;
  const hipStream_t s = (hipStream_t)stream;
  return for_each_mask_batch(images, num_images, [&](const MaskBatch& b, int nb, int max_w, int max_n, long long) {
    hipLaunchKernelGGL(mask_pack_kernel, dim3((max_w + PK_COLS - 1) / PK_COLS, max_n, nb), dim3(256), 0, s, b,
                       (const uint8_t*)canvases, (u64*)planes);
    if (area && box)
      hipLaunchKernelGGL(mask_stats_kernel, dim3(max_n, nb), dim3(256), 0, s, b, (const u64*)planes, area, box);
  });
}

extern "C" int u2_mask_rle_count(const void* planes, int* colcnt, int* last3, const U2MaskImage* images, int num_images,
                                 void* stream) {
  if (num_images <= 0) return 0;
  if (!mask_images_ok(images, num_images) || ((uintptr_t)planes & 7)) return -1;
  const hipStream_t s = (hipStream_t)stream;
  return for_each_mask_batch(images, num_images, [&](const MaskBatch& b, int nb, int max_w, int max_n, long long) {
    hipLaunchKernelGGL(rle_count_kernel, dim3((max_w + 255) / 256, max_n, nb), dim3(256), 0, s, b, (const u64*)planes, colcnt,
                       last3);
  });
}

extern "C" int u2_mask_rle_lengths(const void* planes, const int* colcnt, const int* last3, const long long* cntcum,
                                   const long long* lastne, int* collen, const U2MaskImage* images, int num_images,
                                   void* stream) {
  if (num_images <= 0) return 0;
  if (!mask_images_ok(images, num_images) || ((uintptr_t)planes & 7)) return -1;
  const hipStream_t s = (hipStream_t)stream;
  return for_each_mask_batch(images, num_images, [&](const MaskBatch& b, int nb, int max_w, int max_n, long long) {
    hipLaunchKernelGGL(rle_string_kernel<false>, dim3((max_w + 255) / 256, max_n, nb), dim3(256), 0, s, b, (const u64*)planes,
                       colcnt, last3, cntcum, lastne, collen, (const long long*)nullptr, (uint8_t*)nullptr, 0LL);
  });
}

extern "C" int u2_mask_rle_emit(const void* planes, const int* colcnt, const int* last3, const long long* cntcum,
                                const long long* lastne, const long long* strcum, void* arena, long long arena_bytes,
                                const U2MaskImage* images, int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!mask_images_ok(images, num_images) || ((uintptr_t)planes & 7) || arena_bytes < 0) return -1;
  const hipStream_t s = (hipStream_t)stream;
  return for_each_mask_batch(images, num_images, [&](const MaskBatch& b, int nb, int max_w, int max_n, long long) {
    hipLaunchKernelGGL(rle_string_kernel<true>, dim3((max_w + 255) / 256, max_n, nb), dim3(256), 0, s, b, (const u64*)planes,
                       colcnt, last3, cntcum, lastne, (int*)nullptr, strcum, (uint8_t*)arena, arena_bytes);
  });
}

extern "C" int u2_mask_planes_from_counts(const long long* cum, const long long* offs, void* planes, const U2MaskImage* images,
                                          int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!mask_images_ok(images, num_images) || ((uintptr_t)planes & 7)) return -1;
  const hipStream_t s = (hipStream_t)stream;
  return for_each_mask_batch(images, num_images, [&](const MaskBatch& b, int nb, int, int max_n, long long max_words) {
    hipLaunchKernelGGL(planes_from_counts_kernel, dim3((unsigned)((max_words + 255) / 256), max_n, nb), dim3(256), 0, s, b, cum,
                       offs, (u64*)planes);
  });
}

extern "C" int u2_mask_pair_counts(const void* dt_planes, const void* gt_planes, const int* dt_boxes, int* inter,
                                   const U2PairImage* images, int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!images || ((uintptr_t)dt_planes & 7) || ((uintptr_t)gt_planes & 7)) return -1;
  for (int i = 0; i < num_images; ++i) {
    const U2PairImage& m = images[i];
    if (m.D < 0 || m.G < 0 || m.H < 0 || m.W < 0 || m.dt_first < 0 || m.dt_offset < 0 || m.gt_offset < 0 || m.out_offset < 0)
      return -1;
  }
  for (int i0 = 0; i0 < num_images; i0 += ME_MAXIMG) {
    PairBatch b;
    const int nb = num_images - i0 < ME_MAXIMG ? num_images - i0 : ME_MAXIMG;
    int max_d = 0, max_g = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i] = images[i0 + i];
      if (b.im[i].D == 0 || b.im[i].G == 0) continue;
      if (b.im[i].D > max_d) max_d = b.im[i].D;
      if (b.im[i].G > max_g) max_g = b.im[i].G;
    }
    if (max_d == 0) continue;
    const int gy = (max_g + PR_G - 1) / PR_G;
    if (gy > 65535) return -1;
    hipLaunchKernelGGL(pair_counts_kernel, dim3(max_d, gy, nb), dim3(256), 0, (hipStream_t)stream, b, (const u64*)dt_planes,
                       (const u64*)gt_planes, dt_boxes, inter);
    U2_CHECK_LAUNCH();
  }
  return 0;
}
