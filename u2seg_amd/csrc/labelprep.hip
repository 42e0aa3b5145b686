// Pseudo-panoptic label merge on the device (gfx950): the class-aware pseudo instances painted over the unsupervised semantic
// map, the stuff classes that claim what is left, and the label images of data/pseudo_panoptic.py's merge_image /
// separate_semantic_from_panoptic.  Contracts: include/u2seg_hip.h, design: DESIGN.md section 18.
//
// Three launches per batch: paint (per pixel the last painted instance, per class the pixel counts), decide (segment ids,
// walking the images in order because the ids run on), emit (id image, label map, id map).  Everything is integer work with
// integer atomics and plain stores of values that do not depend on who stores them: no result depends on any order.
// The instances come as the column-major bit planes of maskeval.hip (u2_mask_planes_from_counts).
#include "common.h"
#include "u2seg_hip.h"

typedef unsigned long long u64;

constexpr int LP_MAXIMG = 64;
constexpr int LP_CLASSES = U2_LABEL_CLASSES;  // 27 semantic labels, class c = label + 1
constexpr int LP_HIST = U2_LABEL_HIST;        // ints per image: [c] pixels of class c, [32 + c] of them under an instance
constexpr int LP_DEC = U2_LABEL_DEC;          // words per image: [l] id of label l (0: not claimed), [27] next id, [28] base
constexpr int LP_COLS = 256;                  // columns of a work-group's band
struct LabelBatch { U2LabelImage im[LP_MAXIMG]; };

// ---- paint and count ------------------------------------------------------------------------------------------------------
// One work-group per (strip of 256 columns, band of 64 rows, image).  Phase 1, thread = column: the band's word of plane
// n - 1, n - 2, ... serves the column's 64 pixels at once; the bits that are still undecided take that rank, and the walk ends
// when none is left.  Phase 2, thread = column again but row by row, so that the label bytes are read and the ranks written
// along the rows: the class counts are summed per wave with ballots (a blocky label map gives one or two classes per row of
// 64 pixels), one LDS atomic per wave and class, and the work-group's histogram goes to memory in at most 56 atomics.
// grid (strips of the widest image, bands of the tallest image, images)
__global__ __launch_bounds__(256) void label_paint_kernel(const LabelBatch batch, const u64* __restrict__ planes,
                                                          const uint8_t* __restrict__ sem, int* __restrict__ rank,
                                                          int* __restrict__ present, int* __restrict__ hist, int img0) {
  const U2LabelImage im = batch.im[blockIdx.z];
  const int H = im.H, W = im.W, x0 = (int)blockIdx.x * LP_COLS, j = (int)blockIdx.y, y0 = j * 64;
  if (x0 >= W || y0 >= H) return;
  const int wpc = (H + 63) >> 6, rows = min(64, H - y0), tx = (int)threadIdx.x, x = x0 + tx;
  __shared__ __attribute__((aligned(16))) uint16_t win[64 * LP_COLS];  // rank + 1 of the band's pixels (n <= 65535), row-major
  __shared__ int lhist[LP_HIST];
  for (int t = tx; t < 64 * LP_COLS / 8; t += 256) reinterpret_cast<uint4*>(win)[t] = make_uint4(0u, 0u, 0u, 0u);
  if (tx < LP_HIST) lhist[tx] = 0;
  __syncthreads();
  if (x < W) {
    u64 open = rows == 64 ? ~0ull : (1ull << rows) - 1ull;
    const u64* col = planes + im.plane_offset + (long long)x * wpc + j;
    const long long nw = (long long)W * wpc;
    for (int k = im.n - 1; k >= 0 && open; --k) {
      u64 w = col[(long long)k * nw] & open;
      if (!w) continue;
      present[im.first + k] = 1;
      open &= ~w;
      while (w) {
        const int b = (int)__builtin_ctzll(w);
        w &= w - 1ull;
        win[b * LP_COLS + tx] = (uint16_t)(k + 1);
      }
    }
  }
  __syncthreads();
  const int lane = tx & 63;
  for (int r = 0; r < rows; ++r) {
    int c = 0, rk = 0;
    if (x < W) {
      const long long p = im.pix_offset + (long long)(y0 + r) * W + x;
      const int s = sem[p];
      c = s < LP_CLASSES ? s + 1 : 0;
      rk = win[r * LP_COLS + tx];
      rank[p] = rk;
    }
    u64 todo = __ballot(c != 0);
    while (todo) {  // wave-uniform: every lane of the wave takes part in the ballots
      const int lead = (int)__builtin_ctzll(todo);
      const int c0 = __shfl(c, lead, 64);
      const u64 same = __ballot(c == c0), cov = __ballot(c == c0 && rk != 0);
      if (lane == lead) {
        atomicAdd(&lhist[c0], __popcll(same));
        if (cov) atomicAdd(&lhist[32 + c0], __popcll(cov));
      }
      todo &= ~same;
    }
  }
  __syncthreads();
  if (tx < LP_HIST && lhist[tx]) atomicAdd(hist + (long long)(img0 + (int)blockIdx.z) * LP_HIST + tx, lhist[tx]);
}

// ---- decide and number ----------------------------------------------------------------------------------------------------
// One wave for the whole batch.  Image i's instances are base_i + rank; lane c = 1..27 then decides its class and the claimed
// classes take the following ids in class order (a ballot's prefix count).  total - covered > 0 and not
// 10 covered > 7 total is the host's `covered / total > 0.7` in float64, exactly.
__global__ __launch_bounds__(64) void label_decide_kernel(const int* __restrict__ hist, const int* __restrict__ counts,
                                                          unsigned* __restrict__ dec, unsigned first_id, int num_images) {
  const int c = (int)threadIdx.x;
  unsigned next = first_id;
  for (int i = 0; i < num_images; ++i) {
    const int* h = hist + (long long)i * LP_HIST;
    bool claim = false;
    if (c >= 1 && c <= LP_CLASSES) {
      const long long total = h[c], covered = h[32 + c];
      claim = total - covered > 0 && !(10 * covered > 7 * total);
    }
    const u64 claims = __ballot(claim);
    const unsigned base = next, stuff0 = base + (unsigned)counts[i];
    unsigned* d = dec + (long long)i * LP_DEC;
    if (c >= 1 && c <= LP_CLASSES) d[c - 1] = claim ? stuff0 + (unsigned)__popcll(claims & ((1ull << c) - 1ull)) : 0u;
    next = stuff0 + (unsigned)__popcll(claims);
    if (c == 0) { d[LP_CLASSES] = next; d[LP_CLASSES + 1] = base; }
  }
}

// ---- emit -----------------------------------------------------------------------------------------------------------------
// Thread = four consecutive pixels of the image's flat pixel list (pix_offset is a multiple of 4, so the 16 bytes of ranks,
// the 4 label bytes and the 12 bytes of the id image are aligned vector accesses); the last, partial group goes pixel by pixel.
// grid (blocks of the largest image, images)
__device__ __forceinline__ void label_pixel(int rk, int s, unsigned base, const unsigned* stuff, unsigned& id, unsigned& lab) {
  const unsigned st = s < LP_CLASSES ? stuff[s] : 0u;
  id = rk ? base + (unsigned)(rk - 1) : st;
  lab = rk ? 0u : (st ? (unsigned)(s + 1) : 255u);
}

__global__ __launch_bounds__(256) void label_emit_kernel(const LabelBatch batch, const int* __restrict__ rank,
                                                         const uint8_t* __restrict__ sem, const unsigned* __restrict__ dec,
                                                         uint8_t* __restrict__ rgb, uint8_t* __restrict__ label,
                                                         unsigned* __restrict__ ids, int img0) {
  const U2LabelImage im = batch.im[blockIdx.y];
  const long long npix = (long long)im.H * im.W, g = (long long)blockIdx.x * 256 + threadIdx.x;
  if ((long long)blockIdx.x * 1024 >= npix) return;
  __shared__ unsigned stuff[LP_DEC];
  if (threadIdx.x < LP_DEC) stuff[threadIdx.x] = dec[(long long)(img0 + (int)blockIdx.y) * LP_DEC + threadIdx.x];
  __syncthreads();
  const unsigned base = stuff[LP_CLASSES + 1];
  const long long p = im.pix_offset + 4 * g;
  if (4 * g + 4 <= npix) {
    const int4 rk = *reinterpret_cast<const int4*>(rank + p);
    const unsigned s4 = *reinterpret_cast<const unsigned*>(sem + p);
    unsigned id[4], lab[4];
    label_pixel(rk.x, (int)(s4 & 255u), base, stuff, id[0], lab[0]);
    label_pixel(rk.y, (int)((s4 >> 8) & 255u), base, stuff, id[1], lab[1]);
    label_pixel(rk.z, (int)((s4 >> 16) & 255u), base, stuff, id[2], lab[2]);
    label_pixel(rk.w, (int)(s4 >> 24), base, stuff, id[3], lab[3]);
    if (rgb) {  // bytes id & 255, id >> 8 & 255, id >> 16 & 255 of four pixels = three little-endian words
      unsigned* o = reinterpret_cast<unsigned*>(rgb + 3 * p);
      const unsigned a = id[0] & 0xffffffu, b = id[1] & 0xffffffu, c = id[2] & 0xffffffu, d = id[3] & 0xffffffu;
      o[0] = a | (b << 24);
      o[1] = (b >> 8) | (c << 16);
      o[2] = (c >> 16) | (d << 8);
    }
    if (label) *reinterpret_cast<unsigned*>(label + p) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
    if (ids) *reinterpret_cast<uint4*>(ids + p) = make_uint4(id[0], id[1], id[2], id[3]);
  } else {
    for (long long q = 4 * g; q < npix; ++q) {
      unsigned id, lab;
      const long long at = im.pix_offset + q;
      label_pixel(rank[at], sem[at], base, stuff, id, lab);
      if (rgb) {
        rgb[3 * at + 0] = (uint8_t)(id & 255u);
        rgb[3 * at + 1] = (uint8_t)((id >> 8) & 255u);
        rgb[3 * at + 2] = (uint8_t)((id >> 16) & 255u);
      }
      if (label) label[at] = (uint8_t)lab;
      if (ids) ids[at] = id;
    }
  }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
static bool label_images_ok(const U2LabelImage* images, int num_images) {
  if (!images) return false;
  for (int i = 0; i < num_images; ++i) {
    const U2LabelImage& m = images[i];
    if (m.first < 0 || m.n < 0 || m.H < 0 || m.W < 0 || m.plane_offset < 0 || m.pix_offset < 0 || (m.pix_offset & 3)) return false;
    if ((long long)m.H * m.W >= (1LL << 31) || m.n > 65535) return false;
  }
  return true;
}

extern "C" int u2_label_paint(const void* planes, const void* sem, int* rank, int* present, int* hist,
                              const U2LabelImage* images, int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!label_images_ok(images, num_images) || !sem || !rank || !present || !hist || ((uintptr_t)planes & 7) ||
      ((uintptr_t)rank & 15))
    return -1;
  const hipStream_t s = (hipStream_t)stream;
  long long instances = 0;
  for (int i = 0; i < num_images; ++i) {
    if (images[i].n > 0 && !planes) return -1;
    if ((long long)images[i].first + images[i].n > instances) instances = (long long)images[i].first + images[i].n;
  }
  u2_zero_words(hist, (size_t)num_images * LP_HIST, s);
  u2_zero_words(present, (size_t)instances, s);
  U2_CHECK_LAUNCH();
  for (int i0 = 0; i0 < num_images; i0 += LP_MAXIMG) {
    LabelBatch b;
    const int nb = num_images - i0 < LP_MAXIMG ? num_images - i0 : LP_MAXIMG;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i] = images[i0 + i];
      if (b.im[i].H == 0 || b.im[i].W == 0) continue;
      if (b.im[i].W > max_w) max_w = b.im[i].W;
      if (b.im[i].H > max_h) max_h = b.im[i].H;
    }
    if (max_w == 0) continue;
    const int gy = (max_h + 63) / 64;
    if (gy > 65535) return -1;
    hipLaunchKernelGGL(label_paint_kernel, dim3((max_w + LP_COLS - 1) / LP_COLS, gy, nb), dim3(256), 0, s, b, (const u64*)planes,
                       (const uint8_t*)sem, rank, present, hist, i0);
    U2_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int u2_label_decide(const int* hist, const int* counts, void* decisions, long long first_id, int num_images,
                               void* stream) {
  if (num_images <= 0) return 0;
  if (!hist || !counts || !decisions || first_id < 0 || first_id > 0xffffffffLL) return -1;
  hipLaunchKernelGGL(label_decide_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hist, counts, (unsigned*)decisions,
                     (unsigned)first_id, num_images);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_label_emit(const int* rank, const void* sem, const void* decisions, void* rgb, void* label, void* ids,
                             const U2LabelImage* images, int num_images, void* stream) {
  if (num_images <= 0) return 0;
  if (!label_images_ok(images, num_images) || !rank || !sem || !decisions || ((uintptr_t)rank & 15) || ((uintptr_t)sem & 3) ||
      ((uintptr_t)rgb & 3) || ((uintptr_t)label & 3) || ((uintptr_t)ids & 15))
    return -1;
  for (int i0 = 0; i0 < num_images; i0 += LP_MAXIMG) {
    LabelBatch b;
    const int nb = num_images - i0 < LP_MAXIMG ? num_images - i0 : LP_MAXIMG;
    long long max_pix = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i] = images[i0 + i];
      const long long np = (long long)b.im[i].H * b.im[i].W;
      if (np > max_pix) max_pix = np;
    }
    if (max_pix == 0) continue;
    hipLaunchKernelGGL(label_emit_kernel, dim3((unsigned)((max_pix + 1023) / 1024), nb), dim3(256), 0, (hipStream_t)stream, b,
                       rank, (const uint8_t*)sem, (const unsigned*)decisions, (uint8_t*)rgb, (uint8_t*)label, (unsigned*)ids, i0);
    U2_CHECK_LAUNCH();
  }
  return 0;
}
