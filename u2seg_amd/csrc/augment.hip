// Training augmentation on the device (gfx950): PIL's uint8 bilinear resize, its nearest resize and the RLE decode of the
// instance masks, from tables built on the host.  Contract: include/u2seg_hip.h, design: DESIGN.md section 17.
//
// The kernels are byte movers.  The outputs are planes of W-byte rows with W arbitrary, so a thread does not own a piece of a
// row: it owns one aligned dword of the image's flat output (4 consecutive bytes that may wrap into the next row or plane;
// the position is divided out once and stepped) and sends one dword store, 256 contiguous bytes per wave-instruction.  The
// mask kernel cannot do that without a search per byte: there a thread owns a column, searches the run of its first pixel and
// walks, and a wave-instruction stores 64 contiguous bytes of a row.
// Everything is integer work: no result depends on the order of an addition.
// With INPUT.CROP the mask kernel reads its code through a window and also reduces the tight box of what it writes (integer
// wave min / max, one atomic per coordinate per wave); a short second kernel on the same stream puts the empty masks' boxes right.
#include <algorithm>
#include <climits>

#include "common.h"
#include "u2seg_hip.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_MAXIMG = 16;          // descriptors per launch (kernel argument)
constexpr int AG_MAXBLOCKS = 2048;     // work-groups per image along x: the rest is a grid stride
constexpr int AG_ROWS = 32;            // rows a thread of the mask kernel walks
constexpr int AG_SHIFT = 22, AG_HALF = 1 << 21;

struct AugImage {
  U2AugImage d;
  long long scratch_offset;
};
struct AugBatch { AugImage im[AG_MAXIMG]; };

__device__ __forceinline__ unsigned clip8(int v) {
  v >>= AG_SHIFT;
  return (unsigned)min(max(v, 0), 255);
}

// position (c, y, x) of byte i of [3][rows][W], stepped byte by byte
struct PlanePos {
  int c, y, x;
  __device__ __forceinline__ PlanePos(long long i, int rows, int W) {
    const long long plane = (long long)rows * W;
    c = (int)(i / plane);
    const int rem = (int)(i - c * plane);
    y = rem / W;
    x = rem - y * W;
  }
  __device__ __forceinline__ void step(int rows, int W) {
    if (++x == W) {
      x = 0;
      if (++y == rows) { y = 0; ++c; }
    }
  }
};

// Stores up to 4 bytes at byte i of dst (dst + i 4-byte aligned): one dword when all four exist.
__device__ __forceinline__ void store4(uint8_t* dst, long long i, long long total, unsigned v) {
  if (i + 4 <= total) {
    *reinterpret_cast<unsigned*>(dst + i) = v;
  } else {
    for (int b = 0; i + b < total; ++b) dst[i + b] = (uint8_t)(v >> (8 * b));
  }
}

// Horizontal pass.  Destination rows d = 0 .. rows - 1 of [3][rows][W]: with a vertical pass to come, the scratch rows
// (source row row0 + d); with none (y_identity), the output itself (source row by_first[d]).
// grid (blocks, images)
__global__ __launch_bounds__(AG_THREADS) void aug_hpass_kernel(const AugBatch batch, const uint8_t* __restrict__ block,
                                                                uint8_t* __restrict__ img_out, uint8_t* __restrict__ scratch) {
  const AugImage& a = batch.im[blockIdx.y];
  const U2AugImage& im = a.d;
  if (im.x_identity) return;
  const int W = im.W, w = im.w, kx = im.kx;
  const int rows = im.y_identity ? im.H : im.nrows;
  const long long total = 3LL * rows * W;
  const int* tab = reinterpret_cast<const int*>(block);
  const int *bounds = tab + im.bx_bounds, *coef = tab + im.bx_coef, *ybounds = tab + im.by_bounds;
  const uint8_t* src = block + im.src_offset;
  uint8_t* dst = im.y_identity ? img_out + im.img_out_offset : scratch + a.scratch_offset;
  for (long long i = 4 * ((long long)blockIdx.x * AG_THREADS + threadIdx.x); i < total; i += 4LL * gridDim.x * AG_THREADS) {
    PlanePos p(i, rows, W);
    unsigned v = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (i + b < total) {
        const int r = im.y_identity ? ybounds[2 * p.y] : im.row0 + p.y;
        const int first = bounds[2 * p.x], n = bounds[2 * p.x + 1];
        const uint8_t* s = src + ((long long)r * w + first) * 3 + p.c;
        const int* k = coef + (long long)p.x * kx;
        int acc = AG_HALF;
        for (int t = 0; t < n; ++t) acc += (int)s[3 * t] * k[t];
        v |= clip8(acc) << (8 * b);
        p.step(rows, W);
      }
    }
    store4(dst, i, total, v);
  }
}

// Vertical pass into the CHW output; reads the scratch planes, or the source itself when there was no horizontal pass
// (x_identity: column bx_first[x]).  With both axes identities this is the (possibly reordered) HWC -> CHW copy: one tap of 2^22.
__global__ __launch_bounds__(AG_THREADS) void aug_vpass_kernel(const AugBatch batch, const uint8_t* __restrict__ block,
                                                                uint8_t* __restrict__ img_out, const uint8_t* __restrict__ scratch) {
  const AugImage& a = batch.im[blockIdx.y];
  const U2AugImage& im = a.d;
  if (im.y_identity && !im.x_identity) return;
  const int W = im.W, H = im.H, w = im.w, ky = im.ky;
  const long long total = 3LL * H * W;
  const int* tab = reinterpret_cast<const int*>(block);
  const int *bounds = tab + im.by_bounds, *coef = tab + im.by_coef, *xbounds = tab + im.bx_bounds;
  const uint8_t* src = block + im.src_offset;
  const uint8_t* tmp = scratch + a.scratch_offset;
  uint8_t* dst = img_out + im.img_out_offset;
  const long long plane = (long long)im.nrows * W;
  for (long long i = 4 * ((long long)blockIdx.x * AG_THREADS + threadIdx.x); i < total; i += 4LL * gridDim.x * AG_THREADS) {
    PlanePos p(i, H, W);
    unsigned v = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (i + b < total) {
        const int first = bounds[2 * p.y], n = bounds[2 * p.y + 1];
        const int* k = coef + (long long)p.y * ky;
        int acc = AG_HALF;
        if (im.x_identity) {
          const uint8_t* s = src + ((long long)first * w + xbounds[2 * p.x]) * 3 + p.c;
          for (int t = 0; t < n; ++t) acc += (int)s[3LL * t * w] * k[t];
        } else {
          const uint8_t* s = tmp + p.c * plane + (long long)(first - im.row0) * W + p.x;
          for (int t = 0; t < n; ++t) acc += (int)s[(long long)t * W] * k[t];
        }
        v |= clip8(acc) << (8 * b);
        p.step(H, W);
      }
    }
    store4(dst, i, total, v);
  }
}

// one int64 per lane: 512 contiguous bytes per wave-instruction
__global__ __launch_bounds__(AG_THREADS) void aug_nearest_kernel(const AugBatch batch, const uint8_t* __restrict__ block,
                                                                  long long* __restrict__ lab_out) {
  const U2AugImage& im = batch.im[blockIdx.y].d;
  if (im.lab_offset < 0) return;
  const int W = im.W, w = im.w;
  const long long total = (long long)im.H * W;
  const int* tab = reinterpret_cast<const int*>(block);
  const int *nx = tab + im.nx, *ny = tab + im.ny;
  const uint8_t* src = block + im.lab_offset;
  long long* dst = lab_out + im.lab_out_offset;
  for (long long i = (long long)blockIdx.x * AG_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * AG_THREADS) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    dst[i] = (long long)src[(long long)ny[y] * w + nx[x]];
  }
}

// grid (column blocks x row chunks of the largest image, masks of the image with most, images); a thread owns output column x
// and walks AG_ROWS rows: j = number of run ends <= p is found by bisection for its first pixel and followed in both
// directions afterwards (ny is monotone for a resize and a flip, so the walk is short; any table gives the right answer).
// The code is one of mask_h x mask_w read through the window at (wx0, wy0); the plain decode is the window (0, 0) of an h x w code.
// BOXES: the tight box of the 1 bytes.  A lane's candidate is its column and the first and last set row of its walk; a wave
// that saw a set pixel reduces the four coordinates and sends one atomic min / max each (boxes: (INT_MAX, INT_MAX, 0, 0) before,
// x1 / y1 carry the + 1; aug_boxes_kernel behind it puts the empty masks right).
template <bool BOXES>
__device__ __forceinline__ void rle_masks_walk(const U2AugImage& im, int wx0, int wy0, int mask_h, const uint8_t* __restrict__ block,
                                               uint8_t* __restrict__ mask_out, int* __restrict__ counts, int* __restrict__ boxes,
                                               int col_blocks) {
  const int m = (int)blockIdx.y;
  const int cb = (int)blockIdx.x % col_blocks, rc = (int)blockIdx.x / col_blocks;
  const int x = cb * AG_THREADS + (int)threadIdx.x, y0 = rc * AG_ROWS;
  if (m >= im.num_masks || cb * AG_THREADS >= im.W || y0 >= im.H) return;
  const int H = im.H, W = im.W;
  const int* tab = reinterpret_cast<const int*>(block);
  const int* offs = tab + im.mask_offs;
  const unsigned* ends = reinterpret_cast<const unsigned*>(tab) + im.ends_base + offs[m];
  const int nruns = offs[m + 1] - offs[m];
  const int* ny = tab + im.ny;
  int ones = 0, first = INT_MAX, last = -1;
  if (x < W) {
    const unsigned colbase = (unsigned)(wx0 + tab[im.nx + x]) * (unsigned)mask_h + (unsigned)wy0;
    const int y1 = min(y0 + AG_ROWS, H);
    uint8_t* dst = mask_out + im.mask_out_offset + ((long long)m * H + y0) * W + x;
    unsigned p = colbase + (unsigned)ny[y0];
    int lo = 0, hi = nruns;                                      // first j with ends[j] > p; ends[nruns - 1] == mask_h * mask_w > p
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ends[mid] <= p) lo = mid + 1; else hi = mid;
    }
    int j = lo;
    for (int y = y0; y < y1; ++y) {
      p = colbase + (unsigned)ny[y];
      while (ends[j] <= p) ++j;                                  // stops at nruns - 1 at the latest
      while (j > 0 && ends[j - 1] > p) --j;
      const int v = j & 1;
      *dst = (uint8_t)v;
      dst += W;
      ones += v;
      if (BOXES && v) {
        first = min(first, y);
        last = y;
      }
    }
  }
  const int mine = ones;
  ones = wave_isum(ones);
  if (!ones) return;                                             // the same for every lane of the wave
  if (BOXES) {
    const int bx0 = wave_imin(mine ? x : INT_MAX), bx1 = wave_imax(mine ? x + 1 : 0);
    const int by0 = wave_imin(first), by1 = wave_imax(last + 1);
    if ((threadIdx.x & 63) == 0) {
      int* b = boxes + 4LL * (im.first_mask + m);
      atomicMin(b + 0, bx0);
      atomicMin(b + 1, by0);
      atomicMax(b + 2, bx1);
      atomicMax(b + 3, by1);
    }
  }
  if ((threadIdx.x & 63) == 0) atomicAdd(&counts[im.first_mask + m], ones);
}

__global__ __launch_bounds__(AG_THREADS) void aug_rle_masks_kernel(const AugBatch batch, const uint8_t* __restrict__ block,
                                                                    uint8_t* __restrict__ mask_out, int* __restrict__ counts,
                                                                    int col_blocks) {
  const U2AugImage& im = batch.im[blockIdx.z].d;
  rle_masks_walk<false>(im, 0, 0, im.h, block, mask_out, counts, nullptr, col_blocks);
}

struct AugWindows { U2AugWindow w[AG_MAXIMG]; };

__global__ __launch_bounds__(AG_THREADS) void aug_rle_masks_boxes_kernel(const AugBatch batch, const AugWindows windows,
                                                                          const uint8_t* __restrict__ block,
                                                                          uint8_t* __restrict__ mask_out, int* __restrict__ counts,
                                                                          int* __restrict__ boxes, int col_blocks) {
  const U2AugWindow& win = windows.w[blockIdx.z];
  rle_masks_walk<true>(batch.im[blockIdx.z].d, win.x0, win.y0, win.mask_h, block, mask_out, counts, boxes, col_blocks);
}

// before the walk (finish == 0): every box (INT_MAX, INT_MAX, 0, 0); behind it (finish == 1): a box no wave touched is zeros
__global__ void aug_boxes_kernel(int* __restrict__ boxes, int n, int finish) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int4* b = reinterpret_cast<int4*>(boxes) + i;
  if (!finish) {
    *b = make_int4(INT_MAX, INT_MAX, 0, 0);
  } else if (b->z == 0) {
    *b = make_int4(0, 0, 0, 0);
  }
}

// ---- host side: the contract, checked on the host copy of the tables ----------------------------------------------------
struct Tables {
  const int* t;
  long long n;  // int32 elements
  bool has(long long off, long long count) const { return off >= 0 && count >= 0 && off <= n && count <= n - off; }
};

bool geometry_ok(const U2AugImage& im) {
  if (im.h < 1 || im.w < 1 || im.H < 1 || im.W < 1) return false;
  if ((long long)im.h * im.w >= (1LL << 31) || 3LL * im.H * im.W >= (1LL << 31)) return false;
  if ((im.x_identity && im.w != im.W) || (im.y_identity && im.h != im.H)) return false;
  return im.num_masks >= 0 && im.first_mask >= 0;
}

// -1: the table does not fit the block, -3: an entry out of range, 0: fine
int bilinear_axis_ok(const Tables& tb, long long bounds, long long coef, int out, int in, int k) {
  if (k < 1 || !tb.has(bounds, 2LL * out) || !tb.has(coef, (long long)out * k)) return -1;
  for (int i = 0; i < out; ++i) {
    const int first = tb.t[bounds + 2 * i], n = tb.t[bounds + 2 * i + 1];
    if (first < 0 || n < 1 || n > k || first > in - n) return -3;
  }
  return 0;
}

int nearest_axis_ok(const Tables& tb, long long tab, int out, int in) {
  if (!tb.has(tab, out)) return -1;
  for (int i = 0; i < out; ++i)
    if (tb.t[tab + i] < 0 || tb.t[tab + i] >= in) return -3;
  return 0;
}

int bilinear_image_ok(const Tables& tb, const U2AugImage& im) {
  if (!geometry_ok(im)) return -1;
  int rc = bilinear_axis_ok(tb, im.bx_bounds, im.bx_coef, im.W, im.w, im.kx);
  if (rc) return rc;
  rc = bilinear_axis_ok(tb, im.by_bounds, im.by_coef, im.H, im.h, im.ky);
  if (rc) return rc;
  if (im.row0 < 0 || im.nrows < 1 || im.row0 > im.h - im.nrows) return -1;
  if (3LL * im.nrows * im.W >= (1LL << 31)) return -1;             // the scratch planes are indexed like the output
  for (int y = 0; y < im.H; ++y) {
    const int first = tb.t[im.by_bounds + 2 * y], n = tb.t[im.by_bounds + 2 * y + 1];
    if (first < im.row0 || first + n > im.row0 + im.nrows) return -3;
    if (im.y_identity && n != 1) return -3;
  }
  if (im.x_identity)
    for (int x = 0; x < im.W; ++x)
      if (tb.t[im.bx_bounds + 2 * x + 1] != 1) return -3;
  return 0;
}

long long image_scratch_bytes(const U2AugImage& im) {
  if (im.x_identity || im.y_identity) return 0;
  return (3LL * im.nrows * im.W + 15) & ~15LL;
}

unsigned blocks_for(long long items) {
  const long long b = (items + AG_THREADS - 1) / AG_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > AG_MAXBLOCKS ? AG_MAXBLOCKS : b));
}

bool block_ok(const void* block, long long block_bytes, const void* tables_host) {
  return block && tables_host && block_bytes >= 4 && !((uintptr_t)block & 3) && !((uintptr_t)tables_host & 3);
}

}  // namespace

extern "C" long long u2_aug_resize_bilinear_scratch_bytes(const U2AugImage* images, int num_images) {
  if (num_images < 0 || (num_images > 0 && !images)) return -1;
  long long total = 0;
  for (int i = 0; i < num_images; ++i) {
    if (!geometry_ok(images[i]) || images[i].nrows < 1 || images[i].nrows > images[i].h) return -1;
    if (3LL * images[i].nrows * images[i].W >= (1LL << 31)) return -1;
    total += image_scratch_bytes(images[i]);
  }
  return total;
}

extern "C" int u2_aug_resize_bilinear_u8(const void* block, long long block_bytes, const void* tables_host, void* img_out,
                                         long long img_out_bytes, void* scratch, long long scratch_bytes, const U2AugImage* images,
                                         int num_images, void* stream) {
  if (num_images <= 0) return num_images < 0 ? -1 : 0;
  if (!images || !block_ok(block, block_bytes, tables_host) || !img_out || ((uintptr_t)img_out & 3)) return -1;
  const Tables tb{(const int*)tables_host, block_bytes / 4};
  long long need = 0;
  for (int i = 0; i < num_images; ++i) {
    const U2AugImage& im = images[i];
    const int rc = bilinear_image_ok(tb, im);
    if (rc) return rc;
    const long long src_bytes = 3LL * im.h * im.w, out_bytes = 3LL * im.H * im.W;
    if (im.src_offset < 0 || src_bytes > block_bytes || im.src_offset > block_bytes - src_bytes) return -1;
    if (im.img_out_offset < 0 || (im.img_out_offset & 3) || out_bytes > img_out_bytes || im.img_out_offset > img_out_bytes - out_bytes)
      return -1;
    need += image_scratch_bytes(im);
  }
  if (need > 0 && (!scratch || scratch_bytes < need || ((uintptr_t)scratch & 3))) return -1;
  const hipStream_t s = (hipStream_t)stream;
  long long cursor = 0;
  for (int i0 = 0; i0 < num_images; i0 += AG_MAXIMG) {
    AugBatch b;
    const int nb = num_images - i0 < AG_MAXIMG ? num_images - i0 : AG_MAXIMG;
    long long hmax = 0, vmax = 0;
    for (int i = 0; i < nb; ++i) {
      const U2AugImage& im = images[i0 + i];
      b.im[i].d = im;
      b.im[i].scratch_offset = cursor;
      cursor += image_scratch_bytes(im);
      if (!im.x_identity) hmax = std::max(hmax, 3LL * (im.y_identity ? im.H : im.nrows) * im.W);
      if (!im.y_identity || im.x_identity) vmax = std::max(vmax, 3LL * im.H * im.W);
    }
    if (hmax) {
      hipLaunchKernelGGL(aug_hpass_kernel, dim3(blocks_for((hmax + 3) / 4), nb), dim3(AG_THREADS), 0, s, b, (const uint8_t*)block,
                         (uint8_t*)img_out, (uint8_t*)scratch);
      U2_CHECK_LAUNCH();
    }
    if (vmax) {
      hipLaunchKernelGGL(aug_vpass_kernel, dim3(blocks_for((vmax + 3) / 4), nb), dim3(AG_THREADS), 0, s, b, (const uint8_t*)block,
                         (uint8_t*)img_out, (const uint8_t*)scratch);
      U2_CHECK_LAUNCH();
    }
  }
  return 0;
}

extern "C" int u2_aug_resize_nearest_u8(const void* block, long long block_bytes, const void* tables_host, long long* lab_out,
                                        long long lab_out_elems, const U2AugImage* images, int num_images, void* stream) {
  if (num_images <= 0) return num_images < 0 ? -1 : 0;
  if (!images || !block_ok(block, block_bytes, tables_host) || !lab_out || ((uintptr_t)lab_out & 7)) return -1;
  const Tables tb{(const int*)tables_host, block_bytes / 4};
  for (int i = 0; i < num_images; ++i) {
    const U2AugImage& im = images[i];
    if (!geometry_ok(im)) return -1;
    if (im.lab_offset < 0) continue;
    int rc = nearest_axis_ok(tb, im.nx, im.W, im.w);
    if (rc) return rc;
    rc = nearest_axis_ok(tb, im.ny, im.H, im.h);
    if (rc) return rc;
    const long long src_bytes = (long long)im.h * im.w, out_elems = (long long)im.H * im.W;
    if (src_bytes > block_bytes || im.lab_offset > block_bytes - src_bytes) return -1;
    if (im.lab_out_offset < 0 || out_elems > lab_out_elems || im.lab_out_offset > lab_out_elems - out_elems) return -1;
  }
  const hipStream_t s = (hipStream_t)stream;
  for (int i0 = 0; i0 < num_images; i0 += AG_MAXIMG) {
    AugBatch b;
    const int nb = num_images - i0 < AG_MAXIMG ? num_images - i0 : AG_MAXIMG;
    long long most = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i].d = images[i0 + i];
      b.im[i].scratch_offset = 0;
      if (b.im[i].d.lab_offset >= 0) most = std::max(most, (long long)b.im[i].d.H * b.im[i].d.W);
    }
    if (!most) continue;
    hipLaunchKernelGGL(aug_nearest_kernel, dim3(blocks_for(most), nb), dim3(AG_THREADS), 0, s, b, (const uint8_t*)block, lab_out);
    U2_CHECK_LAUNCH();
  }
  return 0;
}

// The two mask entries: windows == nullptr is the plain decode (no boxes), otherwise the windowed one with boxes.
static int rle_masks_launch(const void* block, long long block_bytes, const void* tables_host, void* mask_out,
                            long long mask_out_bytes, int* counts, int* boxes, int num_counts, const U2AugImage* images,
                            const U2AugWindow* windows, int num_images, void* stream) {
  if (num_images <= 0) return num_images < 0 ? -1 : 0;
  if (!images || !block_ok(block, block_bytes, tables_host) || num_counts < 0) return -1;
  const Tables tb{(const int*)tables_host, block_bytes / 4};
  long long masks = 0;
  for (int i = 0; i < num_images; ++i) {
    const U2AugImage& im = images[i];
    if (!geometry_ok(im)) return -1;
    long long code = (long long)im.h * im.w;
    if (windows) {
      const U2AugWindow& win = windows[i];
      if (win.x0 < 0 || win.y0 < 0 || win.mask_h < 1 || win.mask_w < 1) return -1;
      if ((long long)win.x0 + im.w > win.mask_w || (long long)win.y0 + im.h > win.mask_h) return -1;
      code = (long long)win.mask_h * win.mask_w;
      if (code >= (1LL << 31)) return -1;
    }
    if (im.num_masks == 0) continue;
    if (im.num_masks > 65535 || !mask_out || !counts) return -1;
    if (windows && (!boxes || ((uintptr_t)boxes & 15))) return -1;
    int rc = nearest_axis_ok(tb, im.nx, im.W, im.w);
    if (rc) return rc;
    rc = nearest_axis_ok(tb, im.ny, im.H, im.h);
    if (rc) return rc;
    if ((long long)im.first_mask + im.num_masks > num_counts) return -1;
    const long long out_bytes = (long long)im.num_masks * im.H * im.W;
    if (im.mask_out_offset < 0 || out_bytes > mask_out_bytes || im.mask_out_offset > mask_out_bytes - out_bytes) return -1;
    if (!tb.has(im.mask_offs, (long long)im.num_masks + 1)) return -1;
    const unsigned hw = (unsigned)code;
    for (int m = 0; m < im.num_masks; ++m) {
      const long long o0 = tb.t[im.mask_offs + m], o1 = tb.t[im.mask_offs + m + 1];
      if (im.ends_base < 0 || im.ends_base > tb.n || o0 < 0 || o1 <= o0 || !tb.has(im.ends_base + o0, o1 - o0)) return -2;
      const unsigned* e = (const unsigned*)tb.t + im.ends_base + o0;
      for (long long j = 1; j < o1 - o0; ++j)
        if (e[j] < e[j - 1]) return -2;
      if (e[o1 - o0 - 1] != hw) return -2;
    }
    masks += im.num_masks;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (counts && num_counts > 0) {
    u2_zero_words(counts, (size_t)num_counts, s);
    U2_CHECK_LAUNCH();
  }
  if (!masks) {
    if (windows && boxes && num_counts > 0) {                     // rows nobody owns: cleared like the counts
      u2_zero_words(boxes, 4 * (size_t)num_counts, s);
      U2_CHECK_LAUNCH();
    }
    return 0;
  }
  if (windows) {
    hipLaunchKernelGGL(aug_boxes_kernel, dim3((unsigned)((num_counts + AG_THREADS - 1) / AG_THREADS)), dim3(AG_THREADS), 0, s, boxes,
                       num_counts, 0);
    U2_CHECK_LAUNCH();
  }
  for (int i0 = 0; i0 < num_images; i0 += AG_MAXIMG) {
    AugBatch b;
    AugWindows wb;
    const int nb = num_images - i0 < AG_MAXIMG ? num_images - i0 : AG_MAXIMG;
    int max_w = 0, max_h = 0, max_n = 0;
    for (int i = 0; i < nb; ++i) {
      b.im[i].d = images[i0 + i];
      b.im[i].scratch_offset = 0;
      if (windows) wb.w[i] = windows[i0 + i];
      if (!b.im[i].d.num_masks) continue;
      max_w = std::max(max_w, b.im[i].d.W);
      max_h = std::max(max_h, b.im[i].d.H);
      max_n = std::max(max_n, b.im[i].d.num_masks);
    }
    if (!max_n) continue;
    const int col_blocks = (max_w + AG_THREADS - 1) / AG_THREADS, row_chunks = (max_h + AG_ROWS - 1) / AG_ROWS;
    const dim3 grid((unsigned)(col_blocks * row_chunks), (unsigned)max_n, (unsigned)nb);
    if (windows)
      hipLaunchKernelGGL(aug_rle_masks_boxes_kernel, grid, dim3(AG_THREADS), 0, s, b, wb, (const uint8_t*)block, (uint8_t*)mask_out,
                         counts, boxes, col_blocks);
    else
      hipLaunchKernelGGL(aug_rle_masks_kernel, grid, dim3(AG_THREADS), 0, s, b, (const uint8_t*)block, (uint8_t*)mask_out, counts,
                         col_blocks);
    U2_CHECK_LAUNCH();
  }
  if (windows) {
    hipLaunchKernelGGL(aug_boxes_kernel, dim3((unsigned)((num_counts + AG_THREADS - 1) / AG_THREADS)), dim3(AG_THREADS), 0, s, boxes,
                       num_counts, 1);
    U2_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int u2_aug_rle_masks(const void* block, long long block_bytes, const void* tables_host, void* mask_out,
                                long long mask_out_bytes, int* counts, int num_counts, const U2AugImage* images, int num_images,
                                void* stream) {
  return rle_masks_launch(block, block_bytes, tables_host, mask_out, mask_out_bytes, counts, nullptr, num_counts, images, nullptr,
                          num_images, stream);
}

extern "C" int u2_aug_rle_masks_boxes(const void* block, long long block_bytes, const void* tables_host, void* mask_out,
                                      long long mask_out_bytes, int* counts, int* boxes, int num_counts, const U2AugImage* images,
                                      const U2AugWindow* windows, int num_images, void* stream) {
  if (num_images > 0 && !windows) return -1;
  return rle_masks_launch(block, block_bytes, tables_host, mask_out, mask_out_bytes, counts, boxes, num_counts, images, windows,
                          num_images, stream);
}
