// Test-time augmentation (gfx950): the box maps between a view and the original image, the mean of the views' mask
// probabilities, and the mean of the views' semantic logits.  Contract: include/u2seg_hip.h, design: DESIGN.md sections 19, 20.
//
// Element-wise kernels, one thread per box or per output pixel.  Their arithmetic restates what the reference does with
// numpy on float32 arrays (modeling/test_time_augmentation.py:244-307 through fvcore's apply_box): every step is one float32
// operation with one rounding - the build has -ffp-contract=off, nothing below may fuse - so that the host definition in
// modeling/test_time_augmentation.py and these kernels agree bit for bit.
#include "common.h"
#include "u2seg_hip.h"

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_DESC = 5;  // floats per view: s1x, s1y, s2x, s2y, width

// numpy's min / max over the corners: a NaN in either operand gives NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float np_min(float a, float b) { return (a != a || b != b) ? (a + b) : (a < b ? a : b); }
__device__ __forceinline__ float np_max(float a, float b) { return (a != a || b != b) ? (a + b) : (a > b ? a : b); }
// Tensor.clamp(min=0, max=hi): NaN stays NaN
__device__ __forceinline__ float clamp0(float v, float hi) {
  if (v != v) return v;
  v = v < 0.f ? 0.f : v;
  return v > hi ? hi : v;
}
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }  // false for NaN and +-inf

// Transform.apply_box: every step maps the corners and takes their bounding box.  For a resize that only matters when x0 > x1
// or one of them is a NaN (then both become one), but it is what the definition does.
__device__ __forceinline__ void corners(float& lo, float& hi, float a, float b) {
  lo = np_min(a, b);
  hi = np_max(a, b);
}
__device__ __forceinline__ void scale_box(float4& b, float sx, float sy) {
  corners(b.x, b.z, b.x * sx, b.z * sx);
  corners(b.y, b.w, b.y * sy, b.w * sy);
}
// HFlipTransform: the corners' x become width - x
__device__ __forceinline__ void flip_box(float4& b, float width) {
  corners(b.x, b.z, width - b.x, width - b.z);
  corners(b.y, b.w, b.y, b.w);
}

// view -> original: flip, then the two scales.  grid: rows
__global__ __launch_bounds__(TT_THREADS) void tta_boxes_to_original_kernel(
    const float4* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ row_view,
    const float* __restrict__ view_desc, const int* __restrict__ view_flip, const int* __restrict__ view_image,
    const float* __restrict__ image_clip, float4* __restrict__ out_boxes, unsigned char* __restrict__ out_cand, int N,
    float score_thresh) {
  const int i = blockIdx.x * TT_THREADS + threadIdx.x;
  if (i >= N) return;
  const int v = row_view[i];
  const float* d = view_desc + (size_t)v * TT_DESC;
  float4 b = boxes[i];
  if (view_flip[v]) flip_box(b, d[4]);
  scale_box(b, d[0], d[1]);
  scale_box(b, d[2], d[3]);
  const float s = scores[i];
  out_cand[i] = (finite_f(b.x) && finite_f(b.y) && finite_f(b.z) && finite_f(b.w) && finite_f(s) && s > score_thresh) ? 1 : 0;
  const float* lim = image_clip + 2 * (size_t)view_image[v];  // (width, height)
  b.x = clamp0(b.x, lim[0]); b.z = clamp0(b.z, lim[0]);
  b.y = clamp0(b.y, lim[1]); b.w = clamp0(b.w, lim[1]);
  out_boxes[i] = b;
}

// original -> view: the two scales, then the flip; no clip.  grid (row blocks of the image with most rows, views)
__global__ __launch_bounds__(TT_THREADS) void tta_boxes_to_views_kernel(
    const float4* __restrict__ boxes, const int* __restrict__ image_rows, const float* __restrict__ view_desc,
    const int* __restrict__ view_flip, const int* __restrict__ view_image, const long long* __restrict__ view_out_row,
    float4* __restrict__ out) {
  const int v = blockIdx.y;
  const int im = view_image[v];
  const int first = image_rows[im], R = image_rows[im + 1] - first;
  const int r = blockIdx.x * TT_THREADS + threadIdx.x;
  if (r >= R) return;
  const float* d = view_desc + (size_t)v * TT_DESC;
  float4 b = boxes[first + r];
  scale_box(b, d[0], d[1]);
  scale_box(b, d[2], d[3]);
  if (view_flip[v]) flip_box(b, d[4]);
  out[view_out_row[v] + r] = b;
}

// grid (pixel blocks of the image with most rows, images); a thread owns one output pixel and adds the views in order
__global__ __launch_bounds__(TT_THREADS) void tta_reduce_masks_kernel(
    const float* const* __restrict__ view_prob, const int* __restrict__ view_flip, const int* __restrict__ image_views,
    const int* __restrict__ image_rows, float* __restrict__ out, int P) {
  const int im = blockIdx.y;
  const int first = image_rows[im], R = image_rows[im + 1] - first;
  const int v0 = image_views[im], v1 = image_views[im + 1];
  const long long pp = (long long)P * P, total = (long long)R * pp;
  const long long e = (long long)blockIdx.x * TT_THREADS + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % P);
  const long long row = e - x;          // offset of (r, y, 0) in the image's [R][P][P] block
  float acc = 0.f;                      // 0 + a == a: the sum is a[0] + a[1] + ... in view order
  for (int v = v0; v < v1; ++v) acc = acc + view_prob[v][row + (view_flip[v] ? P - 1 - x : x)];
  out[(long long)first * pp + e] = acc / (float)(v1 - v0);
}

// ---- the mean of the views' semantic logits ---------------------------------------------------------------
// acc[c][oy][ox] (+)= sem_seg_postprocess(view)[c][oy][flip ? W - 1 - ox : ox] for the views of a call in order, the running sum
// of a pixel's C classes in registers; with divisor > 0 the sum is divided and its argmax written.  The term is
// bilinear_resize_f32_kernel's value (bilinear_tap / bilinear_mix of common.h), or the source element itself where the window
// is H x W already (sem_seg_postprocess returns its input there: 0 * inf would make a NaN of a neighbouring inf).
constexpr int TT_MAXVIEWS = 32;  // views per launch (kernel arguments); the launcher splits longer lists, which changes no bit

struct SemView {
  long long cs, rs;  // channel and row stride of the [C][h][w] window, in elements
  float sch, scw;    // (float)h / (float)H, (float)w / (float)W
  int h, w, flip, identity;
};
struct SemViews {
  SemView v[TT_MAXVIEWS];
};

// grid: pixel blocks; a thread owns one output pixel (neighbouring threads neighbouring x), computes the taps and weights once
// per view and loops over the classes
template <int CMAX>
__global__ __launch_bounds__(TT_THREADS) void tta_accumulate_sem_seg_kernel(const float* const* __restrict__ view_logits,
                                                                            const SemViews views, int n, float* __restrict__ acc_mem,
                                                                            long long* __restrict__ amax, int C, int H, int W,
                                                                            int first, float divisor) {
  const long long hw = (long long)H * W;
  const long long i = (long long)blockIdx.x * TT_THREADS + threadIdx.x;
  if (i >= hw) return;
  const int ox = (int)(i % W), oy = (int)(i / W);
  float acc[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = (!first && c < C) ? acc_mem[c * hw + i] : 0.f;
  for (int v = 0; v < n; ++v) {
    const SemView d = views.v[v];
    const float* __restrict__ src = view_logits[v];
    const int sx = d.flip ? W - 1 - ox : ox;
    const bool start = first && v == 0;  // the sum starts from the first term: nothing is added to it
    if (d.identity) {
      const float* p = src + oy * d.rs + sx;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) {
          const float t = p[c * d.cs];
          acc[c] = start ? t : acc[c] + t;
        }
    } else {
      const BilinearTap y = bilinear_tap(d.sch, oy, d.h), x = bilinear_tap(d.scw, sx, d.w);
      const float* p00 = src + y.i0 * d.rs + x.i0;
      const float* p01 = src + y.i0 * d.rs + x.i1;
      const float* p10 = src + y.i1 * d.rs + x.i0;
      const float* p11 = src + y.i1 * d.rs + x.i1;
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) {
          const long long o = c * d.cs;
          const float t = bilinear_mix(y, x, p00[o], p01[o], p10[o], p11[o]);
          acc[c] = start ? t : acc[c] + t;
        }
    }
  }
  float best = 0.f;
  int besti = 0;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) {
      float f = acc[c];
      if (divisor > 0.f) f = f / divisor;
      acc_mem[c * hw + i] = f;
      // torch.argmax / numpy.argmax: the first maximum, a NaN counts as the largest value
      if (c == 0 || f > best || (f != f && best == best)) { best = f; besti = c; }
    }
  if (amax && divisor > 0.f) amax[i] = besti;
}

unsigned blocks_of(long long items) { return (unsigned)((items + TT_THREADS - 1) / TT_THREADS); }

}  // namespace

extern "C" int u2_tta_boxes_to_original(const float* boxes, const float* scores, const int* row_view, const float* view_desc,
                                        const int* view_flip, const int* view_image, const float* image_clip, float* out_boxes,
                                        void* out_cand, int num_rows, int num_views, int num_images, float score_thresh,
                                        void* stream) {
  if (num_rows < 0 || num_views < 0 || num_images < 0) return -1;
  if (num_rows == 0) return 0;
  if (num_views < 1 || num_images < 1 || !boxes || !scores || !row_view || !view_desc || !view_flip || !view_image || !image_clip ||
      !out_boxes || !out_cand || ((uintptr_t)boxes & 15) || ((uintptr_t)out_boxes & 15))
    return -1;
  hipLaunchKernelGGL(tta_boxes_to_original_kernel, dim3(blocks_of(num_rows)), dim3(TT_THREADS), 0, (hipStream_t)stream,
                     (const float4*)boxes, scores, row_view, view_desc, view_flip, view_image, image_clip, (float4*)out_boxes,
                     (unsigned char*)out_cand, num_rows, score_thresh);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_tta_boxes_to_views(const float* boxes, const int* image_rows, const float* view_desc, const int* view_flip,
                                     const int* view_image, const long long* view_out_row, float* out, int max_rows, int num_views,
                                     int num_images, void* stream) {
  if (max_rows < 0 || num_views < 0 || num_images < 0 || num_views > 65535) return -1;
  if (max_rows == 0 || num_views == 0) return 0;
  if (num_images < 1 || !boxes || !image_rows || !view_desc || !view_flip || !view_image || !view_out_row || !out ||
      ((uintptr_t)boxes & 15) || ((uintptr_t)out & 15))
    return -1;
  hipLaunchKernelGGL(tta_boxes_to_views_kernel, dim3(blocks_of(max_rows), (unsigned)num_views), dim3(TT_THREADS), 0,
                     (hipStream_t)stream, (const float4*)boxes, image_rows, view_desc, view_flip, view_image, view_out_row,
                     (float4*)out);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_tta_reduce_masks(const void* view_prob, const int* view_flip, const int* image_views, const int* image_rows,
                                   float* out, int max_rows, int min_views, int num_images, int P, void* stream) {
  if (max_rows < 0 || num_images < 0 || P < 1 || P > 4096) return -1;
  if (max_rows == 0 || num_images == 0) return 0;
  if (min_views < 1 || num_images > 65535 || !view_prob || !view_flip || !image_views || !image_rows || !out) return -1;
  const long long items = (long long)max_rows * P * P;
  if (items >= (1LL << 31) * TT_THREADS) return -1;
  hipLaunchKernelGGL(tta_reduce_masks_kernel, dim3(blocks_of(items), (unsigned)num_images), dim3(TT_THREADS), 0,
                     (hipStream_t)stream, (const float* const*)view_prob, view_flip, image_views, image_rows, out, P);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_tta_accumulate_sem_seg(const void* view_logits, const long long* views, int n, float* acc, int first, int divisor,
                                         long long* argmax, int C, int H, int W, void* stream) {
  if (C < 1 || C > 64 || n < 1 || H < 1 || W < 1 || divisor < 0 || !view_logits || !views || !acc) return -1;
  const long long hw = (long long)H * W;
  if (hw >= (1LL << 31) * TT_THREADS) return -1;
  for (int v = 0; v < n; ++v) {
    const long long* d = views + 5 * (size_t)v;  // h, w, row stride, channel stride, flip
    if (d[0] < 1 || d[1] < 1 || d[0] > 0x7fffffffLL || d[1] > 0x7fffffffLL || d[2] < d[1] || d[3] < 0) return -1;
  }
  const float* const* ptrs = (const float* const*)view_logits;
  for (int v0 = 0; v0 < n; v0 += TT_MAXVIEWS) {
    const int nv = n - v0 < TT_MAXVIEWS ? n - v0 : TT_MAXVIEWS;
    const bool last = v0 + nv == n;
    SemViews a;
    for (int k = 0; k < nv; ++k) {
      const long long* d = views + 5 * (size_t)(v0 + k);
      SemView& s = a.v[k];
      s.h = (int)d[0]; s.w = (int)d[1]; s.rs = d[2]; s.cs = d[3]; s.flip = d[4] != 0;
      s.identity = s.h == H && s.w == W;
      s.sch = (float)s.h / (float)H; s.scw = (float)s.w / (float)W;  // as u2_bilinear_resize_f32 forms its scales
    }
    for (int k = nv; k < TT_MAXVIEWS; ++k) a.v[k] = a.v[0];
    const int fst = first && v0 == 0;
    const float div = last ? (float)divisor : 0.f;
    long long* am = last ? argmax : nullptr;
    const dim3 grid(blocks_of(hw)), block(TT_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (C <= 8)
      hipLaunchKernelGGL(tta_accumulate_sem_seg_kernel<8>, grid, block, 0, s, ptrs + v0, a, nv, acc, am, C, H, W, fst, div);
    else if (C <= 32)
      hipLaunchKernelGGL(tta_accumulate_sem_seg_kernel<32>, grid, block, 0, s, ptrs + v0, a, nv, acc, am, C, H, W, fst, div);
    else
      hipLaunchKernelGGL(tta_accumulate_sem_seg_kernel<64>, grid, block, 0, s, ptrs + v0, a, nv, acc, am, C, H, W, fst, div);
    U2_CHECK_LAUNCH();
  }
  return 0;
}
