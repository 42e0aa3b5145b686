// The stem's input window, shared by the im2col kernel (pool_resize.hip) and the direct stem kernels (stem_conv.hip): one
// work-group serves a patch of ST_TH x ST_TW output pixels of the 7x7 / stride-2 / pad-3 convolution, whose taps lie in a
// ST_IH x ST_IW x 3 window of the image.  The window is normalised once - (x - mean) / std, one bf16 rounding per pixel, zero for
// the padding and for the canvas beyond the image - and kept in LDS as tile[(c * ST_IH + row) * PITCH + x].
#pragma once
#include "common.h"

constexpr int ST_TH = 8, ST_TW = 32, ST_IH = 2 * ST_TH + 5, ST_IW = 2 * ST_TW + 5;
struct StemImages { const void* img[32]; int h[32]; int w[32]; };

// Element (c, row r, column x) of the window whose first input pixel is (iy0, ix0): its place in the tile and in the image.
// `in` = the element is a pixel of the image (columns from ST_IW on, which the direct kernels fill as well, are not).
struct StemWindowElem { int lds; size_t src; bool in; };
template <int PITCH>
__device__ __forceinline__ StemWindowElem stem_window_elem(int c, int r, int x, int h, int w, int iy0, int ix0) {
  const int iy = iy0 + r, ix = ix0 + x;
  StemWindowElem e;
  e.lds = (c * ST_IH + r) * PITCH + x;
  e.in = x < ST_IW && iy >= 0 && iy < h && ix >= 0 && ix < w;
  e.src = (size_t)c * ((size_t)h * w) + (size_t)iy * w + ix;
  return e;
}
// the one expression every stem path normalises a pixel with
template <typename T> __device__ __forceinline__ bf16_t stem_window_value(T raw, bool in, float mean, float stdv) {
  return f2bf(in ? ((float)raw - mean) / stdv : 0.f);
}

// the whole window, by 256 threads; the caller synchronises
template <typename T, int PITCH>
__device__ __forceinline__ void stem_stage_window(bf16_t* tile, const T* __restrict__ img, int h, int w, int iy0, int ix0,
                                                  const float* __restrict__ mean, const float* __restrict__ stdv, int tid) {
  for (int i = tid; i < 3 * ST_IH * ST_IW; i += 256) {
    const int c = i / (ST_IW * ST_IH);
    const StemWindowElem e = stem_window_elem<PITCH>(c, (i / ST_IW) % ST_IH, i % ST_IW, h, w, iy0, ix0);
    const T raw = e.in ? img[e.src] : (T)0;
    tile[e.lds] = stem_window_value<T>(raw, e.in, mean[c], stdv[c]);
  }
}
