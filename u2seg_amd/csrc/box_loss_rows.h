// The per-row arithmetic of the box regression losses, shared by the kernels of losses.hip that evaluate them: the box heads'
// class-agnostic and class-specific forms and the RPN's per-level kernel.  One row = one predicted set of four deltas against
// its source box (proposal or anchor) and its matched ground truth; the caller decides which rows count and where the four
// gradients go.  fp32 throughout, same operation order as box_regression.py:43-116 and layers/losses.py:5-133.
#pragma once
#include "u2seg_hip.h"

// ------------------------------------------------------------------------------------------------
// Box coding helpers (fp32, same operation order as box_regression.py:43-116)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void get_deltas(const float* s, const float* t, float wx, float wy, float ww, float wh, float* d) {
  const float sw = s[2] - s[0], sh = s[3] - s[1];
  const float scx = s[0] + 0.5f * sw, scy = s[1] + 0.5f * sh;
  const float tw = t[2] - t[0], th = t[3] - t[1];
  const float tcx = t[0] + 0.5f * tw, tcy = t[1] + 0.5f * th;
  d[0] = wx * (tcx - scx) / sw;
  d[1] = wy * (tcy - scy) / sh;
  d[2] = ww * logf(tw / sw);
  d[3] = wh * logf(th / sh);
}

// ------------------------------------------------------------------------------------------------
// The regression losses other than plain L1 (box_regression.py:310-369).
// SMOOTH_L1: on pred - get_deltas(src, gt); beta == 0 is plain L1 (no |d| lies below it).  GIOU / DIOU / CIOU: the box is
// decoded as apply_deltas does (box_regression.py:78-116), the loss of layers/losses.py:5-133 is evaluated against gt
// (GIoU: 1 - I/(U + eps) + (C - U)/(C + eps)) and its gradient is taken back through the decode by hand: d/dx1 .. d/dy2 of the
// loss, then centre / size, then the deltas.  torch's max / min hand half the gradient to each side of a tie; tie() does the
// same.  A clamped dw / dh passes nothing.
// ------------------------------------------------------------------------------------------------
constexpr float BOXLOSS_EPS = 1e-7f;

__device__ __forceinline__ float tie(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }  // d max(a, b) / da

template <int KIND>
__device__ __forceinline__ float iou_family_loss(const float* b, const float* g, float* gb) {
  const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
  const float x1g = g[0], y1g = g[1], x2g = g[2], y2g = g[3];
  // intersection, zero unless both overlaps are strictly positive
  const float iw = fminf(x2, x2g) - fmaxf(x1, x1g), ih = fminf(y2, y2g) - fmaxf(y1, y1g);
  const bool hit = ih > 0.f && iw > 0.f;
  const float I = hit ? iw * ih : 0.f;
  const float m = hit ? 1.f : 0.f;
  const float dI[4] = {-ih * tie(x1, x1g) * m, -iw * tie(y1, y1g) * m, ih * tie(x2g, x2) * m, iw * tie(y2g, y2) * m};
  const float bw = x2 - x1, bh = y2 - y1;
  const float dA[4] = {-bh, -bw, bh, bw};
  // smallest enclosing box
  const float cw = fmaxf(x2, x2g) - fminf(x1, x1g), ch = fmaxf(y2, y2g) - fminf(y1, y1g);
  const float dcw[4] = {-tie(x1g, x1), 0.f, tie(x2, x2g), 0.f};
  const float dch[4] = {0.f, -tie(y1g, y1), 0.f, tie(y2, y2g)};
  if constexpr (KIND == U2_BOXLOSS_GIOU) {
    const float U = bw * bh + (x2g - x1g) * (y2g - y1g) - I;
    const float C = cw * ch;
    const float iou = I / (U + BOXLOSS_EPS), mis = (C - U) / (C + BOXLOSS_EPS);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float dU = dA[q] - dI[q], dC = dcw[q] * ch + cw * dch[q];
      gb[q] = -(dI[q] - iou * dU) / (U + BOXLOSS_EPS) + ((dC - dU) - mis * dC) / (C + BOXLOSS_EPS);
    }
    return 1.f - iou + mis;
  } else {
    const float un = bw * bh + (x2g - x1g) * (y2g - y1g) - I + BOXLOSS_EPS;
    const float iou = I / un;
    const float diag = cw * cw + ch * ch + BOXLOSS_EPS;
    const float ex = (x2 + x1) / 2.f - (x1g + x2g) / 2.f, ey = (y2 + y1) / 2.f - (y1g + y2g) / 2.f;
    const float dist = ex * ex + ey * ey;
    const float term = dist / diag;
    const float ddist[4] = {ex, ey, ex, ey};
    float av = 0.f, dvw = 0.f, dvh = 0.f;   // CIoU: alpha v and alpha dv/d(width, height) of the decoded box
    if constexpr (KIND == U2_BOXLOSS_CIOU) {
      const float k = 4.f / (3.14159265358979323846f * 3.14159265358979323846f);
      const float ratio = bw / bh;
      const float da = atanf((x2g - x1g) / (y2g - y1g)) - atanf(ratio);
      const float v = k * da * da;
      const float alpha = v / (1.f - iou + v + BOXLOSS_EPS);   // a constant of the gradient (no_grad in the reference)
      const float dvdr = -2.f * k * da / (1.f + ratio * ratio);
      av = alpha * v;
      dvw = alpha * dvdr / bh;
      dvh = -alpha * dvdr * ratio / bh;
    }
    const float dshape[4] = {-dvw, -dvh, dvw, dvh};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float dU = dA[q] - dI[q], ddiag = 2.f * (cw * dcw[q] + ch * dch[q]);
      gb[q] = -(dI[q] - iou * dU) / un + (ddist[q] - term * ddiag) / diag + dshape[q];
    }
    return 1.f - iou + term + av;
  }
}

// One row: d = the four predicted deltas, p = the source box, g = the matched ground truth.  The row's loss is added to `l`
// (smooth-L1: coordinate by coordinate, in order) and gd receives d loss / d d, not yet scaled.
template <int KIND>
__device__ __forceinline__ void box_loss_row(const float* d, const float* p, const float* g, float wx, float wy, float ww,
                                             float wh, float beta, float scale_clamp, float& l, float* gd) {
  if constexpr (KIND == U2_BOXLOSS_SMOOTH_L1) {
    float tgt[4];
    get_deltas(p, g, wx, wy, ww, wh, tgt);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float df = d[q] - tgt[q], n = fabsf(df);
      l += n < beta ? 0.5f * n * n / beta : n - 0.5f * beta;
      gd[q] = n < beta ? df / beta : (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f));
    }
  } else {
    const float pw = p[2] - p[0], ph = p[3] - p[1];
    const float cx = p[0] + 0.5f * pw, cy = p[1] + 0.5f * ph;
    const float dx = d[0] / wx, dy = d[1] / wy;
    float dw = d[2] / ww, dh = d[3] / wh;
    const bool open_w = dw <= scale_clamp, open_h = dh <= scale_clamp;   // clamp(max =) passes the gradient up to equality
    dw = fminf(dw, scale_clamp);
    dh = fminf(dh, scale_clamp);
    const float pcx = dx * pw + cx, pcy = dy * ph + cy;
    const float bw = expf(dw) * pw, bh = expf(dh) * ph;
    const float b[4] = {pcx - 0.5f * bw, pcy - 0.5f * bh, pcx + 0.5f * bw, pcy + 0.5f * bh};
    float gb[4];
    l += iou_family_loss<KIND>(b, g, gb);
    gd[0] = (gb[0] + gb[2]) * pw / wx;
    gd[1] = (gb[1] + gb[3]) * ph / wy;
    gd[2] = open_w ? 0.5f * (gb[2] - gb[0]) * bw / ww : 0.f;
    gd[3] = open_h ? 0.5f * (gb[3] - gb[1]) * bh / wh : 0.f;
  }
}
