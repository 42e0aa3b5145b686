// Loss kernels (fp32 arithmetic on bf16 logits; forward and the logit gradient produced in one pass).
//
// Replaces (reference file:line):
//   SemSegFPNHead.losses: bilinear x4 + F.cross_entropy(mean, ignore 255)   meta_arch/semantic_seg.py:255-267
//   FastRCNNOutputLayers.losses: cross_entropy(mean) + box_reg_loss (L1)     roi_heads/fast_rcnn.py:307-347,424-463
//   mask_rcnn_loss: gt-class channel gather + BCE-with-logits(mean)          roi_heads/mask_head.py:33-112
//     (fused with the 1x1 predictor conv of mask_head.py:258 so only the gt-class channel is computed)
//   RPN.losses: BCE-with-logits(sum) + L1 over positives, / (batch_per_image * N)   proposal_generator/rpn.py:366-429
//     (and with MODEL.RPN.BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA / BBOX_REG_WEIGHTS: smooth-L1, GIoU, DIoU, CIoU)
//   _dense_box_regression_loss, class agnostic and class specific                    modeling/box_regression.py:310-369
//     (the per-row arithmetic of the three kernels that evaluate it: box_loss_rows.h)
//   Box2BoxTransform.get_deltas                                               modeling/box_regression.py:43-76
#include "common.h"
#include "u2seg_hip.h"
#include "box_loss_rows.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Semantic head loss: logits [B][h][w][LP] bf16 at stride 4, targets uint8 [B][4h][4w].
//
// "Owner computes": a work-group owns a 15 x 7 block of low-resolution logits and evaluates every full-resolution
// pixel that touches them (64 x 32 pixels: 60 x 28 of its own plus a halo its neighbours evaluate too, 1.22x the
// minimum work).  The logit gradient of the owned block is accumulated in LDS and written once with plain stores:
// no global atomics, no pre-zeroed accumulator.  A pixel's loss is counted by the group owning its upper-left tap.
//
// Work split: with scale 4 and align_corners=False the 4 x 4 pixels x = 4g+2..4g+5, y = 4k+2..4k+5 share one 2 x 2
// set of taps (g, g+1) x (k, k+1).  Four adjacent lanes take such a cell, 8 classes each (softmax max / sum cross the
// four lanes with two DPP shuffles): the 4 taps x 8 classes are read from LDS once, the 16 pixels run out of
// registers, and the cell's gradient is merged in registers into 4 taps x 8 values before it touches LDS.
// ------------------------------------------------------------------------------------------------
constexpr int SS_OW = 15, SS_OH = 7;                 // owned taps per work-group
constexpr int SS_LW = SS_OW + 2, SS_LH = SS_OH + 2;  // staged taps (one halo ring)
constexpr int SS_MAXC = 32, SS_PITCH = 36;           // 36 floats: 16-byte aligned rows, tap columns on distinct banks
constexpr int SS_ZPITCH = 40;                        // the staged logits stay bf16 (round 5): 80-byte rows, 12 KB instead of 22 KB -
                                                     // four work-groups per CU instead of three

// reductions over the 4 lanes of a quad: DPP quad_perm [1,0,3,2] (0xB1) and [2,3,0,1] (0x4E)
template <int CTRL>
__device__ __forceinline__ float quad_swap(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, quad_swap<0xB1>(v));
  return fmaxf(v, quad_swap<0x4E>(v));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += quad_swap<0xB1>(v);
  return v + quad_swap<0x4E>(v);
}

__global__ __launch_bounds__(256, 4) void semseg_ce_kernel(const bf16_t* __restrict__ logits, const uint8_t* __restrict__ target,
                                                        float* __restrict__ grad_acc, float* __restrict__ loss_sum,
                                                        float* __restrict__ valid_cnt, int B, int h, int w, int LP, int NC,
                                                        int ignore) {
  __shared__ __attribute__((aligned(16))) bf16_t zt[SS_LH * SS_LW * SS_ZPITCH];
  __shared__ __attribute__((aligned(16))) float gt[SS_LH * SS_LW * SS_PITCH];
  __shared__ __attribute__((aligned(16))) uint8_t lab[32 * 64];  // the tile's labels; `ignore` outside the image
  __shared__ float red[4];
  const int H = 4 * h, W = 4 * w;
  const int b = blockIdx.z;
  const int ox0 = (int)blockIdx.x * SS_OW, oy0 = (int)blockIdx.y * SS_OH;  // first owned tap
  const int lx0 = ox0 - 1, ly0 = oy0 - 1;                                  // first staged tap
  const int tid = threadIdx.x;
  {  // labels: 32 rows x 64 pixels starting at (4*oy0 - 2, 4*ox0 - 2); rows are 2-byte aligned in memory
    const int px0 = 4 * ox0 - 2, py0 = 4 * oy0 - 2;
    for (int i = tid; i < 32 * 32; i += 256) {
      const int r = i >> 5, cpair = (i & 31) * 2;
      const int y = py0 + r, x = px0 + cpair;
      uint8_t l0 = (uint8_t)ignore, l1 = (uint8_t)ignore;
      if (y >= 0 && y < H && x >= 0 && x + 1 < W) {
        const unsigned short two = *reinterpret_cast<const unsigned short*>(target + ((size_t)b * H + y) * W + x);
        l0 = (uint8_t)(two & 0xFF);
        l1 = (uint8_t)(two >> 8);
      }
      lab[r * 64 + cpair] = l0;
      lab[r * 64 + cpair + 1] = l1;
    }
  }
  for (int i = tid; i < SS_LH * SS_LW * (SS_MAXC / 8); i += 256) {  // logits: 16-byte chunks -> fp32, zero past NC
    const int ch = i % (SS_MAXC / 8);
    const int t = i / (SS_MAXC / 8);
    const int tx = t % SS_LW, ty = t / SS_LW;
    const int lx = min(max(lx0 + tx, 0), w - 1), ly = min(max(ly0 + ty, 0), h - 1);
    bf16_t v[8];
    if (ch * 8 < LP) {
      *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(logits + (((size_t)b * h + ly) * w + lx) * LP + ch * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (ch * 8 + e < NC) ? v[e] : (bf16_t)0;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0;
    }
    float* gd = gt + t * SS_PITCH + ch * 8;
    *reinterpret_cast<uint4*>(zt + t * SS_ZPITCH + ch * 8) = *reinterpret_cast<const uint4*>(v);
    *reinterpret_cast<float4*>(gd) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(gd + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  const int cj = tid & 3;          // class group: classes 8cj .. 8cj+7
  const int qx = (tid >> 2) & 15;  // cell column inside the tile
  const int wv = tid >> 6;
  const int gx = lx0 + qx;         // cell column: pixels 4gx+2 .. 4gx+5, taps gx and gx+1
  bool cvalid[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cvalid[e] = cj * 8 + e < NC;
  float my_loss = 0.f, my_cnt = 0.f;

#pragma unroll 1
  for (int cy = wv; cy < SS_OH + 1; cy += 4) {  // cell row: pixels 4gy+2 .. 4gy+5, taps gy and gy+1
    const int gy = ly0 + cy;
    if (gx >= w || gy >= h) continue;
    // tap coordinates of the cell (clamped exactly as the per-pixel formulas below would produce them)
    const int x0 = max(gx, 0), y0 = max(gy, 0);
    const int x1 = x0 + (x0 < w - 1 ? 1 : 0), y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const int t00 = (y0 - ly0) * SS_LW + (x0 - lx0), t01 = (y0 - ly0) * SS_LW + (x1 - lx0);
    const int t10 = (y1 - ly0) * SS_LW + (x0 - lx0), t11 = (y1 - ly0) * SS_LW + (x1 - lx0);
    const int i00 = t00 * SS_PITCH + cj * 8, i01 = t01 * SS_PITCH + cj * 8;   // the taps' rows of the gradient tile
    const int i10 = t10 * SS_PITCH + cj * 8, i11 = t11 * SS_PITCH + cj * 8;
    // the four taps stay packed (16 registers instead of 32: the kernel is compiled for four waves per SIMD) and are widened
    // where a pixel column uses them
    bf16_t h00[8], h01[8], h10[8], h11[8];
    *reinterpret_cast<uint4*>(h00) = *reinterpret_cast<const uint4*>(zt + t00 * SS_ZPITCH + cj * 8);
    *reinterpret_cast<uint4*>(h01) = *reinterpret_cast<const uint4*>(zt + t01 * SS_ZPITCH + cj * 8);
    *reinterpret_cast<uint4*>(h10) = *reinterpret_cast<const uint4*>(zt + t10 * SS_ZPITCH + cj * 8);
    *reinterpret_cast<uint4*>(h11) = *reinterpret_cast<const uint4*>(zt + t11 * SS_ZPITCH + cj * 8);
    const bool own_cell = y0 >= oy0 && y0 < oy0 + SS_OH && x0 >= ox0 && x0 < ox0 + SS_OW;
    unsigned labrow[4];  // the cell's 4 x 4 labels: row r = bytes of labrow[r]
#pragma unroll
    for (int r = 0; r < 4; ++r) labrow[r] = *reinterpret_cast<const unsigned*>(lab + (cy * 4 + r) * 64 + qx * 4);
    float a00[8], a01[8], a10[8], a11[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a00[e] = 0.f; a01[e] = 0.f; a10[e] = 0.f; a11[e] = 0.f; }
    bool any = false;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      const int x = 4 * gx + 2 + i;
      const float sx = fmaxf((x + 0.5f) * 0.25f - 0.5f, 0.f);
      const float lx = sx - (float)(int)sx, hx = 1.f - lx;
      float p[8], q[8], u0[8], u1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // same association as ATen's upsample_bilinear2d: hy*(hx*v00 + lx*v01) + ly*(hx*v10 + lx*v11)
        p[e] = hx * bf2f(h00[e]) + lx * bf2f(h01[e]);
        q[e] = hx * bf2f(h10[e]) + lx * bf2f(h11[e]);
        u0[e] = 0.f;
        u1[e] = 0.f;
      }
#pragma unroll 1
      for (int r = 0; r < 4; ++r) {
        const int y = 4 * gy + 2 + r;
        const int t = (labrow[r] >> (8 * i)) & 0xFF;
        if (t == ignore) continue;  // also pixels outside the image; uniform over the four class lanes of the pixel
        any = true;
        const float sy = fmaxf((y + 0.5f) * 0.25f - 0.5f, 0.f);
        const float ly = sy - (float)(int)sy, hy = 1.f - ly;
        float z[8];
        float mx = -INFINITY, z_t = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          z[e] = cvalid[e] ? hy * p[e] + ly * q[e] : -INFINITY;
          mx = fmaxf(mx, z[e]);
          if (cj * 8 + e == t) z_t = z[e];
        }
        mx = quad_max(mx);
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { z[e] = __expf(z[e] - mx); se += z[e]; }  // exp(-inf) = 0 for the padding classes
        se = quad_sum(se);
        if (own_cell) {  // the lane holding class t subtracts z_t, lane 0 of the pixel adds the log-sum-exp
          my_loss -= z_t;
          if (cj == 0) { my_loss += mx + __logf(se); my_cnt += 1.f; }
        }
        const float inv = 1.f / se;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = z[e] * inv - (cj * 8 + e == t ? 1.f : 0.f);
          u0[e] += hy * g;
          u1[e] += ly * g;
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a00[e] += hx * u0[e];
        a01[e] += lx * u0[e];
        a10[e] += hx * u1[e];
        a11[e] += lx * u1[e];
      }
    }
    if (any) {
      // contributions to taps outside the owned block land in the (discarded) halo ring of gt
      const int o00 = i00, o01 = i01, o10 = i10, o11 = i11;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (cvalid[e]) {
          atomicAdd(&gt[o00 + e], a00[e]);
          atomicAdd(&gt[o01 + e], a01[e]);
          atomicAdd(&gt[o10 + e], a10[e]);
          atomicAdd(&gt[o11 + e], a11[e]);
        }
      }
    }
  }
  const float bl = block_sum_256(my_loss, red);
  const float bc = block_sum_256(my_cnt, red);
  if (tid == 0 && bc > 0.f) { atomicAdd(loss_sum, bl); atomicAdd(valid_cnt, bc); }
  __syncthreads();
  // every logit of the owned block is written exactly once (channels NC..LP-1 as zeros)
  for (int i = tid; i < SS_OH * SS_OW * LP; i += 256) {
    const int c = i % LP;
    const int t = i / LP;
    const int ox = t % SS_OW, oy = t / SS_OW;
    const int lx = ox0 + ox, ly = oy0 + oy;
    if (lx >= w || ly >= h) continue;
    const float g = c < NC ? gt[((oy + 1) * SS_LW + (ox + 1)) * SS_PITCH + c] : 0.f;
    grad_acc[(((size_t)b * h + ly) * w + lx) * LP + c] = g;
  }
}

// dlogits(bf16) = grad_acc * (*gscale) / (*valid_cnt)
__global__ __launch_bounds__(256) void scale_to_bf16_kernel(const float* __restrict__ acc, const float* __restrict__ num,
                                                            const float* __restrict__ den, float mult,
                                                            bf16_t* __restrict__ out, size_t n) {
  const float s = mult * (num ? *num : 1.f) / (den ? *den : 1.f);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = f2bf(acc[i] * s);
}

// ------------------------------------------------------------------------------------------------
// Row softmax cross-entropy: logits [R][LP] bf16 (NC valid columns), labels int64; one wave per row.
// loss_sum += sum_r (lse - z[label]);  dlogits[r][c] = (softmax - onehot) * gscale  (pad columns = 0)
//
// STATS (u2_softmax_ce_stats): the wave also forms pred = argmax over the NC valid columns (lowest index among equal maxima, as
// torch.argmax documents) and counts what fast_rcnn.py:88-115 logs, counters[0..4] += rows, pred == gt, fg (0 <= gt < bg),
// fg and pred == gt, fg and pred == bg.  The counts of the rows a wave walks stay in registers.  In the register-resident form
// the four waves of a work-group then meet in LDS and threads 0-4 send one integer atomic each (at most 512 x 5 per launch);
// the general form, one row per wave, sends them per wave.  The float arithmetic is that of the instantiation without STATS.
// ------------------------------------------------------------------------------------------------
constexpr int SC_ROWS = 0, SC_ACC = 1, SC_FG = 2, SC_FG_ACC = 3, SC_FN = 4;

struct CeCounts {
  int n[5] = {0, 0, 0, 0, 0};
  // best: the lowest column holding the row's maximum (INT_MAX when no column compared equal: a row of -inf, argmax 0)
  __device__ __forceinline__ void add(int best, int t, int bg) {
    const int pred = best == 0x7fffffff ? 0 : best;
    const bool fg = t >= 0 && t < bg;
    n[SC_ROWS] += 1;
    n[SC_ACC] += pred == t;
    n[SC_FG] += fg;
    n[SC_FG_ACC] += fg && pred == t;
    n[SC_FN] += fg && pred == bg;
  }
  // the four waves of a work-group meet in LDS and threads 0-4 send one atomic each: a quarter of the same-address atomics
  // (every thread of the work-group must arrive here)
  __device__ __forceinline__ void send_group(int* __restrict__ counters) const {
    __shared__ int part[4][5];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane < 5) {
      int mine = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) mine = lane == i ? n[i] : mine;
      part[wv][lane] = mine;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
      const int c = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
      if (c != 0) atomicAdd(counters + threadIdx.x, c);
    }
  }
  __device__ __forceinline__ void send(int lane, int* __restrict__ counters) const {
    int mine = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) mine = lane == i ? n[i] : mine;
    if (lane < 5 && mine != 0) atomicAdd(counters + lane, mine);
  }
};

template <bool STATS>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const bf16_t* __restrict__ logits, const long long* __restrict__ labels,
                                                         bf16_t* __restrict__ dlogits, float* __restrict__ loss_sum, int R,
                                                         int NC, int LP, float gscale, int* __restrict__ counters, int bg) {
  const int lane = threadIdx.x & 63;
  CeCounts cnt;
  if (LP <= 1024 && (LP & 7) == 0) {
    // a wave walks rows with the grid's stride and sends ONE atomic at the end: 8192 same-address atomics (one per row) were
    // the whole 0.11 ms of this kernel
    float loss_acc = 0.f;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < R; row += gridDim.x * 4) {
    const bf16_t* zr = logits + (size_t)row * LP;
    // the whole row in registers (<= 2 x 16 bytes per lane): one read of the logits instead of three passes of 2-byte loads
    const int chunks = LP >> 3;
    float v[2][8];
    float mx = -INFINITY;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int ch = it * 64 + lane;
      bf16_t raw[8];
      if (ch < chunks) *reinterpret_cast<uint4*>(raw) = *reinterpret_cast<const uint4*>(zr + ch * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[it][e] = (ch < chunks && ch * 8 + e < NC) ? bf2f(raw[e]) : -INFINITY;
        mx = fmaxf(mx, v[it][e]);
      }
    }
    mx = wave_max(mx);
    int best = 0x7fffffff;
    if constexpr (STATS) {
#pragma unroll
      for (int it = 1; it >= 0; --it)
#pragma unroll
        for (int e = 7; e >= 0; --e) {
          const int c = (it * 64 + lane) * 8 + e;
          if (c < NC && v[it][e] == mx) best = c;  // (walked downwards: the lane's lowest such column stays)
        }
      best = wave_imin(best);
    }
    float se = 0.f;
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[it][e] = __expf(v[it][e] - mx);  // exp(-inf) = 0 for the pad columns
        se += v[it][e];
      }
    se = wave_sum(se);
    const int t = (int)labels[row];
    const float inv = 1.f / se;
    bf16_t* dr = dlogits + (size_t)row * LP;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int ch = it * 64 + lane;
      if (ch < chunks) {
        bf16_t ov[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int c = ch * 8 + e;
          ov[e] = f2bf(c < NC ? (v[it][e] * inv - (c == t ? 1.f : 0.f)) * gscale : 0.f);
        }
        *reinterpret_cast<uint4*>(dr + ch * 8) = *reinterpret_cast<const uint4*>(ov);
      }
    }
    loss_acc += mx + __logf(se) - bf2f(zr[t]);
    if constexpr (STATS) cnt.add(best, t, bg);
    }
    if (lane == 0 && loss_acc != 0.f) atomicAdd(loss_sum, loss_acc);
    if constexpr (STATS) cnt.send_group(counters);
    return;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const bf16_t* zr = logits + (size_t)row * LP;
  float mx = -INFINITY;
  for (int c = lane; c < NC; c += 64) mx = fmaxf(mx, bf2f(zr[c]));
  mx = wave_max(mx);
  int best = 0x7fffffff;
  if constexpr (STATS) {
    for (int c = lane; c < NC && best == 0x7fffffff; c += 64)
      if (bf2f(zr[c]) == mx) best = c;
    best = wave_imin(best);
  }
  float se = 0.f;
  for (int c = lane; c < NC; c += 64) se += __expf(bf2f(zr[c]) - mx);
  se = wave_sum(se);
  const int t = (int)labels[row];
  const float inv = 1.f / se;
  bf16_t* dr = dlogits + (size_t)row * LP;
  for (int c = lane; c < LP; c += 64) {
    float g = 0.f;
    if (c < NC) g = (__expf(bf2f(zr[c]) - mx) * inv - (c == t ? 1.f : 0.f)) * gscale;
    dr[c] = f2bf(g);
  }
  if (lane == 0) atomicAdd(loss_sum, mx + __logf(se) - bf2f(zr[t]));
  if constexpr (STATS) {
    cnt.add(best, t, bg);
    cnt.send(lane, counters);
  }
}

// ------------------------------------------------------------------------------------------------
// Mask head: logit[n][p] = x[n][p][:] . Wp[cls_n][:] + bp[cls_n] (rounded to bf16 like the autocast conv),
// loss_sum += BCEwithLogits(logit, target);  dx = dlogit * Wp[cls];  dWp[cls] += sum_p dlogit x;  dbp[cls] += sum dlogit
// x: [N][P][C] bf16 (C = 256), target uint8 [N][P].  One workgroup per ROI, one wave per position.
//
// STATS (u2_mask_predict_bce_stats, the loss-only form): what mask_head.py:90-102 logs, from the rounded logit z and the target
// t of every position: incorrect = (z > 0) != (t != 0); counters[0..3] += incorrect & !t, incorrect & t, t != 0, 1.  A wave keeps
// its counts in registers, the four waves meet in four more columns of red[][] (integers, bit-cast), and threads 0-3 send one
// integer atomic each per work-group.
// ------------------------------------------------------------------------------------------------
constexpr int MC_FALSE_POS = 0, MC_FALSE_NEG = 1, MC_POS = 2, MC_TOTAL = 3;

template <bool STATS>
__global__ __launch_bounds__(256) void mask_predict_bce_kernel(const bf16_t* __restrict__ x, const float* __restrict__ Wp,
                                                               const float* __restrict__ bp, const long long* __restrict__ cls,
                                                               const uint8_t* __restrict__ target, bf16_t* __restrict__ dx,
                                                               float* __restrict__ dWp, float* __restrict__ dbp,
                                                               float* __restrict__ loss_sum, bf16_t* __restrict__ logit_out,
                                                               int P, int C, float gscale, int phased_side,
                                                               const float* __restrict__ gmul, int* __restrict__ counters) {
  __shared__ float red[4][STATS ? 264 : 260];
  int mc[4] = {0, 0, 0, 0};
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int k = (int)cls[n];
  // C == 256: 4 channels per lane; weights are rounded to bf16 like the autocast conv operand
  float wq[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) wq[e] = bf2f(f2bf(Wp[(size_t)k * C + lane * 4 + e]));
  const float bias = bf2f(f2bf(bp[k]));
  if (gmul) gscale *= *gmul;   // the upstream gradient of the loss (a device scalar): the backward launch
  float dw[4] = {0.f, 0.f, 0.f, 0.f};
  float db = 0.f, ls = 0.f;
  // round 6: blockIdx.y = a slice of the ROI's positions.  With one work-group per ROI a launch was 260 work-groups whose waves
  // walked 196 positions each, one dependent load -> wave sum -> store chain at a time: 0.18 ms for 104 MB.
  for (int p = wv + 4 * blockIdx.y; p < P; p += 4 * gridDim.y) {
    const size_t off = ((size_t)n * P + p) * C + lane * 4;
    bf16_t xv[4];
    *reinterpret_cast<uint2*>(xv) = *reinterpret_cast<const uint2*>(x + off);
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) d += bf2f(xv[e]) * wq[e];
    d = wave_sum(d);
    const float z = bf2f(f2bf(d + bias));
    // phased: position p of x / dx is (h, w, dy, dx) of the deconvolution's unshuffled output = pixel (2 h + dy, 2 w + dx) of the
    // target and of logit_out
    int o = p;
    if (phased_side) {
      const int S = phased_side >> 1, hw = p >> 2;
      const int h = hw / S, w = hw - h * S;
      o = (2 * h + ((p >> 1) & 1)) * phased_side + 2 * w + (p & 1);
    }
    const float t = (float)target[(size_t)n * P + o];
    // max(z,0) - z*t + log1p(exp(-|z|))
    ls += fmaxf(z, 0.f) - z * t + log1pf(__expf(-fabsf(z)));
    if constexpr (STATS) {
      const bool on = t != 0.f, wrong = (z > 0.f) != on;
      mc[MC_FALSE_POS] += wrong && !on;
      mc[MC_FALSE_NEG] += wrong && on;
      mc[MC_POS] += on;
      mc[MC_TOTAL] += 1;
    }
    const float sg = 1.f / (1.f + __expf(-z));
    const float g = (sg - t) * gscale;
    bf16_t ov[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ov[e] = f2bf(g * wq[e]);
      dw[e] += g * bf2f(xv[e]);
    }
    if (dx) *reinterpret_cast<uint2*>(dx + off) = *reinterpret_cast<const uint2*>(ov);
    db += g;
    if (logit_out && lane == 0) logit_out[(size_t)n * P + o] = f2bf(z);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wv][lane * 4 + e] = dw[e];
  if (lane == 0) { red[wv][256] = db; red[wv][257] = ls; }
  if constexpr (STATS) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wv][260 + i] = __int_as_float(mc[i]);
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  const float s = red[0][t] + red[1][t] + red[2][t] + red[3][t];
  if (dWp) atomicAdd(dWp + (size_t)k * C + t, s);
  if (t == 0) {
    if (dbp) atomicAdd(dbp + k, red[0][256] + red[1][256] + red[2][256] + red[3][256]);
    if (loss_sum) atomicAdd(loss_sum, red[0][257] + red[1][257] + red[2][257] + red[3][257]);
  }
  if constexpr (STATS) {
    if (t < 4) {
      const int c = __float_as_int(red[0][260 + t]) + __float_as_int(red[1][260 + t]) + __float_as_int(red[2][260 + t]) +
                    __float_as_int(red[3][260 + t]);
      if (c != 0) atomicAdd(counters + t, c);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// counters[0] += #(labels == 1), counters[1] += #(labels == 0) over n int8 labels (the RPN's subsampled anchor labels,
// rpn.py:396-403).  16 labels per load where the address allows it, a work-group's counts meet in LDS, two integer atomics
// per work-group.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void count_labels_i8_kernel(const int8_t* __restrict__ labels, long long n,
                                                              int* __restrict__ counters) {
  __shared__ int red[2][4];
  // [0, head): bytes in front of the first 16-byte boundary; [head, head + 16 * nvec): whole vectors; the rest: the tail
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(labels) & 15)) & 15);
  if (head > n) head = n;
  const long long nvec = (n - head) >> 4;
  const uint4* vec = reinterpret_cast<const uint4*>(labels + head);
  int ones = 0, zeros = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const uint4 q = vec[i];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const unsigned v = (w[k] >> (8 * b)) & 0xffu;
        ones += v == 1u;
        zeros += v == 0u;
      }
  }
  if (blockIdx.x == 0) {  // head and tail: fewer than 32 labels
    const long long tail0 = head + (nvec << 4);
    const long long rest = head + (n - tail0);
    for (long long i = threadIdx.x; i < rest; i += 256) {
      const int8_t v = labels[i < head ? i : tail0 + (i - head)];
      ones += v == 1;
      zeros += v == 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ones += __shfl_xor(ones, o, 64);
    zeros += __shfl_xor(zeros, o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[0][wv] = ones; red[1][wv] = zeros; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int c = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (c != 0) atomicAdd(counters + threadIdx.x, c);
  }
}

// RPN losses for one FPN level.  obj: [B][HW][LPo] (A valid cols), dlt: [B][HW][LPd] (4A valid cols),
// labels int8 [B][Atot] (-1 ignore / 0 / 1, already subsampled), match int32 [B][Atot], gt fp32 [B][G][4],
// anchors fp32 [HW*A][4] of this level.  Writes dobj/ddlt (bf16, same layouts, pads zero) and adds to loss[0:2].
// FUSED3: one 32-wide map holds both predictions of A = 3 anchors (columns 0-2 objectness, 3-14 deltas) and takes one gradient row

// objectness of one anchor with label t in {0, 1}: BCE-with-logits added to lc, the logit gradient returned
__device__ __forceinline__ bf16_t rpn_objectness(float z, float t, float gscale, float& lc) {
  lc += fmaxf(z, 0.f) - z * t + log1pf(__expf(-fabsf(z)));
  return f2bf((1.f / (1.f + __expf(-z)) - t) * gscale);
}

// one position's gradient rows: go_l[8] objectness, gd_l[16] deltas, pads zero; every column of the maps' rows is written
template <bool FUSED3>
__device__ __forceinline__ void rpn_store_grads(bf16_t* __restrict__ dobj, bf16_t* __restrict__ ddlt, size_t i, int LPo, int LPd,
                                                const bf16_t* go_l, const bf16_t* gd_l) {
  uint4* go = reinterpret_cast<uint4*>(dobj + i * LPo);
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  if (FUSED3) {
    bf16_t row[16];
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = go_l[c];
#pragma unroll
    for (int c = 0; c < 12; ++c) row[3 + c] = gd_l[c];
    row[15] = 0;
    go[0] = *reinterpret_cast<const uint4*>(row);
    go[1] = *reinterpret_cast<const uint4*>(row + 8);
    for (int c = 2; c < LPo / 8; ++c) go[c] = zero4;
    return;
  }
  uint4* gd = reinterpret_cast<uint4*>(ddlt + i * LPd);
  go[0] = *reinterpret_cast<const uint4*>(go_l);
  for (int c = 1; c < LPo / 8; ++c) go[c] = zero4;
  gd[0] = *reinterpret_cast<const uint4*>(gd_l);
  gd[1] = *reinterpret_cast<const uint4*>(gd_l + 8);
  for (int c = 2; c < LPd / 8; ++c) gd[c] = zero4;
}

template <bool FUSED3>
__global__ __launch_bounds__(256) void rpn_loss_level_kernel(const bf16_t* __restrict__ obj, const bf16_t* __restrict__ dlt,
                                                             const int8_t* __restrict__ labels, const int* __restrict__ match,
                                                             const float* __restrict__ gt, const float* __restrict__ anchors,
                                                             bf16_t* __restrict__ dobj, bf16_t* __restrict__ ddlt,
                                                             float* __restrict__ loss, int B, int HW, int A, int LPo, int LPd,
                                                             int Atot, int lvl_off, int G, float gscale) {
  __shared__ float red[4];
  float lc = 0.f, ll = 0.f;
  const size_t total = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / HW);
    const int pix = (int)(i - (size_t)b * HW);
    bf16_t go_l[8], gd_l[16];
#pragma unroll
    for (int c = 0; c < 8; ++c) go_l[c] = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) gd_l[c] = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= A) break;
      const int aidx = pix * A + a;
      const int lab = labels[(size_t)b * Atot + lvl_off + aidx];
      if (lab < 0) continue;
      go_l[a] = rpn_objectness(bf2f(obj[i * LPo + a]), (float)lab, gscale, lc);
      if (lab == 1) {
        const int g = match[(size_t)b * Atot + lvl_off + aidx];
        float d[4];
        get_deltas(anchors + (size_t)aidx * 4, gt + ((size_t)b * G + g) * 4, 1.f, 1.f, 1.f, 1.f, d);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float pr = bf2f(dlt[i * LPd + a * 4 + q]);
          const float df = pr - d[q];
          ll += fabsf(df);
          gd_l[a * 4 + q] = f2bf((df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f)) * gscale);
        }
      }
    }
    rpn_store_grads<FUSED3>(dobj, ddlt, i, LPo, LPd, go_l, gd_l);
  }
  const float s0 = block_sum_256(lc, red);
  const float s1 = block_sum_256(ll, red);
  if (threadIdx.x == 0) { atomicAdd(loss + 0, s0); atomicAdd(loss + 1, s1); }
}

// The same level with the localisation loss options (rpn.py:366-429 over box_regression.py:310-369): the positives' rows go
// through box_loss_row (box_loss_rows.h) with the anchor as the source box - smooth-L1 with any beta >= 0 on
// delta - get_deltas(anchor, gt; weights), or GIoU / DIoU / CIoU on apply_deltas(delta, anchor; weights, scale_clamp) with the
// gradient taken back through the decode.  Objectness, layouts and stores are rpn_loss_level_kernel's.
template <bool FUSED3, int KIND>
__global__ __launch_bounds__(256) void rpn_loss_level_opt_kernel(const bf16_t* __restrict__ obj, const bf16_t* __restrict__ dlt,
                                                                 const int8_t* __restrict__ labels, const int* __restrict__ match,
                                                                 const float* __restrict__ gt, const float* __restrict__ anchors,
                                                                 bf16_t* __restrict__ dobj, bf16_t* __restrict__ ddlt,
                                                                 float* __restrict__ loss, int B, int HW, int A, int LPo, int LPd,
                                                                 int Atot, int lvl_off, int G, float gscale, float wx, float wy,
                                                                 float ww, float wh, float beta, float scale_clamp) {
  __shared__ float red[4];
  float lc = 0.f, ll = 0.f;
  const size_t total = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int b = (int)(i / HW);
    const int pix = (int)(i - (size_t)b * HW);
    bf16_t go_l[8], gd_l[16];
#pragma unroll
    for (int c = 0; c < 8; ++c) go_l[c] = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) gd_l[c] = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= A) break;
      const int aidx = pix * A + a;
      const int lab = labels[(size_t)b * Atot + lvl_off + aidx];
      if (lab < 0) continue;
      go_l[a] = rpn_objectness(bf2f(obj[i * LPo + a]), (float)lab, gscale, lc);
      if (lab == 1) {
        const int g = match[(size_t)b * Atot + lvl_off + aidx];
        float d[4], gd[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = bf2f(dlt[i * LPd + a * 4 + q]);
        box_loss_row<KIND>(d, anchors + (size_t)aidx * 4, gt + ((size_t)b * G + g) * 4, wx, wy, ww, wh, beta, scale_clamp, ll, gd);
#pragma unroll
        for (int q = 0; q < 4; ++q) gd_l[a * 4 + q] = f2bf(gd[q] * gscale);
      }
    }
    rpn_store_grads<FUSED3>(dobj, ddlt, i, LPo, LPd, go_l, gd_l);
  }
  const float s0 = block_sum_256(lc, red);
  const float s1 = block_sum_256(ll, red);
  if (threadIdx.x == 0) { atomicAdd(loss + 0, s0); atomicAdd(loss + 1, s1); }
}

// Box-head regression loss (class agnostic): pred [R][LP] bf16 (4 valid), proposals/gt fp32 [R][4],
// labels int64 [R]; fg = 0 <= label < bg_label.  loss += sum_fg |pred - target|; dpred = sign * gscale.
__global__ __launch_bounds__(256) void box_reg_l1_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ prop,
                                                         const float* __restrict__ gtb, const long long* __restrict__ labels,
                                                         bf16_t* __restrict__ dpred, float* __restrict__ loss, int R, int LP,
                                                         int bg_label, float wx, float wy, float ww, float wh, float gscale) {
  __shared__ float red[4];
  float l = 0.f;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
    bf16_t* gp = dpred + (size_t)r * LP;
    for (int c = 0; c < LP; ++c) gp[c] = 0;
    const long long lab = labels[r];
    if (lab < 0 || lab >= bg_label) continue;
    float d[4];
    get_deltas(prop + (size_t)r * 4, gtb + (size_t)r * 4, wx, wy, ww, wh, d);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float df = bf2f(pred[(size_t)r * LP + q]) - d[q];
      l += fabsf(df);
      gp[q] = f2bf((df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f)) * gscale);
    }
  }
  const float s = block_sum_256(l, red);
  if (threadIdx.x == 0) atomicAdd(loss, s);
}

// ------------------------------------------------------------------------------------------------
// Per-class sigmoid cross-entropy (fast_rcnn.py:386-422): logits [R][LP] bf16, NC valid columns, the last of them the
// background, which takes no part; labels int64; cw fp32 [NC - 1] or NULL (= 1): the federated mask.
//   loss_sum += sum_{r, c < NC-1} cw[c] (max(x,0) - x t + log1p(exp(-|x|))),  dlogits = (sigmoid(x) - t) cw[c] gscale
// with one e = exp(-|x|) serving both: sigmoid(x) = 1 / (1 + e) for x >= 0 and e / (1 + e) below.
//
// One wave per row, rows walked with the grid's stride; no value crosses lanes except the loss (one atomic per work-group)
// and, with STATS, the row's argmax over the NC valid logits (CeCounts, as in softmax_ce_kernel).  Where LP % 8 == 0 a lane
// moves 16-byte pieces of the row, and up to LP = 1024 it keeps the weights of its two pieces in registers across rows.
// ------------------------------------------------------------------------------------------------
struct SigRow {
  float loss = 0.f;
  float mxv = -INFINITY;   // the lane's largest valid logit so far and the lowest column holding it
  int mxc = 0x7fffffff;
};

// one column: x = logit, c its column, t the row's label, w the column's weight (ignored for c >= K)
template <bool STATS>
__device__ __forceinline__ float sig_column(float x, int c, int t, int K, int NC, float w, float gscale, SigRow& row) {
  if constexpr (STATS) {
    if (c < NC && x > row.mxv) { row.mxv = x; row.mxc = c; }  // (columns arrive in rising order: the first maximum stays)
  }
  if (c >= K) return 0.f;   // background and pads: no loss, gradient exactly 0 whatever they hold
  const float tt = c == t ? 1.f : 0.f;
  const float e = __expf(-fabsf(x));
  const float inv = 1.f / (1.f + e);
  const float sg = x >= 0.f ? inv : e * inv;
  row.loss += w * (fmaxf(x, 0.f) - x * tt + log1pf(e));
  return (sg - tt) * w * gscale;
}

template <bool STATS>
__device__ __forceinline__ void sig_piece(const bf16_t* __restrict__ zr, bf16_t* __restrict__ dr, int c0, int t, int K, int NC,
                                          const float (&w)[8], float gscale, SigRow& row) {
  bf16_t raw[8], ov[8];
  *reinterpret_cast<uint4*>(raw) = *reinterpret_cast<const uint4*>(zr + c0);
#pragma unroll
  for (int e = 0; e < 8; ++e) ov[e] = f2bf(sig_column<STATS>(bf2f(raw[e]), c0 + e, t, K, NC, w[e], gscale, row));
  *reinterpret_cast<uint4*>(dr + c0) = *reinterpret_cast<const uint4*>(ov);
}

__device__ __forceinline__ void sig_weights(const float* __restrict__ cw, int c0, int K, float (&w)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) w[e] = (c0 + e < K) ? (cw ? cw[c0 + e] : 1.f) : 0.f;
}

template <bool STATS>
__global__ __launch_bounds__(256) void sigmoid_ce_kernel(const bf16_t* __restrict__ logits, const long long* __restrict__ labels,
                                                         const float* __restrict__ cw, bf16_t* __restrict__ dlogits,
                                                         float* __restrict__ loss_sum, int R, int NC, int LP, float gscale,
                                                         int* __restrict__ counters, int bg) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63;
  const int K = NC - 1;
  const int row0 = blockIdx.x * 4 + (threadIdx.x >> 6), rstep = gridDim.x * 4;
  const int chunks = LP >> 3;
  const bool vec = (LP & 7) == 0, resident = vec && chunks <= 128;
  float w[2][8];
  if (resident) {
#pragma unroll
    for (int it = 0; it < 2; ++it) sig_weights(cw, (it * 64 + lane) * 8, K, w[it]);
  }
  CeCounts cnt;
  float loss_acc = 0.f;
  for (int r = row0; r < R; r += rstep) {
    const bf16_t* zr = logits + (size_t)r * LP;
    bf16_t* dr = dlogits + (size_t)r * LP;
    const int t = (int)labels[r];
    SigRow row;
    if (resident) {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int ch = it * 64 + lane;
        if (ch < chunks) sig_piece<STATS>(zr, dr, ch * 8, t, K, NC, w[it], gscale, row);
      }
    } else if (vec) {
      for (int ch = lane; ch < chunks; ch += 64) {
        float wc[8];
        sig_weights(cw, ch * 8, K, wc);
        sig_piece<STATS>(zr, dr, ch * 8, t, K, NC, wc, gscale, row);
      }
    } else {
      for (int c = lane; c < LP; c += 64) {
        const float wc = c < K ? (cw ? cw[c] : 1.f) : 0.f;
        dr[c] = f2bf(sig_column<STATS>(bf2f(zr[c]), c, t, K, NC, wc, gscale, row));
      }
    }
    loss_acc += row.loss;
    if constexpr (STATS) {
      const float mx = wave_max(row.mxv);
      cnt.add(wave_imin(row.mxv == mx ? row.mxc : 0x7fffffff), t, bg);
    }
  }
  const float s = block_sum_256(loss_acc, red);
  if (threadIdx.x == 0 && s != 0.f) atomicAdd(loss_sum, s);
  if constexpr (STATS) cnt.send_group(counters);
}

// ------------------------------------------------------------------------------------------------
// The box heads' regression losses other than plain L1 (box_regression.py:310-369), class agnostic, one thread per row; the
// row's arithmetic is box_loss_row (box_loss_rows.h).
// ------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void box_reg_loss_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ prop,
                                                           const float* __restrict__ gtb, const long long* __restrict__ labels,
                                                           bf16_t* __restrict__ dpred, float* __restrict__ loss, int R, int LP,
                                                           int bg_label, float wx, float wy, float ww, float wh, float beta,
                                                           float scale_clamp, float gscale) {
  __shared__ float red[4];
  float l = 0.f;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < R; r += gridDim.x * 256) {
    float gd[4] = {0.f, 0.f, 0.f, 0.f};
    const long long lab = labels[r];
    if (lab >= 0 && lab < bg_label) {
      float d[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) d[q] = bf2f(pred[(size_t)r * LP + q]);
      box_loss_row<KIND>(d, prop + (size_t)r * 4, gtb + (size_t)r * 4, wx, wy, ww, wh, beta, scale_clamp, l, gd);
    }
    bf16_t* gp = dpred + (size_t)r * LP;
    const bf16_t head[8] = {f2bf(gd[0] * gscale), f2bf(gd[1] * gscale), f2bf(gd[2] * gscale), f2bf(gd[3] * gscale), 0, 0, 0, 0};
    if ((LP & 7) == 0) {   // 16-byte stores: the four gradients and four zeros, then zeros
      uint4* gv = reinterpret_cast<uint4*>(gp);
      gv[0] = *reinterpret_cast<const uint4*>(head);
      for (int c = 1; c < LP / 8; ++c) gv[c] = make_uint4(0, 0, 0, 0);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) gp[c] = head[c];
      for (int c = 4; c < LP; ++c) gp[c] = 0;
    }
  }
  const float s = block_sum_256(l, red);
  if (threadIdx.x == 0 && s != 0.f) atomicAdd(loss, s);
}

// ------------------------------------------------------------------------------------------------
// The same losses with class-specific regression (fast_rcnn.py:424-463 with cls_agnostic_bbox_reg = False): pred [R][LP] bf16
// holds 4 K valid columns and a foreground row of label c reads and differentiates columns 4c .. 4c + 3 only.  Every other
// element of dpred is written as zero here: at K = 800 a row is 6.4 KB of gradient for 8 bytes of payload, so the kernel is a
// fill with a little arithmetic in front.  A work-group takes 256 rows at a time.  First one thread per row evaluates it as
// box_reg_loss_kernel does (the same rows per thread, so the loss is summed in the same order) and leaves its four gradients
// and their column in LDS; then each wave writes every fourth row of the 256 in 16-byte pieces, the piece holding the label's
// columns patched in registers.  Wide rows are cut into gridDim.y column slices, one work-group each: every slice evaluates the
// rows (a few hundred flops against 256 rows x 1 KB of stores), slice 0 alone keeps the loss.  SMOOTH_L1 with beta == 0 is
// plain L1 (box_loss_row).
// ------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void box_reg_loss_cls_kernel(const bf16_t* __restrict__ pred, const float* __restrict__ prop,
                                                               const float* __restrict__ gtb, const long long* __restrict__ labels,
                                                               bf16_t* __restrict__ dpred, float* __restrict__ loss, int R, int LP,
                                                               int bg_label, float wx, float wy, float ww, float wh, float beta,
                                                               float scale_clamp, float gscale) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(8))) bf16_t s_head[256][4];
  __shared__ int s_col[256];   // first of the label's columns, negative for a row without gradient
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float l = 0.f;
  for (int r0 = blockIdx.x * 256; r0 < R; r0 += gridDim.x * 256) {   // (uniform over the work-group: the barriers are safe)
    const int r = r0 + threadIdx.x;
    float gd[4] = {0.f, 0.f, 0.f, 0.f};
    int c0 = -8;
    if (r < R) {
      const long long lab = labels[r];
      if (lab >= 0 && lab < bg_label) {
        c0 = 4 * (int)lab;   // c0 + 3 < 4 bg_label <= LP
        float d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = bf2f(pred[(size_t)r * LP + c0 + q]);
        box_loss_row<KIND>(d, prop + (size_t)r * 4, gtb + (size_t)r * 4, wx, wy, ww, wh, beta, scale_clamp, l, gd);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) s_head[threadIdx.x][q] = f2bf(gd[q] * gscale);
    s_col[threadIdx.x] = c0;
    __syncthreads();
    const int rows = R - r0 < 256 ? R - r0 : 256;
    for (int j = wave; j < rows; j += 4) {
      bf16_t* gp = dpred + (size_t)(r0 + j) * LP;
      const int cj = s_col[j];
      bf16_t head[4];
      *reinterpret_cast<uint2*>(head) = *reinterpret_cast<const uint2*>(s_head[j]);
      if ((LP & 7) == 0) {
        uint4* gv = reinterpret_cast<uint4*>(gp);
        const int hit = cj >> 3;                 // the piece with the label's columns (-1: none) ...
        const bool upper = (cj >> 2) & 1;        // ... and the half of it they are
        const int pieces = LP / 8, per = (pieces + gridDim.y - 1) / gridDim.y;   // this slice's pieces
        const int last = min(pieces, ((int)blockIdx.y + 1) * per);
        for (int ch = blockIdx.y * per + lane; ch < last; ch += 64) {
          bf16_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          if (ch == hit) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              v[q] = upper ? (bf16_t)0 : head[q];
              v[4 + q] = upper ? head[q] : (bf16_t)0;
            }
          }
          gv[ch] = *reinterpret_cast<const uint4*>(v);
        }
      } else {
        for (int c = lane; c < LP; c += 64) {
          const int q = c - cj;
          gp[c] = q == 0 ? head[0] : (q == 1 ? head[1] : (q == 2 ? head[2] : (q == 3 ? head[3] : (bf16_t)0)));
        }
      }
    }
    __syncthreads();   // the rows are out before the next 256 overwrite the LDS
  }
  const float s = block_sum_256(l, red);
  if (threadIdx.x == 0 && blockIdx.y == 0 && s != 0.f) atomicAdd(loss, s);
}

}  // namespace

extern "C" int u2_semseg_upsample_ce(const void* logits, const void* target, float* grad_acc, float* loss_sum,
                                     float* valid_cnt, int B, int h, int w, int LP, int NC, int ignore, void* stream) {
  if (NC > SS_MAXC || LP < NC || (LP & 7) || ignore < 0 || ignore > 255) return -1;
  if (B <= 0) return 0;
  const dim3 grid((w + SS_OW - 1) / SS_OW, (h + SS_OH - 1) / SS_OH, B);
  hipLaunchKernelGGL(semseg_ce_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                     (const uint8_t*)target, grad_acc, loss_sum, valid_cnt, B, h, w, LP, NC, ignore);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_scale_to_bf16(const float* acc, const float* num, const float* den, float mult, void* out,
                                long long n, void* stream) {
  if (n <= 0) return 0;
  size_t g = ((size_t)n + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(scale_to_bf16_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, acc, num, den, mult,
                     (bf16_t*)out, (size_t)n);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_softmax_ce(const void* logits, const void* labels, void* dlogits, float* loss_sum, int R, int NC,
                             int LP, float gscale, void* stream) {
  if (R <= 0) return 0;
  int grid = (R + 3) / 4;
  if (LP <= 1024 && (LP & 7) == 0 && grid > 512) grid = 512;  // the register-resident form loops over rows
  hipLaunchKernelGGL(softmax_ce_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                     (const long long*)labels, (bf16_t*)dlogits, loss_sum, R, NC, LP, gscale, (int*)nullptr, 0);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_softmax_ce_stats(const void* logits, const void* labels, void* dlogits, float* loss_sum, int R, int NC,
                                   int LP, float gscale, int* counters, int bg_label, void* stream) {
  if (!counters) return -1;
  if (R <= 0) return 0;  // (nothing is added: a launch without rows leaves its counter slice untouched)
  int grid = (R + 3) / 4;
  if (LP <= 1024 && (LP & 7) == 0 && grid > 512) grid = 512;
  hipLaunchKernelGGL(softmax_ce_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                     (const long long*)labels, (bf16_t*)dlogits, loss_sum, R, NC, LP, gscale, counters, bg_label);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_mask_predict_bce(const void* x, const float* Wp, const float* bp, const void* cls, const void* target,
                                   void* dx, float* dWp, float* dbp, float* loss_sum, void* logit_out, int N, int P,
                                   int C, float gscale, int phased_side, const float* gmul, void* stream) {
  if (C != 256 || (phased_side && ((phased_side & 1) || phased_side * phased_side != P))) return -1;
  if (N <= 0) return 0;
  // 8 slices: 0.184 -> 0.074 ms per launch at N = 260, P = 784; 24 slices measure 0.081 (256 more atomics per work-group)
  const int slices = P >= 512 ? 8 : (P >= 128 ? 4 : 1);
  hipLaunchKernelGGL(mask_predict_bce_kernel<false>, dim3(N, slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, Wp,
                     bp, (const long long*)cls, (const uint8_t*)target, (bf16_t*)dx, dWp, dbp, loss_sum, (bf16_t*)logit_out,
                     P, C, gscale, phased_side, gmul, (int*)nullptr);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_mask_predict_bce_stats(const void* x, const float* Wp, const float* bp, const void* cls, const void* target,
                                         float* loss_sum, int* counters, int N, int P, int C, int phased_side, void* stream) {
  if (!counters || C != 256 || (phased_side && ((phased_side & 1) || phased_side * phased_side != P))) return -1;
  if (N <= 0) return 0;
  const int slices = P >= 512 ? 8 : (P >= 128 ? 4 : 1);  // (the launch shape of u2_mask_predict_bce)
  hipLaunchKernelGGL(mask_predict_bce_kernel<true>, dim3(N, slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, Wp,
                     bp, (const long long*)cls, (const uint8_t*)target, (bf16_t*)nullptr, (float*)nullptr, (float*)nullptr,
                     loss_sum, (bf16_t*)nullptr, P, C, 0.f, phased_side, (const float*)nullptr, counters);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_count_labels_i8(const void* labels, long long n, int* counters, void* stream) {
  if (!counters) return -1;
  if (n <= 0) return 0;
  long long g = ((n >> 4) + 255) / 256;
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  hipLaunchKernelGGL(count_labels_i8_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const int8_t*)labels, n, counters);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_rpn_loss_level(const void* obj, const void* dlt, const void* labels, const int* match, const float* gt,
                                 const float* anchors, void* dobj, void* ddlt, float* loss, int B, int HW, int A, int LPo,
                                 int LPd, int Atot, int lvl_off, int G, float gscale, void* stream) {
  if (A > 4 || (LPo & 7)) return -1;
  const bool fused = dlt == nullptr;  // fused map: the deltas are columns 3 .. 14 of `obj`, the gradients one row of `dobj`
  if (fused) {
    if (ddlt || A != 3 || LPo < 16) return -1;
    dlt = (const bf16_t*)obj + A;
    LPd = LPo;
  } else if (!ddlt || LPd < 16 || (LPd & 7)) {
    return -1;
  }
  if (B <= 0 || HW <= 0) return 0;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 2048) g = 2048;
  if (fused)
    hipLaunchKernelGGL(rpn_loss_level_kernel<true>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)obj,
                       (const bf16_t*)dlt, (const int8_t*)labels, match, gt, anchors, (bf16_t*)dobj, (bf16_t*)ddlt, loss, B,
                       HW, A, LPo, LPd, Atot, lvl_off, G, gscale);
  else
    hipLaunchKernelGGL(rpn_loss_level_kernel<false>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)obj,
                       (const bf16_t*)dlt, (const int8_t*)labels, match, gt, anchors, (bf16_t*)dobj, (bf16_t*)ddlt, loss, B,
                       HW, A, LPo, LPd, Atot, lvl_off, G, gscale);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_rpn_loss_level_opt(int kind, const void* obj, const void* dlt, const void* labels, const int* match,
                                     const float* gt, const float* anchors, void* dobj, void* ddlt, float* loss, int B, int HW,
                                     int A, int LPo, int LPd, int Atot, int lvl_off, int G, float gscale, float wx, float wy,
                                     float ww, float wh, float beta, float scale_clamp, void* stream) {
  if (kind < U2_BOXLOSS_SMOOTH_L1 || kind > U2_BOXLOSS_CIOU || !(beta >= 0.f)) return -1;
  if (!(wx > 0.f && wy > 0.f && ww > 0.f && wh > 0.f)) return -1;
  if (A > 4 || (LPo & 7)) return -1;
  const bool fused = dlt == nullptr;  // the layouts of u2_rpn_loss_level
  if (fused) {
    if (ddlt || A != 3 || LPo < 16) return -1;
    dlt = (const bf16_t*)obj + A;
    LPd = LPo;
  } else if (!ddlt || LPd < 16 || (LPd & 7)) {
    return -1;
  }
  if (B <= 0 || HW <= 0) return 0;
  size_t g = ((size_t)B * HW + 255) / 256;
  if (g > 2048) g = 2048;
#define U2_RPNLOSS_LAUNCH(FUSED, KIND)                                                                                         \
  hipLaunchKernelGGL((rpn_loss_level_opt_kernel<FUSED, KIND>), dim3((int)g), dim3(256), 0, (hipStream_t)stream,               \
                     (const bf16_t*)obj, (const bf16_t*)dlt, (const int8_t*)labels, match, gt, anchors, (bf16_t*)dobj,         \
                     (bf16_t*)ddlt, loss, B, HW, A, LPo, LPd, Atot, lvl_off, G, gscale, wx, wy, ww, wh, beta, scale_clamp)
#define U2_RPNLOSS_KIND(KIND)                                                                                                  \
  if (fused) U2_RPNLOSS_LAUNCH(true, KIND); else U2_RPNLOSS_LAUNCH(false, KIND)
  switch (kind) {
    case U2_BOXLOSS_SMOOTH_L1: U2_RPNLOSS_KIND(U2_BOXLOSS_SMOOTH_L1); break;
    case U2_BOXLOSS_GIOU: U2_RPNLOSS_KIND(U2_BOXLOSS_GIOU); break;
    case U2_BOXLOSS_DIOU: U2_RPNLOSS_KIND(U2_BOXLOSS_DIOU); break;
    default: U2_RPNLOSS_KIND(U2_BOXLOSS_CIOU); break;
  }
#undef U2_RPNLOSS_KIND
#undef U2_RPNLOSS_LAUNCH
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_box_reg_l1(const void* pred, const float* prop, const float* gtb, const void* labels, void* dpred,
                             float* loss, int R, int LP, int bg_label, float wx, float wy, float ww, float wh, float gscale,
                             void* stream) {
  if (R <= 0) return 0;
  int g = (R + 255) / 256;
  if (g > 1024) g = 1024;
  hipLaunchKernelGGL(box_reg_l1_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pred, prop, gtb,
                     (const long long*)labels, (bf16_t*)dpred, loss, R, LP, bg_label, wx, wy, ww, wh, gscale);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_sigmoid_ce(const void* logits, const void* labels, const float* class_weight, void* dlogits,
                             float* loss_sum, int R, int NC, int LP, float gscale, int* counters, int bg_label, void* stream) {
  if (NC < 2 || LP < NC) return -1;
  if (R <= 0) return 0;
  int grid = (R + 3) / 4;
  if (grid > 1024) grid = 1024;  // the waves loop over rows: at most 1024 loss atomics per launch
  if (counters)
    hipLaunchKernelGGL(sigmoid_ce_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                       (const long long*)labels, class_weight, (bf16_t*)dlogits, loss_sum, R, NC, LP, gscale, counters, bg_label);
  else
    hipLaunchKernelGGL(sigmoid_ce_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)logits,
                       (const long long*)labels, class_weight, (bf16_t*)dlogits, loss_sum, R, NC, LP, gscale, (int*)nullptr, 0);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_box_reg_loss(int kind, const void* pred, const float* prop, const float* gtb, const void* labels, void* dpred,
                               float* loss, int R, int LP, int bg_label, float wx, float wy, float ww, float wh, float beta,
                               float scale_clamp, float gscale, void* stream) {
  if (kind < U2_BOXLOSS_SMOOTH_L1 || kind > U2_BOXLOSS_CIOU || LP < 4) return -1;
  if (kind == U2_BOXLOSS_SMOOTH_L1 && !(beta > 0.f)) return -1;  // beta == 0 is u2_box_reg_l1
  if (R <= 0) return 0;
  int g = (R + 255) / 256;
  if (g > 1024) g = 1024;
#define U2_BOXLOSS_LAUNCH(KIND)                                                                                              \
  hipLaunchKernelGGL(box_reg_loss_kernel<KIND>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pred, prop, gtb, \
                     (const long long*)labels, (bf16_t*)dpred, loss, R, LP, bg_label, wx, wy, ww, wh, beta, scale_clamp, gscale)
  switch (kind) {
    case U2_BOXLOSS_SMOOTH_L1: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_SMOOTH_L1); break;
    case U2_BOXLOSS_GIOU: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_GIOU); break;
    case U2_BOXLOSS_DIOU: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_DIOU); break;
    default: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_CIOU); break;
  }
#undef U2_BOXLOSS_LAUNCH
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_box_reg_loss_cls(int kind, const void* pred, const float* prop, const float* gtb, const void* labels,
                                   void* dpred, float* loss, int R, int LP, int bg_label, float wx, float wy, float ww, float wh,
                                   float beta, float scale_clamp, float gscale, void* stream) {
  if (kind < U2_BOXLOSS_SMOOTH_L1 || kind > U2_BOXLOSS_CIOU || !(beta >= 0.f)) return -1;
  if (bg_label < 1 || bg_label > (1 << 24) || LP < 4 * bg_label) return -1;   // 4 K valid columns
  if (R <= 0) return 0;
  int g = (R + 255) / 256;   // (the geometry of u2_box_reg_loss: the loss is summed in the same order)
  if (g > 1024) g = 1024;
  int slices = (LP & 7) ? 1 : (LP / 8 + 63) / 64;   // one pass of a wave's 64 lanes per slice and row where 8 slices reach
  if (slices > 8) slices = 8;
#define U2_BOXLOSS_LAUNCH(KIND)                                                                                                  \
  hipLaunchKernelGGL(box_reg_loss_cls_kernel<KIND>, dim3(g, slices), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pred, prop, gtb, \
                     (const long long*)labels, (bf16_t*)dpred, loss, R, LP, bg_label, wx, wy, ww, wh, beta, scale_clamp, gscale)
  switch (kind) {
    case U2_BOXLOSS_SMOOTH_L1: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_SMOOTH_L1); break;
    case U2_BOXLOSS_GIOU: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_GIOU); break;
    case U2_BOXLOSS_DIOU: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_DIOU); break;
    default: U2_BOXLOSS_LAUNCH(U2_BOXLOSS_CIOU); break;
  }
#undef U2_BOXLOSS_LAUNCH
  U2_CHECK_LAUNCH();
  return 0;
}
