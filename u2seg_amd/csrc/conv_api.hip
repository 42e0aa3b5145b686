// The public surface of the convolution family (include/u2seg_hip.h): every extern "C" conv entry point, and the two dispatch
// chains that hand a launch to the first kernel family that serves it,
//
//   forward / data gradient:  conv_stream.hip -> conv_halo.hip -> conv_tile.hip -> conv_igemm.hip
//   weight gradient:          wgrad_stream.hip -> wgrad_halo.hip -> conv_wgrad.hip
//
// An entry point validates, fills the argument block (ConvArgs / WgradArgs, conv_args.h), decodes its variant word
// (conv_variant.h) and walks its chain; what a family serves, its tile and split policy and its U2_K_ code are that family's own
// business (the launcher convention: conv_args.h).  The only kernel here is the zero fill of a strided data gradient.
#include <stdlib.h>

#include "common.h"
#include "conv_args.h"
#include "u2seg_hip.h"

using namespace u2conv;

namespace u2conv {
int g_last_conv_kernel = 0;
}
extern "C" int u2_conv_last_kernel(void) { return g_last_conv_kernel; }

namespace {

// Zero padding / row tails of every conv kernel read this page instead of branching
__device__ __attribute__((aligned(256))) bf16_t g_zero_page[128];

const bf16_t* zero_page_ptr() {
  static const bf16_t* p = nullptr;
  if (!p) {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_zero_page)) != hipSuccess) return nullptr;
    p = reinterpret_cast<const bf16_t*>(q);
  }
  return p;
}

// a caller that passes variant 0 (the product path always does) can be steered from the environment: tests and A/B runs
int env_variant(const char* name, int variant) {
  if (variant != 0) return variant;
  const char* e = getenv(name);
  return e ? (int)strtol(e, nullptr, 0) : 0;
}

// A launcher's answer (conv_args.h) at its call site: true when it settles the call, with the C status - 0, or the launcher's
// negative code - in *status; false when the family does not serve the launch.  A chain then tries its next family; an entry
// point without a fallback answers 1 = "not served, take the separate launches".
bool launch_settled(int rc, int* status) {
  if (rc == LAUNCH_NOT_SERVED) return false;
  *status = rc == LAUNCH_TAKEN ? 0 : rc;
  return true;
}

int launch_conv(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s) {
  a.abl = v.abl;  // measurement switches (conv_args.h); bit 3 = `nt` output stores, applies to every kernel below
  int status;
  // 1x1 / stride 1 layers with <= 256 input channels on large maps: weights-resident streaming kernel
  if (launch_settled(launch_conv_stream(a, N, C, v, s), &status)) return status;
  // 3x3 / stride 1 / pad 1 layers on large maps: halo-staged kernel
  if (launch_settled(launch_conv_halo(a, N, C, v, s), &status)) return status;
  // persistent tile kernels
  if (launch_settled(launch_conv_tile(a, N, C, v, s), &status)) return status;
  return launch_conv_igemm(a, N, C, v, s);
}

// The ConvArgs of a stride-1 gather that writes the whole Hout x Wout map: everything but the tiling, which the launchers set.
// The parity classes of a strided data gradient replace the tap table, the launch extent and the output placement.
// False: no zero page.
bool fill_conv_args(ConvArgs& a, const void* in, const void* wt, void* out, const float* bias, float* stats,
                    int B, int Hin, int Win, int C, int in_ld, int Hout, int Wout, int N, int out_ld, int KH, int KW, int pad_h,
                    int pad_w, int mul, int relu, int accumulate) {
  a.in = (const bf16_t*)in; a.wt = (const bf16_t*)wt; a.out = (bf16_t*)out; a.bias = bias; a.stats = stats;
  a.zero = zero_page_ptr();
  if (!a.zero) return false;
  a.abl = 0; a.stagger_by_parity = 0; a.sk_ws = nullptr; a.sk_flags = nullptr;
  a.B = B; a.Hin = Hin; a.Win = Win; a.C = C; a.in_ld = in_ld;
  a.N = N; a.out_ld = out_ld; a.mul = mul; a.relu = relu; a.accumulate = accumulate;
  a.wt_taps = KH * KW;
  a.KW = KW; a.pad_h = pad_h; a.pad_w = pad_w;
  a.Hfull = Hout; a.Wfull = Wout;
  a.Hout = Hout; a.Wout = Wout; a.M = B * Hout * Wout;
  a.ntaps = KH * KW;
  for (int kh = 0; kh < KH; ++kh)
    for (int kw = 0; kw < KW; ++kw) {
      const int t = kh * KW + kw;
      a.tap_dy[t] = (short)(kh - pad_h); a.tap_dx[t] = (short)(kw - pad_w); a.tap_w[t] = (short)t;
      a.tap_pk[t] = ((kh - pad_h) & 0xff) | (((kw - pad_w) & 0xff) << 8) | (t << 16);
    }
  a.remap_out = 0; a.out_sy = a.out_sx = 1; a.out_y0 = a.out_x0 = 0;
  return true;
}

inline int floor_div(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }

// Data gradient of a strided conv: the output pixels whose parity class (y % div, x % div) meets no filter tap (three of the four
// classes of a 1x1 / stride-2 layer) are zero.  One fill launch over all such classes (bit py * div + px of `classes`) instead of
// a GEMM-shaped launch per class that multiplies nothing (round 5).
__global__ __launch_bounds__(256) void parity_zero_fill_kernel(bf16_t* __restrict__ out, long long pixels, int H, int W, int ld, int chunks,
                                                               int div, unsigned classes) {
  const long long total = pixels * chunks;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long p = i / chunks;
    const int c = (int)(i - p * chunks);
    const int x = (int)(p % W), y = (int)((p / W) % H);
    if ((classes >> ((y % div) * div + (x % div))) & 1u)
      *reinterpret_cast<uint4*>(out + (size_t)p * ld + c * 8) = make_uint4(0u, 0u, 0u, 0u);
  }
}

// Data gradient of a stride-`div` conv: output pixels of parity class (py, px) only meet the taps with
// (py - pad + kh) % div == 0, so each class is its own small stride-1 conv (1, 2, 2 and 4 taps for 3x3 / stride 2)
// instead of 9 taps of which 3/4 would multiply the zero page.
int launch_parity_classes(ConvArgs& a, int KH, int div, const ConvVariant& v, hipStream_t s) {
  const int B = a.B, Hout = a.Hfull, Wout = a.Wfull, N = a.N, C = a.C, KW = a.KW, pad_h = a.pad_h, pad_w = a.pad_w;
  // classes without a tap: one fill launch (a class with a bias, statistics or an accumulating epilogue keeps its own launch)
  unsigned empty = 0;
  if (!a.bias && !a.stats && !a.accumulate && div * div <= 32 && (N & 7) == 0) {
    for (int py = 0; py < div; ++py)
      for (int px = 0; px < div; ++px) {
        bool any = false;
        for (int kh = 0; kh < KH && !any; ++kh)
          for (int kw = 0; kw < KW && !any; ++kw)
            any = ((((py - pad_h + kh) % div) + div) % div) == 0 && ((((px - pad_w + kw) % div) + div) % div) == 0;
        if (!any && py < Hout && px < Wout) empty |= 1u << (py * div + px);
      }
    if (empty) {
      const long long pixels = (long long)B * Hout * Wout;
      long long g = (pixels * (N / 8) + 255) / 256;
      if (g > 256 * 32) g = 256 * 32;
      hipLaunchKernelGGL(parity_zero_fill_kernel, dim3((unsigned)g), dim3(256), 0, s, a.out, pixels, Hout, Wout, a.out_ld, N / 8, div, empty);
      U2_CHECK_LAUNCH();
    }
  }
  for (int py = 0; py < div; ++py)
    for (int px = 0; px < div; ++px) {
      if ((empty >> (py * div + px)) & 1u) continue;
      const int Hq = (Hout - py + div - 1) / div, Wq = (Wout - px + div - 1) / div;
      if (Hq <= 0 || Wq <= 0) continue;
      int nt = 0;
      for (int kh = 0; kh < KH; ++kh) {
        const int vy = py - pad_h + kh;
        if (((vy % div) + div) % div) continue;
        for (int kw = 0; kw < KW; ++kw) {
          const int vx = px - pad_w + kw;
          if (((vx % div) + div) % div) continue;
          a.tap_dy[nt] = (short)floor_div(vy, div); a.tap_dx[nt] = (short)floor_div(vx, div);
          a.tap_w[nt] = (short)(kh * KW + kw);
          a.tap_pk[nt] = (a.tap_dy[nt] & 0xff) | ((a.tap_dx[nt] & 0xff) << 8) | ((kh * KW + kw) << 16);
          ++nt;
        }
      }
      a.ntaps = nt;
      a.Hout = Hq; a.Wout = Wq; a.M = B * Hq * Wq;
      a.remap_out = 1; a.out_sy = a.out_sx = div; a.out_y0 = py; a.out_x0 = px;
      const int rc = launch_conv(a, N, C, v, s);
      if (rc) return rc;
    }
  return 0;
}

// u2_conv1x1_bwd_fused and u2_conv1x1_bwd_fused_bn (yn, k1..k3: the batch norm's apply step in front, or all null)
int conv1x1_bwd_fused(const void* x, const void* dy, const void* yn, const float* k1, const float* k2, const float* k3,
                      const void* wt, void* dx, float* dw, int M, int C, int x_ld, int N, int dy_ld, int wt_ld, int dx_ld,
                      int n_valid, int c_valid, long long dw_stride_n, int dw_stride_c, int variant, void* stream) {
  if (n_valid > N || c_valid > C) return -1;
  const bf16_t* zero = zero_page_ptr();
  if (!zero) return -2;
  if (M <= 0) return 0;
  const FusedBwdVariant v = decode_fused_bwd_variant((unsigned)env_variant("U2_WDGRAD_VARIANT", variant));
  if (v.never) return 1;   // switched off (A/B runs): the caller takes the two separate launches
  int status;
  const int rc = launch_wdgrad_stream((const bf16_t*)x, (const bf16_t*)dy, (const bf16_t*)wt, (bf16_t*)dx, dw, dw_stride_n,
                                      dw_stride_c, n_valid, c_valid, zero, M, C, x_ld, N, dy_ld, wt_ld, dx_ld, v,
                                      (hipStream_t)stream, (const bf16_t*)yn, k1, k2, k3);
  return launch_settled(rc, &status) ? status : 1;
}

}  // namespace

extern "C" int u2_conv_igemm(const void* in, const void* wt, void* out, const float* bias, float* stats,
                             int B, int Hin, int Win, int C, int in_ld, int Hout, int Wout, int N, int out_ld,
                             int KH, int KW, int pad_h, int pad_w, int mul, int div, int relu, int accumulate,
                             int variant, void* stream) {
  if (C % 32 != 0 || (in_ld & 7) != 0 || KH * KW > 64 || (div > 1 && mul != 1)) return -1;
  if (B <= 0 || Hout <= 0 || Wout <= 0 || N <= 0) return 0;
  const ConvVariant v = decode_conv_variant((unsigned)env_variant("U2_CONV_VARIANT", variant));
  ConvArgs a;
  if (!fill_conv_args(a, in, wt, out, bias, stats, B, Hin, Win, C, in_ld, Hout, Wout, N, out_ld, KH, KW, pad_h, pad_w, mul, relu,
                      accumulate))
    return -2;
  if (div <= 1) return launch_conv(a, N, C, v, (hipStream_t)stream);
  return launch_parity_classes(a, KH, div, v, (hipStream_t)stream);
}

extern "C" int u2_conv_dgrad_tail(const void* in, const void* wt, const void* dout2, const void* y, const void* bits,
                                  const float* mean, const float* invstd, void* dz, float* sums, int B, int H, int W, int C,
                                  int in_ld, int N, int out_ld, int variant, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || N <= 0 || C <= 0) return 1;
  const ConvVariant v = decode_conv_variant((unsigned)env_variant("U2_CONV_VARIANT", variant));
  ConvArgs a;
  if (!fill_conv_args(a, in, wt, dz, nullptr, sums, B, H, W, C, in_ld, H, W, N, out_ld, 1, 1, 0, 0, 1, 0, 0)) return -2;
  TailArgs t;
  t.g2 = (const bf16_t*)dout2; t.y = (const bf16_t*)y; t.bits = (const unsigned char*)bits; t.mean = mean; t.invstd = invstd;
  int status;
  return launch_settled(launch_conv_stream_tail(a, t, N, C, v, (hipStream_t)stream), &status) ? status : 1;
}

extern "C" int u2_conv1x1_bwd_fused(const void* x, const void* dy, const void* wt, void* dx, float* dw, int M, int C, int x_ld,
                                    int N, int dy_ld, int wt_ld, int dx_ld, int n_valid, int c_valid, long long dw_stride_n,
                                    int dw_stride_c, int variant, void* stream) {
  return conv1x1_bwd_fused(x, dy, nullptr, nullptr, nullptr, nullptr, wt, dx, dw, M, C, x_ld, N, dy_ld, wt_ld, dx_ld, n_valid,
                           c_valid, dw_stride_n, dw_stride_c, variant, stream);
}

extern "C" int u2_conv1x1_bwd_fused_bn(const void* x, const void* dz, const void* y, const float* k1, const float* k2,
                                       const float* k3, const void* wt, void* dx, float* dw, int M, int C, int x_ld, int N, int dy_ld,
                                       int wt_ld, int dx_ld, int n_valid, int c_valid, long long dw_stride_n, int dw_stride_c,
                                       int variant, void* stream) {
  if (!y || !k1 || !k2 || !k3) return -1;
  return conv1x1_bwd_fused(x, dz, y, k1, k2, k3, wt, dx, dw, M, C, x_ld, N, dy_ld, wt_ld, dx_ld, n_valid, c_valid, dw_stride_n,
                           dw_stride_c, variant, stream);
}

extern "C" int u2_conv_wgrad(const void* x, const void* dy, float* dw, int B, int Hin, int Win, int C, int x_ld,
                             int Hout, int Wout, int N, int dy_ld, int KH, int KW, int pad_h, int pad_w,
                             int stride, int variant, void* stream) {
  return u2_conv_wgrad_into(x, dy, dw, B, Hin, Win, C, x_ld, Hout, Wout, N, dy_ld, KH, KW, pad_h, pad_w, stride, N, C,
                            (long long)KH * KW * C, C, 1, variant, stream);
}

extern "C" int u2_conv_wgrad_into(const void* x, const void* dy, float* dw, int B, int Hin, int Win, int C, int x_ld,
                                  int Hout, int Wout, int N, int dy_ld, int KH, int KW, int pad_h, int pad_w,
                                  int stride, int n_valid, int c_valid, long long dw_stride_n, int dw_stride_tap,
                                  int dw_stride_c, int variant, void* stream) {
  if ((C & 7) != 0 || (x_ld & 7) != 0 || (dy_ld & 7) != 0 || (N & 7) != 0) return -1;
  if (n_valid > N || c_valid > C) return -1;
  if (B <= 0 || Hout <= 0 || Wout <= 0) return 0;
  WgradArgs a;
  a.x = (const bf16_t*)x; a.dy = (const bf16_t*)dy; a.dw = dw; a.zero = zero_page_ptr();
  if (!a.zero) return -2;
  a.dw_sn = dw_stride_n; a.dw_st = dw_stride_tap; a.dw_sc = dw_stride_c; a.n_valid = n_valid; a.c_valid = c_valid;
  a.B = B; a.Hin = Hin; a.Win = Win; a.C = C; a.x_ld = x_ld;
  a.Hout = Hout; a.Wout = Wout; a.N = N; a.dy_ld = dy_ld;
  a.KH = KH; a.KW = KW; a.pad_h = pad_h; a.pad_w = pad_w; a.stride = stride;
  a.M = B * Hout * Wout;
  const WgradVariant v = decode_wgrad_variant((unsigned)env_variant("U2_WGRAD_VARIANT", variant));
  hipStream_t s = (hipStream_t)stream;
  int status;
  // 1x1 / stride 1 over large maps: streaming kernel with the whole dW block in registers
  if (launch_settled(launch_wgrad_stream(a, v, s), &status)) return status;
  // 3x3 / stride 1 / pad 1: all nine taps per work-group, input halo in LDS
  if (launch_settled(launch_wgrad_halo(a, v, s), &status)) return status;
  return launch_wgrad_per_tap(a, v, s);
}
