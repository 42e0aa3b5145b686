// DINO ViT forward for the stage-1 instance features (u2seg/Instance_Clustering/selective_labeling/dino.py:77-308).
//
// The four linears of every block and the patch-embed GEMM run through u2_conv_igemm (a [1, R, 1, K] view, as
// layers.functional.linear); this file holds everything around them:
//   patchify            images -> bf16 patch rows [B*P][3*p*p] in (c, kh, kw) order (patch_embed.proj, dino.py:170-173), from
//                       uint8 NHWC RGB (ToTensor + Normalize in fp32, torchvision's order) or fp32 NCHW already normalised
//   embed               prepare_tokens (dino.py:224-235): x[b][0] = cls + pos[0], x[b][1+p] = (gemm + bias) + pos[1+p], fp32
//   residual_layernorm  Block.forward's residual adds (dino.py:135-142) fused with the following LayerNorm: fp32 stream,
//                       fp32 statistics, bf16 output for the next GEMM (fp32 for the final norm)
//   attention           Attention.forward (dino.py:108-120) flash-style: the T x T scores never reach memory
//   gelu                nn.GELU() (exact erf) in place on the fc1 output (dino.py:77-93)
//
// Attention (head dim 64).  A work-group is 4 waves x 32 queries of one (image, head); K/V tiles of 64 keys are read from the
// qkv GEMM output (column s*D + h*64 + d, dino.py:110) into registers, written to LDS after the tile's first barrier and
// consumed after the second; the next tile's global loads are issued before the current tile's MFMAs (issue-early /
// write-late).  Per tile and wave:
//   S^T = K Q^T   v_mfma_f32_32x32x16_bf16 with K as the A operand (ds_read_b128 rows of the K image) and Q as the B operand
//                 (kept in registers for the whole loop): the accumulator has the query on the lane and 16 of the 32 keys in
//                 its registers (the other 16 in lane ^ 32), so the softmax row is lane-local plus one cross-half exchange.
//   softmax       online, fp32, base 2 with log2(e) * head_dim^-0.5 folded into one multiply; the rescale of O and l happens on
//                 every tile (no deferred-max threshold).
//   O^T += V^T P^T  the S^T accumulator converted pairwise to bf16 IS the B operand of the next MFMA (registers 8s .. 8s+7 are
//                 k-step s); the A operand V^T comes from the row-major V image by ds_read_b64_tr_b16, whose key order matches
//                 the accumulator's permuted row order (rows 16s + 4h + 0..3 and 16s + 8 + 4h + 0..3 for lane half h).
// Keys >= T are loaded as zeros and their scores set to -inf; queries >= q_rows are computed on a clamped row and not stored.
#include <math.h>

#include "common.h"
#include "u2seg_hip.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int AT_WAVES = 4;
constexpr int AT_QW = 32;                   // queries per wave
constexpr int AT_QB = AT_WAVES * AT_QW;     // queries per work-group
constexpr int AT_KV = 64;                   // keys per tile
constexpr int AT_LD = 72;                   // LDS row pitch in bf16 (144 B: 16-B aligned rows, K row reads spread over the banks)

// ---------------------------------------------------------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(256) void vit_patchify_kernel(const void* __restrict__ img, const float* __restrict__ norm,
                                                            bf16_t* __restrict__ out, int B, int H, int W, int p, int gh,
                                                            int gw) {
  const int K = 3 * p * p;
  const long long total = (long long)B * gh * gw * K;
  float mean[3], stdv[3];
  if (U8) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { mean[c] = norm[c]; stdv[c] = norm[3 + c]; }
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const long long rowi = i / K;
    const int px = (int)(rowi % gw);
    const long long t = rowi / gw;
    const int py = (int)(t % gh);
    const int b = (int)(t / gh);
    const int c = k / (p * p), kh = (k / p) % p, kw = k % p;
    const int y = py * p + kh, x = px * p + kw;
    float v;
    if (U8) {
      const unsigned char u = static_cast<const unsigned char*>(img)[(((long long)b * H + y) * W + x) * 3 + c];
      // ToTensor: u / 255 (fp32 division), then Normalize: (v - mean) / std
      v = ((float)u / 255.0f - mean[c]) / stdv[c];
    } else {
      v = static_cast<const float*>(img)[(((long long)b * 3 + c) * H + y) * W + x];
    }
    out[i] = f2bf(v);
  }
}

__global__ __launch_bounds__(256) void vit_embed_kernel(const bf16_t* __restrict__ g, int g_ld, const float* __restrict__ bias,
                                                        const float* __restrict__ cls, const float* __restrict__ pos,
                                                        float* __restrict__ x, int B, int T, int D) {
  const long long total = (long long)B * T * D;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const long long bt = i / D;
    const int t = (int)(bt % T);
    const int b = (int)(bt / T);
    float v;
    if (t == 0) {
      v = cls[d] + pos[d];
    } else {
      const float y = bf2f(g[((long long)b * (T - 1) + (t - 1)) * g_ld + d]) + bias[d];
      v = y + pos[(long long)t * D + d];
    }
    x[i] = v;
  }
}

// one wave per row; lane owns columns lane + 64 i
constexpr int LN_MAXI = 16;  // D <= 1024
__global__ __launch_bounds__(256) void vit_residual_ln_kernel(float* __restrict__ x, long long x_stride,
                                                              const bf16_t* __restrict__ br, long long br_stride,
                                                              const float* __restrict__ br_bias, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, void* __restrict__ out,
                                                              long long out_stride, int out_fp32, int rows, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int n = D >> 6;
  float* xr = x + (long long)row * x_stride;
  float v[LN_MAXI];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXI; ++i) {
    if (i < n) {
      const int d = lane + 64 * i;
      float a = xr[d];
      if (br != nullptr) {
        float y = bf2f(br[(long long)row * br_stride + d]);
        if (br_bias != nullptr) y = y + br_bias[d];
        a = a + y;
        xr[d] = a;
      }
      v[i] = a;
      s += a;
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXI; ++i)
    if (i < n) { const float c = v[i] - mean; q += c * c; }
  const float var = wave_sum(q) / (float)D;
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int i = 0; i < LN_MAXI; ++i) {
    if (i < n) {
      const int d = lane + 64 * i;
      const float y = (v[i] - mean) * rstd * gamma[d] + beta[d];
      if (out_fp32) static_cast<float*>(out)[(long long)row * out_stride + d] = y;
      else static_cast<bf16_t*>(out)[(long long)row * out_stride + d] = f2bf(y);
    }
  }
}

__global__ __launch_bounds__(256) void vit_gelu_kernel(bf16_t* __restrict__ x, long long n8) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    s16x8 v = reinterpret_cast<s16x8*>(x)[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bf2f((bf16_t)v[j]);
      const float y = 0.5f * a * (1.0f + erff(a * 0.70710678118654752f));
      v[j] = (short)f2bf(y);
    }
    reinterpret_cast<s16x8*>(x)[i] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vit_attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, int T, int H,
                                                            int ld, int q_rows, int nqb, float c2) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_KV * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[AT_KV * AT_LD];
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / H, h = bh - b * H;
  const int D = H * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * AT_QB + wave * AT_QW;
  const bool active = q0 < q_rows;  // wave-uniform: the transposed LDS reads below need a full EXEC mask
  const bf16_t* base = qkv + (long long)b * T * ld;

  // Q as the B operand: lane (r, hh), k-step s holds Q[q0 + r][16 s + 8 hh + 0..7]
  s16x8 qf[4];
  {
    const int qr = min(q0 + r, q_rows - 1);
    const bf16_t* qp = base + (long long)qr * ld + h * 64 + 8 * hh;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const s16x8*>(qp + 16 * s);
  }

  // staging: 64 rows x 8 chunks of 16 B per operand, two chunks of K and two of V per thread
  s16x8 kr[2], vr[2];
  auto load = [&](int t0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cidx = tid + 256 * i, row = cidx >> 3, ch = cidx & 7;
      const int key = t0 + row;
      if (key < T) {
        const bf16_t* kp = base + (long long)key * ld + D + h * 64 + ch * 8;
        kr[i] = *reinterpret_cast<const s16x8*>(kp);
        vr[i] = *reinterpret_cast<const s16x8*>(kp + D);
      } else {
        kr[i] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
        vr[i] = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };

  f32x16 o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m = -INFINITY, l = 0.f;

  // transposed-read lane roles: lane 4 qq + pp of its 16-lane group g supplies row qq, columns 4 pp .. 4 pp + 3
  const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
  const int tr_off = (4 * hh + qq) * AT_LD + 16 * (g & 1) + 4 * pp;

  load(0);
  for (int t0 = 0; t0 < T; t0 += AT_KV) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int cidx = tid + 256 * i, row = cidx >> 3, ch = cidx & 7;
      *reinterpret_cast<s16x8*>(Ks + row * AT_LD + ch * 8) = kr[i];
      *reinterpret_cast<s16x8*>(Vs + row * AT_LD + ch * 8) = vr[i];
    }
    __syncthreads();
    if (t0 + AT_KV < T) load(t0 + AT_KV);
    if (!active) continue;

    f32x16 st[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[kt][e] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const s16x8 ka = *reinterpret_cast<const s16x8*>(Ks + (32 * kt + r) * AT_LD + 16 * s + 8 * hh);
        st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], st[kt], 0, 0, 0);
      }
    }
    // st[kt][e] = score of key t0 + 32 kt + (e & 3) + 8 (e >> 2) + 4 hh for query q0 + r
    float tmax = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = t0 + 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * hh;
        const float v = key < T ? st[kt][e] * c2 : -INFINITY;
        st[kt][e] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mn = fmaxf(m, tmax);  // finite: every tile holds at least one key < T
    const float alpha = exp2f(m - mn);
    m = mn;
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = exp2f(st[kt][e] - mn);
        st[kt][e] = p;
        psum += p;
      }
    l = l * alpha + psum;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] *= alpha;

#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        s16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = (short)f2bf(st[kt][8 * s + j]);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const bf16_t* vp = Vs + (32 * kt + 16 * s) * AT_LD + 32 * db + tr_off;
          const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vp));
          const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vp + 8 * AT_LD));
          const s16x8 va = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb, o[db], 0, 0, 0);
        }
      }
  }
  if (!active) return;
  const float inv = 1.0f / (l + __shfl_xor(l, 32, 64));
  const int q = q0 + r;
  if (q >= q_rows) return;
  bf16_t* op = out + ((long long)b * q_rows + q) * D + h * 64;
  // o[db][e] = O[query q][d = 32 db + (e & 3) + 8 (e >> 2) + 4 hh]: four consecutive d per register quad
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      s16x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = (short)f2bf(o[db][4 * e4 + j] * inv);
      *reinterpret_cast<s16x4*>(op + 32 * db + 8 * e4 + 4 * hh) = w;
    }
}

inline unsigned grid_for(long long n) {
  long long g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  return (unsigned)(g < 1 ? 1 : g);
}

bool misaligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) != 0; }

}  // namespace

extern "C" int u2_vit_patchify(const void* img, const float* norm, void* out, int B, int H, int W, int C, int patch, int in_u8,
                               void* stream) {
  if (B < 1 || C != 3 || patch < 1 || H < patch || W < patch || (in_u8 && norm == nullptr)) return -1;
  const int gh = H / patch, gw = W / patch;
  const long long n = (long long)B * gh * gw * 3 * patch * patch;
  hipStream_t s = (hipStream_t)stream;
  if (in_u8)
    hipLaunchKernelGGL(vit_patchify_kernel<true>, dim3(grid_for(n)), dim3(256), 0, s, img, norm, (bf16_t*)out, B, H, W, patch,
                       gh, gw);
  else
    hipLaunchKernelGGL(vit_patchify_kernel<false>, dim3(grid_for(n)), dim3(256), 0, s, img, norm, (bf16_t*)out, B, H, W, patch,
                       gh, gw);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_vit_embed(const void* patch_out, int out_ld, const float* bias, const float* cls, const float* pos, float* x,
                            int B, int T, int D, void* stream) {
  if (B < 1 || T < 1 || D < 1 || out_ld < D) return -1;
  const long long n = (long long)B * T * D;
  hipLaunchKernelGGL(vit_embed_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)patch_out, out_ld,
                     bias, cls, pos, x, B, T, D);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_vit_residual_layernorm(float* x, long long x_stride, const void* branch, long long branch_stride,
                                         const float* branch_bias, const float* gamma, const float* beta, void* out,
                                         long long out_stride, int out_fp32, int rows, int D, float eps, void* stream) {
  if (rows < 1 || D < 64 || D % 64 != 0 || D > 64 * LN_MAXI || x_stride < D || out_stride < D ||
      (branch != nullptr && branch_stride < D))
    return -1;
  hipLaunchKernelGGL(vit_residual_ln_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, x_stride,
                     (const bf16_t*)branch, branch_stride, branch_bias, gamma, beta, out, out_stride, out_fp32, rows, D, eps);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_vit_attention(const void* qkv, void* out, int B, int T, int heads, int head_dim, int qkv_ld, int q_rows,
                                void* stream) {
  if (head_dim != 64 || B < 1 || T < 1 || heads < 1 || q_rows < 1 || q_rows > T || qkv_ld < 3 * heads * 64 || qkv_ld % 8 != 0 ||
      misaligned(qkv, 16) || misaligned(out, 8))
    return -1;
  const int nqb = (q_rows + AT_QB - 1) / AT_QB;
  const long long nwg = (long long)B * heads * nqb;
  if (nwg > 0x7fffffffLL) return -1;
  const float c2 = 1.4426950408889634f * (1.0f / sqrtf((float)head_dim));
  hipLaunchKernelGGL(vit_attention_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                     (bf16_t*)out, T, heads, qkv_ld, q_rows, nqb, c2);
  U2_CHECK_LAUNCH();
  return 0;
}

extern "C" int u2_vit_gelu(void* x, long long n, void* stream) {
  if (n < 0 || n % 8 != 0 || misaligned(x, 16)) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(vit_gelu_kernel, dim3(grid_for(n / 8)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x, n / 8);
  U2_CHECK_LAUNCH();
  return 0;
}
