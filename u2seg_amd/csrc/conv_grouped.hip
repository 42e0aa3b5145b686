// Grouped 3x3 / pad 1 / stride 1 or 2 convolution on CDNA4 MFMA: forward, data gradient and weight gradient of conv2 of a ResNeXt
// bottleneck (F.conv2d(groups = G) behind detectron2/layers/wrappers.py:127-134 for backbone/resnet.py:155-166).  DESIGN.md section 26.
//
// All three passes read the fp32 parameter in the reference's own layout w[N][cg][3][3] (cg = C / groups channels per group, N == C)
// and, optionally, a per-output-channel scale (the FrozenBN fold): W'[n][c][t] = bf16(w[n][c][t] * scale[n]), one fp32 multiply and
// one rounding, made while the slice a work-group needs is staged into LDS.  There is no bf16 kernel layout to keep up to date.
//
// Tiling.  S = max(cg, 32) channels form a super-group: cg <= 32 divides 32, so a block of 32 consecutive output channels reads
// exactly the same 32 input channels, and its 32 x 32 x 9 filter slice is block diagonal with 32 / cg blocks; cg = 64 is one dense
// 64 x 64 x 9 block.  The slice is staged DENSE (zeros off the diagonal), so one K step is one tap x 32 channels of
// __builtin_amdgcn_mfma_f32_16x16x32_bf16 whatever cg is; at cg < 32 that spends 32 / cg times the useful MACs, which is still
// 1 / (C / 32) of the dense layer's, and every layer is bound by its activation bytes (section 26 has the counts).
//
//  * forward / data gradient (gconv_kernel): a work-group owns one super-group and walks pixel patches of the map it writes
//    (8 x 32 pixels; 8 x 16 for the stride-2 forward pass).  Per patch the input halo of its S channels is staged once for all
//    nine taps (conv_halo.hip's image: 64-byte rows of 32 channels in raster order, chunk c of halo column hx stored at
//    c ^ (2 * ((hx >> 2) & 1))), every tap reads its pixel fragments from it at an offset.  The super-group index runs fastest in
//    the grid, so the work-groups that are resident together read the SAME pixels' other channels: whole cache lines are
//    consumed at about the same time although a work-group reads 64 (or 128) bytes per pixel.
//    The stride-2 data gradient splits a row of dx into its even and odd columns (16 pixels each per fragment): which taps
//    contribute is then uniform per fragment (row parity x column parity), no multiply is spent on the zeros of the dilated dz.
//    Filter rows are permuted in LDS as in conv_tile.hip, so that the MFMA D layout leaves a lane with 8 consecutive channels of
//    one pixel: one 16-byte store, four lanes a 64-byte run.
//  * weight gradient (gwgrad_kernel): the contraction runs over pixels, which are NOT contiguous in NHWC: x halo and dz patch
//    are staged in their natural layout with a row pitch of 2 S + 8 bytes and the MFMA operands (8 consecutive pixels of one
//    channel per lane) are gathered with 16-bit LDS reads (the pitch makes the four 8-pixel groups of a fragment hit disjoint
//    banks at stride 1).  A work-group keeps the 9 x S x S partial tile in registers over all the patches it walks, the waves'
//    partials meet in LDS in a fixed order, and only the block-diagonal part goes out: fp32 atomics straight into the caller's
//    [N][cg][3][3] buffer, scaled by scale[n].
//
// No stream-K, no library-owned scratch, no dependence on other streams.
#include "common.h"
#include "u2seg_hip.h"

namespace {

struct GArgs {
  const bf16_t* in;     // the map that is staged: x (forward) or dz (data gradient), [B][Hin][Win][C]
  const float* w;       // [C][cg][3][3]
  const float* scale;   // [C] or null
  const float* bias;    // [C] or null
  bf16_t* out;          // the map that is written: [B][Hout][Wout][C]
  float* stats;         // [2][C] or null
  int B, Hin, Win, Hout, Wout, C, cg, relu;
  int tiles_x, tiles_y, ntiles, tsplit, nsg;
};

__device__ __forceinline__ int swz2(int col) { return ((col >> 2) & 1) << 1; }

// filter row `o` (0 .. S-1: the channel this pass writes, relative to the super-group) -> (16-row fragment, row in it), the
// inverse of channel = (frag >> 1) * 32 + (row >> 2) * 8 + (frag & 1) * 4 + (row & 3)
__device__ __forceinline__ int wrow_offset(int o) {
  const int frag = (o >> 5) * 2 + ((o >> 2) & 1), row = ((o >> 3) & 3) * 4 + (o & 3);
  return frag * 1024 + row * 64;
}

// Stages W' of super-group channels nb .. nb + S - 1 as [tap][K chunk][fragment][16 rows][32 k] bf16 (1 KB per fragment).
// DG: the data gradient's operand, rows = input channels c, k = output channels n.
template <int S, bool DG>
__device__ __forceinline__ void stage_filter(unsigned char* wl, const float* __restrict__ w, const float* __restrict__ scale, int nb,
                                             int cg, int tid) {
  constexpr int KC = S / 32, NF = S / 16;
  if (cg < S) {
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int i = tid; i < 9 * KC * NF * 64; i += 256) reinterpret_cast<uint4*>(wl)[i] = z;
    __syncthreads();
  }
  const int per_row = cg * 9, total = S * per_row;
  const float* src = w + (size_t)nb * per_row;   // rows nb .. nb + S - 1 of w are one contiguous run
  for (int idx = tid; idx < total; idx += 256) {
    const int nrow = idx / per_row, rem = idx - nrow * per_row;
    const int cl = rem / 9, tap = rem - cl * 9;
    const int n = nb + nrow;
    const float v = src[idx] * (scale ? scale[n] : 1.0f);
    const int kk = (n / cg) * cg + cl - nb;      // the input channel, relative to the super-group
    const int o = DG ? kk : nrow, k = DG ? nrow : kk;
    const int kc = k >> 5, k5 = k & 31;
    const int row = ((o >> 3) & 3) * 4 + (o & 3);
    *reinterpret_cast<bf16_t*>(wl + (tap * KC + kc) * NF * 1024 + wrow_offset(o) + (((k5 >> 3) ^ swz2(row)) << 4) + (k5 & 7) * 2) =
        f2bf(v);
  }
}

// MODE 0: forward stride 1, 1: forward stride 2, 2: data gradient stride 1, 3: data gradient stride 2
template <int MODE> struct GGeom;
template <> struct GGeom<0> { static constexpr int PH = 8, PW = 32, HH = 10, HWD = 34, HPITCH = 36; };
template <> struct GGeom<1> { static constexpr int PH = 8, PW = 16, HH = 17, HWD = 33, HPITCH = 36; };
template <> struct GGeom<2> { static constexpr int PH = 8, PW = 32, HH = 10, HWD = 34, HPITCH = 36; };
template <> struct GGeom<3> { static constexpr int PH = 8, PW = 32, HH = 5, HWD = 17, HPITCH = 20; };

template <int S, int MODE>
constexpr int gconv_lds_bytes() {
  return 9 * (S / 32) * (S / 16) * 1024 + (S / 32) * GGeom<MODE>::HH * GGeom<MODE>::HPITCH * 64;
}

template <int S, int MODE>
__global__ __launch_bounds__(256) void gconv_kernel(const GArgs a) {
  using G = GGeom<MODE>;
  constexpr int KC = S / 32, NF = S / 16, NP = S / 32;       // K chunks, 16-row filter fragments, 32-channel output runs
  constexpr int WBYTES = 9 * KC * NF * 1024;
  constexpr int HSLAB = G::HH * G::HPITCH * 64;
  constexpr int NPF = G::PH * G::PW / 16 / 4;                // pixel fragments per wave
  constexpr bool DG = MODE >= 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* wl = smem;
  unsigned char* hl = smem + WBYTES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int sg = blockIdx.x % a.nsg, split = blockIdx.x / a.nsg;
  const int nb = sg * S;

  stage_filter<S, DG>(wl, a.w, a.scale, nb, a.cg, tid);

  float bia[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) bia[p][e] = a.bias ? a.bias[nb + p * 32 + fg * 8 + e] : 0.f;
  float st_s[NP][8], st_q[NP][8];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) { st_s[p][e] = 0.f; st_q[p][e] = 0.f; }

  const int tiles_per_img = a.tiles_x * a.tiles_y;
  for (int t = split; t < a.ntiles; t += a.tsplit) {
    const int img = t / tiles_per_img, tr = t - img * tiles_per_img;
    const int ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
    const int y0 = ty * G::PH, x0 = tx * G::PW;              // origin of the patch in the map that is written
    // origin of the halo in the map that is staged
    const int hy0 = MODE == 1 ? 2 * y0 - 1 : MODE == 3 ? (y0 >> 1) : y0 - 1;
    const int hx0 = MODE == 1 ? 2 * x0 - 1 : MODE == 3 ? (x0 >> 1) : x0 - 1;
    __syncthreads();   // the filter is staged / the previous patch's fragments are read
    {
      constexpr int Q = 4 * KC, ITEMS = G::HH * G::HPITCH * Q;
      for (int base = 0; base < ITEMS; base += 256 * 4) {
        uint4 v[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = base + u * 256 + tid;
          const int R = idx / Q, q = idx - R * Q;
          const int hy = R / G::HPITCH, hx = R - hy * G::HPITCH;
          const int kc = q >> 2, c = q & 3;
          const int y = hy0 + hy, x = hx0 + hx;
          dst[u] = idx < ITEMS && hx < G::HWD ? kc * HSLAB + R * 64 + ((c ^ swz2(hx)) << 4) : -1;
          v[u] = uint4{0u, 0u, 0u, 0u};
          if (dst[u] >= 0 && (unsigned)y < (unsigned)a.Hin && (unsigned)x < (unsigned)a.Win)
            v[u] = *reinterpret_cast<const uint4*>(a.in + ((size_t)(img * a.Hin + y) * a.Win + x) * a.C + nb + kc * 32 + c * 8);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (dst[u] >= 0) *reinterpret_cast<uint4*>(hl + dst[u]) = v[u];
      }
    }
    __syncthreads();

    f32x4 acc[NF][NPF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < NPF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        s16x8 af[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i)
          af[i] = *reinterpret_cast<const s16x8*>(wl + ((tap * KC + kc) * NF + i) * 1024 + fr * 64 + ((fg ^ swz2(fr)) << 4));
#pragma unroll
        for (int jj = 0; jj < NPF; ++jj) {
          // the lane's source pixel in the halo for this fragment and tap
          int hy, hx;
          bool valid = true;
          if (MODE == 0 || MODE == 2) {
            const int yl = wv * 2 + (jj >> 1), xl = (jj & 1) * 16 + fr;
            hy = MODE == 0 ? yl + kh : yl + 2 - kh;
            hx = MODE == 0 ? xl + kw : xl + 2 - kw;
          } else if (MODE == 1) {
            const int yl = wv * 2 + jj;
            hy = 2 * yl + kh;
            hx = 2 * fr + kw;
          } else {
            // dx row y0 + 2 wv + (jj >> 1) (y0 is even), columns x0 + 2 fr + (jj & 1): dz[(y + 1 - kh) / 2][(x + 1 - kw) / 2]
            const int ry = (jj >> 1) + 1 - kh, rx = (jj & 1) + 1 - kw;
            valid = !(ry & 1) && !(rx & 1);
            hy = wv + ry / 2;
            hx = fr + rx / 2;
          }
          if (valid) {
            const s16x8 pf = *reinterpret_cast<const s16x8*>(hl + kc * HSLAB + (hy * G::HPITCH + hx) * 64 + ((fg ^ swz2(hx)) << 4));
#pragma unroll
            for (int i = 0; i < NF; ++i) acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], pf, acc[i][jj], 0, 0, 0);
          }
        }
      }
    }

    // epilogue: the lane holds channels p * 32 + fg * 8 .. + 7 of one pixel per fragment
#pragma unroll
    for (int jj = 0; jj < NPF; ++jj) {
      int y, x;
      if (MODE == 0 || MODE == 2) { y = y0 + wv * 2 + (jj >> 1); x = x0 + (jj & 1) * 16 + fr; }
      else if (MODE == 1) { y = y0 + wv * 2 + jj; x = x0 + fr; }
      else { y = y0 + wv * 2 + (jj >> 1); x = x0 + 2 * fr + (jj & 1); }
      const bool ok = y < a.Hout && x < a.Wout;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        uint32_t pk[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float v0 = acc[2 * p + h][jj][0] + bia[p][4 * h], v1 = acc[2 * p + h][jj][1] + bia[p][4 * h + 1];
          float v2 = acc[2 * p + h][jj][2] + bia[p][4 * h + 2], v3 = acc[2 * p + h][jj][3] + bia[p][4 * h + 3];
          if (a.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
          pk[2 * h] = pack_bf16(v0, v1);
          pk[2 * h + 1] = pack_bf16(v2, v3);
        }
        if (ok) {
          if (a.stats) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float lo = __uint_as_float(pk[e] << 16), hi = __uint_as_float(pk[e] & 0xffff0000u);
              st_s[p][2 * e] += lo; st_q[p][2 * e] += lo * lo;
              st_s[p][2 * e + 1] += hi; st_q[p][2 * e + 1] += hi * hi;
            }
          }
          *reinterpret_cast<uint4*>(a.out + ((size_t)(img * a.Hout + y) * a.Wout + x) * a.C + nb + p * 32 + fg * 8) =
              uint4{pk[0], pk[1], pk[2], pk[3]};
        }
      }
    }
  }

  if (a.stats) {
    // the 16 pixel lanes of a channel run, then the four waves through LDS, then one atomic per channel and sum
    float* red = reinterpret_cast<float*>(smem);
    __syncthreads();
    if (tid < 2 * S) red[tid] = 0.f;
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float s = st_s[p][e], q = st_q[p][e];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
        if (fr == 0) {
          atomicAdd(red + p * 32 + fg * 8 + e, s);
          atomicAdd(red + S + p * 32 + fg * 8 + e, q);
        }
      }
    __syncthreads();
    if (tid < 2 * S) atomicAdd(a.stats + (tid < S ? nb + tid : a.C + nb + tid - S), red[tid]);
  }
}

template <int S, int MODE>
int launch_gconv(GArgs& a, hipStream_t s) {
  using G = GGeom<MODE>;
  a.tiles_x = (a.Wout + G::PW - 1) / G::PW;
  a.tiles_y = (a.Hout + G::PH - 1) / G::PH;
  const long long nt = (long long)a.B * a.tiles_x * a.tiles_y;
  if (nt >= (1 << 30)) return 1;
  a.ntiles = (int)nt;
  a.nsg = a.C / S;
  const int want = 1024 / a.nsg > 0 ? 1024 / a.nsg : 1;
  a.tsplit = a.ntiles < want ? a.ntiles : want;
  constexpr int lds = gconv_lds_bytes<S, MODE>();
  static_assert(lds <= 160 * 1024, "LDS budget");
  static PerDeviceOnce attr_set;
  if (auto once_guard = attr_set.first()) {
    (void)hipFuncSetAttribute((const void*)gconv_kernel<S, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  hipLaunchKernelGGL((gconv_kernel<S, MODE>), dim3((unsigned)(a.nsg * a.tsplit)), dim3(256), lds, s, a);
  U2_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------------------
struct GWArgs {
  const bf16_t* x;      // [B][H][W][C]
  const bf16_t* dz;     // [B][Hout][Wout][C]
  const float* scale;   // [C] or null
  float* dw;            // [C][cg][3][3], accumulated into
  int B, H, W, Hout, Wout, C, cg;
  int tiles_x, tiles_y, ntiles, tsplit, nsg;
};

template <int S, int STRIDE> struct GWGeom {
  static constexpr int TR = STRIDE == 1 ? 8 : 4;            // output rows of a patch (32 columns)
  static constexpr int HH = (TR - 1) * STRIDE + 3, HW = 31 * STRIDE + 3;
  static constexpr int PB = 2 * S + 8;                      // bytes of one pixel's row in LDS
  static constexpr int XBYTES = HH * HW * PB, ZBYTES = TR * 32 * PB;
  static constexpr int RED = S == 32 ? 32 * 32 * 9 * 4 : 0; // the waves' partial tiles meet here (S = 64: one wave per filter row block)
  static constexpr int LDS = XBYTES + ZBYTES > RED ? XBYTES + ZBYTES : RED;
};

template <int S, int STRIDE>
__global__ __launch_bounds__(256) void gwgrad_kernel(const GWArgs a) {
  using G = GWGeom<S, STRIDE>;
  constexpr int NF = S / 16;
  constexpr int NFW = S == 32 ? 2 : 1;      // filter row fragments (16 output channels) per wave
  constexpr int NG = NF / NFW;              // waves along the output channels
  constexpr int KS = 4 / NG;                // waves along the pixels
  constexpr int CH = S / 8;                 // 16-byte chunks per pixel
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* xl = smem;
  unsigned char* zl = smem + G::XBYTES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int ng = wv % NG, ks = wv / NG;
  const int sg = blockIdx.x % a.nsg, split = blockIdx.x / a.nsg;
  const int nb = sg * S;

  f32x4 acc[NFW][NF][9];
#pragma unroll
  for (int i = 0; i < NFW; ++i)
#pragma unroll
    for (int c = 0; c < NF; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[i][c][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int tiles_per_img = a.tiles_x * a.tiles_y;
  for (int t = split; t < a.ntiles; t += a.tsplit) {
    const int img = t / tiles_per_img, tr = t - img * tiles_per_img;
    const int ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
    const int y0 = ty * G::TR, x0 = tx * 32;                 // patch origin in the output map
    const int hy0 = y0 * STRIDE - 1, hx0 = x0 * STRIDE - 1;  // halo origin in x
    __syncthreads();
    // x halo and dz patch in their natural layout, zero outside the maps
    for (int idx = tid; idx < G::HH * G::HW * CH; idx += 256) {
      const int R = idx / CH, c = idx - R * CH;
      const int hy = R / G::HW, hx = R - hy * G::HW;
      const int y = hy0 + hy, x = hx0 + hx;
      uint4 v = {0u, 0u, 0u, 0u};
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W)
        v = *reinterpret_cast<const uint4*>(a.x + ((size_t)(img * a.H + y) * a.W + x) * a.C + nb + c * 8);
      uint2* d = reinterpret_cast<uint2*>(xl + R * G::PB + c * 16);
      d[0] = uint2{v.x, v.y};
      d[1] = uint2{v.z, v.w};
    }
    for (int idx = tid; idx < G::TR * 32 * CH; idx += 256) {
      const int R = idx / CH, c = idx - R * CH;
      const int y = y0 + (R >> 5), x = x0 + (R & 31);
      uint4 v = {0u, 0u, 0u, 0u};
      if (y < a.Hout && x < a.Wout)
        v = *reinterpret_cast<const uint4*>(a.dz + ((size_t)(img * a.Hout + y) * a.Wout + x) * a.C + nb + c * 8);
      uint2* d = reinterpret_cast<uint2*>(zl + R * G::PB + c * 16);
      d[0] = uint2{v.x, v.y};
      d[1] = uint2{v.z, v.w};
    }
    __syncthreads();

    for (int r = ks; r < G::TR; r += KS) {   // one K step of 32 pixels = one output row of the patch
      if (y0 + r >= a.Hout) break;           // (rows of zeros)
      s16x8 af[NFW];
#pragma unroll
      for (int i = 0; i < NFW; ++i) {
        const unsigned char* p = zl + (r * 32 + fg * 8) * G::PB + ((ng * NFW + i) * 16 + fr) * 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) af[i][j] = *reinterpret_cast<const short*>(p + j * G::PB);
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
        for (int c = 0; c < NF; ++c) {
          const unsigned char* p = xl + ((r * STRIDE + kh) * G::HW + fg * 8 * STRIDE + kw) * G::PB + (c * 16 + fr) * 2;
          s16x8 bfm;
#pragma unroll
          for (int j = 0; j < 8; ++j) bfm[j] = *reinterpret_cast<const short*>(p + j * STRIDE * G::PB);
#pragma unroll
          for (int i = 0; i < NFW; ++i) acc[i][c][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfm, acc[i][c][tap], 0, 0, 0);
        }
      }
    }
  }

  // D layout: row (output channel in the fragment) fg * 4 + e, column (input channel in the fragment) fr
  if constexpr (KS > 1) {
    float* red = reinterpret_cast<float*>(smem);   // [S rows][S columns][9]
    for (int round = 0; round < KS; ++round) {
      __syncthreads();
      if (ks == round) {
#pragma unroll
        for (int i = 0; i < NFW; ++i)
#pragma unroll
          for (int c = 0; c < NF; ++c)
#pragma unroll
            for (int tp = 0; tp < 9; ++tp)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                float* d = red + (((ng * NFW + i) * 16 + fg * 4 + e) * S + c * 16 + fr) * 9 + tp;
                *d = round == 0 ? acc[i][c][tp][e] : *d + acc[i][c][tp][e];
              }
      }
    }
    __syncthreads();
    const int per_row = a.cg * 9, total = S * per_row;
    float* dst = a.dw + (size_t)nb * per_row;
    for (int idx = tid; idx < total; idx += 256) {
      const int nrow = idx / per_row, rem = idx - nrow * per_row;
      const int cl = rem / 9, tp = rem - cl * 9;
      const int n = nb + nrow;
      const int kk = (n / a.cg) * a.cg + cl - nb;
      atomicAdd(dst + idx, (a.scale ? a.scale[n] : 1.0f) * red[(nrow * S + kk) * 9 + tp]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NFW; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int nrow = (ng * NFW + i) * 16 + fg * 4 + e, n = nb + nrow;
        const float sc = a.scale ? a.scale[n] : 1.0f;
        const int c0 = (n / a.cg) * a.cg - nb;   // first channel of n's group, relative to the super-group
#pragma unroll
        for (int c = 0; c < NF; ++c) {
          const int cl = c * 16 + fr - c0;
          if (cl >= 0 && cl < a.cg) {
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) atomicAdd(a.dw + ((size_t)n * a.cg + cl) * 9 + tp, sc * acc[i][c][tp][e]);
          }
        }
      }
  }
}

template <int S, int STRIDE>
int launch_gwgrad(GWArgs& a, hipStream_t s) {
  using G = GWGeom<S, STRIDE>;
  a.tiles_x = (a.Wout + 31) / 32;
  a.tiles_y = (a.Hout + G::TR - 1) / G::TR;
  const long long nt = (long long)a.B * a.tiles_x * a.tiles_y;
  if (nt >= (1 << 30)) return 1;
  a.ntiles = (int)nt;
  a.nsg = a.C / S;
  const int want = 1024 / a.nsg > 0 ? 1024 / a.nsg : 1;
  a.tsplit = a.ntiles < want ? a.ntiles : want;
  static_assert(G::LDS <= 160 * 1024, "LDS budget");
  static PerDeviceOnce attr_set;
  if (auto once_guard = attr_set.first()) {
    (void)hipFuncSetAttribute((const void*)gwgrad_kernel<S, STRIDE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  hipLaunchKernelGGL((gwgrad_kernel<S, STRIDE>), dim3((unsigned)(a.nsg * a.tsplit)), dim3(256), G::LDS, s, a);
  U2_CHECK_LAUNCH();
  return 0;
}

// shapes served: groups >= 2, C = groups * cg, C % 32 == 0, cg in {4, 8, 16, 32, 64}, stride 1 or 2
bool gconv_served(int B, int H, int W, int C, int groups, int stride) {
  if (B < 1 || H < 1 || W < 1 || C < 32 || (C & 31) || groups < 2 || C % groups) return false;
  const int cg = C / groups;
  if (!(cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64)) return false;
  return stride == 1 || stride == 2;
}

}  // namespace

extern "C" int u2_gconv3x3_fwd(const void* in, const float* w, const float* scale, const float* bias, void* out, float* stats, int B,
                               int H, int W, int C, int groups, int stride, int relu, void* stream) {
  if (!gconv_served(B, H, W, C, groups, stride) || !in || !w || !out) return 1;
  GArgs a{};
  a.in = (const bf16_t*)in; a.w = w; a.scale = scale; a.bias = bias; a.out = (bf16_t*)out; a.stats = stats;
  a.B = B; a.Hin = H; a.Win = W; a.Hout = (H + 2 - 3) / stride + 1; a.Wout = (W + 2 - 3) / stride + 1;
  a.C = C; a.cg = C / groups; a.relu = relu;
  hipStream_t s = (hipStream_t)stream;
  if (a.cg == 64) return stride == 1 ? launch_gconv<64, 0>(a, s) : launch_gconv<64, 1>(a, s);
  return stride == 1 ? launch_gconv<32, 0>(a, s) : launch_gconv<32, 1>(a, s);
}

extern "C" int u2_gconv3x3_dgrad(const void* dz, const float* w, const float* scale, void* dx, int B, int H, int W, int C, int groups,
                                 int stride, void* stream) {
  if (!gconv_served(B, H, W, C, groups, stride) || !dz || !w || !dx) return 1;
  GArgs a{};
  a.in = (const bf16_t*)dz; a.w = w; a.scale = scale; a.bias = nullptr; a.out = (bf16_t*)dx; a.stats = nullptr;
  a.B = B; a.Hin = (H + 2 - 3) / stride + 1; a.Win = (W + 2 - 3) / stride + 1; a.Hout = H; a.Wout = W;
  a.C = C; a.cg = C / groups; a.relu = 0;
  hipStream_t s = (hipStream_t)stream;
  if (a.cg == 64) return stride == 1 ? launch_gconv<64, 2>(a, s) : launch_gconv<64, 3>(a, s);
  return stride == 1 ? launch_gconv<32, 2>(a, s) : launch_gconv<32, 3>(a, s);
}

extern "C" int u2_gconv3x3_wgrad(const void* x, const void* dz, const float* scale, float* dw, int B, int H, int W, int C, int groups,
                                 int stride, void* stream) {
  if (!gconv_served(B, H, W, C, groups, stride) || !x || !dz || !dw) return 1;
  GWArgs a{};
  a.x = (const bf16_t*)x; a.dz = (const bf16_t*)dz; a.scale = scale; a.dw = dw;
  a.B = B; a.H = H; a.W = W; a.Hout = (H + 2 - 3) / stride + 1; a.Wout = (W + 2 - 3) / stride + 1;
  a.C = C; a.cg = C / groups;
  hipStream_t s = (hipStream_t)stream;
  if (a.cg == 64) return stride == 1 ? launch_gwgrad<64, 1>(a, s) : launch_gwgrad<64, 2>(a, s);
  return stride == 1 ? launch_gwgrad<32, 1>(a, s) : launch_gwgrad<32, 2>(a, s);
}
