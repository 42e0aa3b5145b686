// Argument blocks, staging and LDS-layout helpers and the launcher interface shared by the convolution sources: the entry points
// and dispatch chains (conv_api.hip), the kernel families (conv_stream.hip, conv_halo.hip, conv_tile.hip, conv_igemm.hip;
// wgrad_stream.hip, wgrad_halo.hip, conv_wgrad.hip) and the library's device scratch (conv_scratch.hip).
#pragma once
#include "common.h"
#include "conv_variant.h"

namespace u2conv {

struct ConvArgs {
  const bf16_t* in;
  const bf16_t* wt;
  bf16_t* out;
  const float* bias;
  float* stats;
  const bf16_t* zero;
  int B, Hin, Win, C, in_ld;
  int Hout, Wout, N, out_ld;
  int mul;                 // source pixel = output pixel * mul + tap offset
  int relu, accumulate;
  int M, tiles_m, tiles_n;
  // tap table: tap t reads the source at (qy*mul + tap_dy[t], qx*mul + tap_dx[t]) and uses filter tap tap_w[t]
  int ntaps, wt_taps;      // taps of this launch / taps in the weight layout ([N][wt_taps][C])
  int KW, pad_h, pad_w;    // regular launches (remap_out == 0) derive tap t = (kh, kw) arithmetically, no table reads
  short tap_dy[64], tap_dx[64], tap_w[64];
  int tap_pk[64];          // the same table as one dword per tap (scalar loads): (dy & 0xff) | (dx & 0xff) << 8 | w << 16
  // output placement: pixel (img, qy, qx) of the Hout x Wout grid is written at
  // (img, qy*out_sy + out_y0, qx*out_sx + out_x0) of the Hfull x Wfull map (identity for ordinary launches)
  int remap_out, Hfull, Wfull, out_sy, out_sx, out_y0, out_x0;
  int stagger_by_parity;   // conv_igemm256<true>: wave groups = even / odd waves instead of waves 0-3 / 4-7
  // stream-K launches of conv_tile.hip (work-groups own equal shares of the (tile, half K tile) sequence): one fp32 partial-tile
  // slot and one flag per work-group, device memory owned by the library (per stream)
  float* sk_ws;
  int* sk_flags;
  int abl;                 // measurement switches (tests/native/selftest bench2 only; 0 in production): the U2_CV_ABL field of the
                           // conv word (include/u2seg_hip.h), bit k here = bit U2_CV_ABL_SHIFT + k there.  Bit 3, `nt` stores, was
                           // the default of rounds 1-2; round 3 measured it 29-38 % SLOWER on the write-heavy 1x1 layers
};

// Tile shapes: (TM pixels x TN output channels) = 128x128 (default) or 256x64 (layers with <= 64 output channels,
// so no half of the MFMA work is spent on zero-padded channels).  4 waves, each a 64(n) x 64(m) sub-tile.

template <int BK> __device__ __forceinline__ int swz(int row);
template <> __device__ __forceinline__ int swz<64>(int row) { return row & 7; }
template <> __device__ __forceinline__ int swz<32>(int row) { return (-(row >> 2)) & 3; }

__device__ __forceinline__ void glds16(const bf16_t* src, void* lds_dst_wave_base) {
  __builtin_amdgcn_global_load_lds(U2_GLB_PTR(src), U2_LDS_PTR(lds_dst_wave_base), 16, 0, 0);
}

// XOR applied to the 16-byte chunk index of pixel row `pix` of a step image with rows of RB bytes.  A half-wave of
// ds_read_b64_tr_b16 reads 32 bytes (one chunk pair) of each of the pixels {P .. P+3, P+8 .. P+11}; the eight pieces must cover
// the 64 banks once.  RB >= 256: every row starts a bank row, eight different pairs (bits 1-3); RB = 128: two rows per bank
// row, the four rows of equal parity need four different pairs for every start P (the taps of wgrad_halo.hip shift P by 0..2):
// bits 1 and 3 of the pixel index do that; RB = 64: four rows per bank row, rows P + k and P + 8 + k need different pairs.
template <int RB> __device__ __forceinline__ int tr_swz(int pix) {
  if constexpr (RB >= 256) return ((pix & 3) << 1) | (pix & 8);
  else if constexpr (RB == 128) return (((pix >> 1) & 1) | (((pix >> 3) & 1) << 1)) << 1;
  else return ((pix >> 3) & 1) << 1;
}

// The transposing read as inline asm (through the builtin the compiler assumes that an LDS read may alias the LDS-DMA writes
// in flight and drains them), and the two reads that make one MFMA operand.
template <int IMM = 0> __device__ __forceinline__ unsigned long long tr_read(unsigned addr) {
  unsigned long long r;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(IMM) : "memory");
  return r;
}
union Frag {
  unsigned long long u[2];
  s16x8 v;
};

// Argument block of the weight-gradient families (a kernel argument of conv_wgrad.hip: fields and order are fixed).
// dW[n][tap][c] += sum_m dY[m][n] * X[src(m,tap)][c]; the entry point fills everything down to M, a launcher the rest.
struct WgradArgs {
  const bf16_t* x;    // NHWC input of the forward conv (pixel pitch x_ld)
  const bf16_t* dy;   // [M][dy_ld] output gradient
  float* dw;          // fp32, accumulated atomically at dw[n * dw_sn + tap * dw_st + c * dw_sc], n < n_valid, c < c_valid
  long long dw_sn;
  int dw_st, dw_sc, n_valid, c_valid;
  const bf16_t* zero;
  int B, Hin, Win, C, x_ld;
  int Hout, Wout, N, dy_ld;
  int KH, KW, pad_h, pad_w, stride;
  int M, tiles_n, tiles_c, pix_per_wg;
  int tiles, xcd_group;  // tiles = tiles_n * tiles_c * taps; xcd_group: 1-D launch, all tiles of a pixel split on one XCD
  // Partial tiles instead of atomics (round 4): when `part` is set a work-group stores its fp32 tile, [c][n] with n fastest, at
  // part + (split * tiles + tile) * TILE * TILE and wgrad_reduce_kernel sums the splits into dw afterwards.  fp32 atomics retire
  // at ~0.25 T operations/s on this part whatever their scope (tests/native/atomics_bench: ~1 TB/s of partial sums) - the
  // 64 KB x 512 work-group epilogue of a small-map 1x1 layer was 30 of its 77 us - plain 16-byte stores + one pass that reads
  // the partials back from the MALL move the same bytes at 5+ TB/s.
  float* part;
};

// Which kernel the most recent u2_conv_igemm / u2_conv_wgrad launch selected (u2_conv_last_kernel, a test / debugging aid):
// the U2_K_ codes of include/u2seg_hip.h.  Defined in conv_api.hip; every launcher sets the code of the kernel it launches.
extern int g_last_conv_kernel;

// The launcher convention.  Each family's launch_* decides for itself whether it serves the shape and the variant: it answers
// LAUNCH_TAKEN when it launched, LAUNCH_NOT_SERVED when the caller has to try the next family of its chain, and
// -1000 - hipError_t when its launch failed.  The two families that end a chain (launch_conv_igemm, launch_wgrad_per_tap) serve
// everything and answer with the C status of the entry point instead.  The chains themselves are in conv_api.hip.
constexpr int LAUNCH_NOT_SERVED = 0, LAUNCH_TAKEN = 1;

// conv_tile.hip: persistent 64(ch) x 128(px)-per-wave tile kernels.
int launch_conv_tile(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s);

// conv_halo.hip: 3x3 / stride 1 / pad 1 with the input halo of a 16 x 32 pixel patch staged once per 32-channel slab.
// g_last_conv_kernel code: 300.
int launch_conv_halo(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s);

// conv_stream.hip: 1x1 / stride 1 layers with <= 256 input channels - weights resident in registers, whole pixel rows streamed
// through an LDS ring.  g_last_conv_kernel code: 7xx.
int launch_conv_stream(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s);

// conv_igemm.hip: the 128 x 128 ... 256 x 256 tile kernels that serve every shape, the end of the forward chain.
int launch_conv_igemm(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s);

// conv_stream.hip, tail mode: the same launch as the data gradient of a residual block's conv1, with the backward reduce of the
// previous block's tail in the epilogue.  out = dz = mask * bf16(bf16(conv) + g2), stats[0][n] += sum dz,
// stats[1][n] += sum dz (y - mean) invstd (u2_norm_bwd_reduce with dout2, dz_out and the bit mask).
struct TailArgs {
  const bf16_t* g2 = nullptr;           // the other consumer's gradient, [M][N]
  const bf16_t* y = nullptr;            // the normalised tensor (conv3 output), [M][N]
  const unsigned char* bits = nullptr;  // ReLU bits of u2_affine_act, [M][N / 8]
  const float* mean = nullptr;
  const float* invstd = nullptr;
};
int launch_conv_stream_tail(ConvArgs& a, const TailArgs& t, int N, int C, const ConvVariant& v, hipStream_t s);

// wgrad_halo.hip: 3x3 / stride 1 / pad 1 weight gradient, all nine taps per work-group with the input halo in LDS.
// g_last_conv_kernel code: 2900.
int launch_wgrad_halo(const WgradArgs& a, const WgradVariant& v, hipStream_t s);

// wgrad_stream.hip: 1x1 / stride 1 weight gradient over large maps - a persistent work-group per pixel range accumulates a whole
// block of dW in registers, operands streamed once through an LDS ring of whole pixel rows.  g_last_conv_kernel code: 2700 +
// block configuration.
int launch_wgrad_stream(const WgradArgs& a, const WgradVariant& v, hipStream_t s);

// conv_wgrad.hip: one GEMM over the pixels per (n-tile, c-tile, filter tap), the end of the weight-gradient chain.  Fills the
// launch half of `a`.
int launch_wgrad_per_tap(WgradArgs& a, const WgradVariant& v, hipStream_t s);

// wgrad_stream.hip: the streaming weight gradient with the data gradient (and optionally a batch norm's apply step) fused in.
int launch_wdgrad_stream(const bf16_t* x, const bf16_t* dy, const bf16_t* wt, bf16_t* dx, float* dw, long long dw_sn, int dw_sc,
                         int n_valid, int c_valid, const bf16_t* zero, int M, int C, int x_ld, int N, int dy_ld, int wt_ld,
                         int dx_ld, const FusedBwdVariant& v, hipStream_t s, const bf16_t* yn = nullptr, const float* k1 = nullptr,
                         const float* k2 = nullptr, const float* k3 = nullptr);

// Library-owned device scratch (conv_scratch.hip), one block per (device, stream, kind): the kernels of a stream run one after
// the other, so consecutive launches share it.  Sized to the largest launch seen so far - allocated on first need, grown on
// demand by at least half (an outgrown block is retired, not freed: another host thread may still be about to launch on it),
// never above `limit_bytes` (nullptr: the caller takes its scratch-free path).  Nothing is freed before u2_release_scratch(),
// which drains the streams and frees the live and the retired blocks.  kind 0: stream-K hand-over slots, 1: stream-K flags (zero on
// allocation; their consumers leave them at zero), 2: weight-gradient partial tiles.
void* scratch_get(int kind, hipStream_t s, size_t need_bytes, size_t limit_bytes, bool zero_on_alloc);

}  // namespace u2conv
