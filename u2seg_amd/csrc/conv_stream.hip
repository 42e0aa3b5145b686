// Weights-resident streaming kernel for the short-reduction 1x1 convolutions (C <= 256 input channels, stride 1, no padding):
// F.conv2d behind detectron2/layers/wrappers.py:127-134 for conv1 / conv3 / shortcut of the res2-res4 bottlenecks
// (backbone/resnet.py:194-203), the FPN laterals (backbone/fpn.py:141-158) and their data gradients.
//
// Why (round-3 measurements): these launches move 2 (C + N) bytes per pixel for 2 C N flop - 51 to 205 flop/B, left of the 312
// flop/B ridge - so they are HBM-bound by construction, and the tile kernel (conv_tile.hip) ran them at 4.0 TB/s algorithmic:
// its K loop alone (no epilogue) reads at 3.7 TB/s, because a pixel's channel row arrives as 64-byte pieces, one per half K tile
// and each in its own LDS-DMA instruction (profiles/r02_dma_bench.txt: 4.8 TB/s from HBM in 64-byte pieces, 7.0 in >= 128-byte
// pieces), because the same <= 128 KB of weights are staged again for every tile, and because only 32 KB of pixels per CU are in
// flight.  Here
//   * the weights of a wave's 64-channel slice live in REGISTERS for the whole life of the persistent work-group (the MFMA A
//     operand: C / 2 registers per lane), loaded once;
//   * the whole LDS is a ring of pixel tiles [TM pixels][C channels], each pixel row one contiguous run of 64-512 bytes moved
//     by consecutive lanes of one LDS-DMA instruction (16-byte chunks XOR-swizzled on the source side so that every
//     ds_read_b128 fragment read is conflict-free for rows of 64 / 128 / 256 / 512 bytes), 64-160 KB per CU in flight;
//   * one raw barrier per pixel tile, counted vmcnt (DMA pieces only: loads retire in order; the epilogue's stores may retire
//     out of order and only make the wait conservative);
//   * wave tile 64 channels x (16..128) pixels, conv_tile.hip's register-direct epilogue (two 16-byte runs per lane, bias / ReLU,
//     BN column statistics by a transposing DPP reduction, accumulated per lane over the work-group's life and flushed once).
//
// TAIL (the data gradient of a residual block's conv1 whose input is the previous block's output): the epilogue is also the
// backward reduce of that block's tail (colreduce_kernel<1, 3, true> of norm.hip).  The lane that holds 16 channels of a pixel
// of the gradient g1 loads the other consumer's gradient g2, the conv3 output y and the pixel's ReLU bits at the same place,
// stores dz = mask * bf16(bf16(g1) + g2) and accumulates sum dz and sum dz (y - mean) invstd - g1 is never stored, and the
// reduce pass (3 reads, 1 write of the block output's size) does not run.
#include <stdlib.h>

#include "common.h"
#include "conv_args.h"

namespace u2conv {
namespace {

// XOR applied to the 16-byte chunk index of LDS row `row` (rows of RB bytes): conflict-free ds_read_b128 fragment reads
// (16 rows x 4 chunks per instruction) - checked by brute force over the four lane groups of MI355X_MICROARCH.md's LDS table
template <int RB> __device__ __forceinline__ int row_swz(int row) {
  if constexpr (RB == 64) return swz<32>(row);  // 32 channels = 64 bytes: the tile kernels' layout
  else if constexpr (RB == 128) return (row >> 1) & 7;  // not swz<64> (row & 7): another layout for the same row length
  else return row & 15;
}

// NF fragment reads at immediate offsets J * 16 * RB from one address, as inline asm: the compiler's wait-count pass answers
// compiler-visible LDS reads beside an LDS-DMA ring with lgkmcnt(0) even where a counted wait would do (LDS returns in order),
// which exposes the round trip a register double buffer is there to hide
template <int NF, int RB, int J = 0> __device__ __forceinline__ void lds_read_frags(s16x8 (&pf)[NF], unsigned addr) {
  if constexpr (J < NF) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(pf[J]) : "v"(addr), "n"(J * 16 * RB) : "memory");
    lds_read_frags<NF, RB, J + 1>(pf, addr);
  }
}
// waits until at most CNT LDS operations are outstanding; the empty statements tie the released registers to the wait, so no
// MFMA that reads them can be scheduled in front of it
template <int CNT, int NF> __device__ __forceinline__ void lds_wait_frags(s16x8 (&pf)[NF]) {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(CNT) : "memory");
#pragma unroll
  for (int j = 0; j < NF; ++j) asm volatile("" : "+v"(pf[j])::"memory");
}

// KS: 32-channel slabs of the reduction (C = 32 KS); TM: pixels per tile; PSW: waves along the pixels (NWV / PSW along the
// channels, 64 each); NWV: waves per work-group (4: two groups per CU, 8: one); KSS: slabs per ring step - a tile arrives in
// KS / KSS steps of TM x (64 KSS)-byte rows (KSS < KS keeps five steps of a 256-channel tile in flight in an 80 KB ring where
// whole tiles would leave room for two: the read-heavy reducing layers 256 -> 64 / 128)
// value of lane E of the caller's DPP row (16 lanes), in every lane of the row
template <int E> __device__ __forceinline__ float row_bcast(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + E, 0xf, 0xf, true));
}

// lanes 2 e and 2 e + 1 (e a constant after unrolling)
__device__ __forceinline__ f32x2_t row_bcast_pair(float v, int e) {
  switch (e) {
    case 0: return f32x2_t{row_bcast<0>(v), row_bcast<1>(v)};
    case 1: return f32x2_t{row_bcast<2>(v), row_bcast<3>(v)};
    case 2: return f32x2_t{row_bcast<4>(v), row_bcast<5>(v)};
    case 3: return f32x2_t{row_bcast<6>(v), row_bcast<7>(v)};
    case 4: return f32x2_t{row_bcast<8>(v), row_bcast<9>(v)};
    case 5: return f32x2_t{row_bcast<10>(v), row_bcast<11>(v)};
    case 6: return f32x2_t{row_bcast<12>(v), row_bcast<13>(v)};
    default: return f32x2_t{row_bcast<14>(v), row_bcast<15>(v)};
  }
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
// what the TAIL epilogue reads beside one output row of a lane: g2 and y under its two 8-channel runs, the row's 64 ReLU bits
struct TailRow {
  u32x4_t ga, gb, ya, yb;
  u32x2_t mk;
};

template <int KS, int TM, int PSW, int NWV, int KSS = KS, bool TAIL = false>
__global__ __launch_bounds__(NWV * 64, 2) void conv_stream_kernel(const ConvArgs a, int ring, const TailArgs t) {
  constexpr int RB = KSS * 64, CPR = KSS * 4, STAGE = TM * RB;
  constexpr int RPP = 16 / KSS;             // pixel rows per 1 KB LDS-DMA piece
  constexpr int PT = TM * KSS / 16;         // pieces per step
  constexpr int PPW = PT / NWV;             // pieces per wave and step
  constexpr int S = KS / KSS;               // steps per tile
  constexpr int CBW = NWV / PSW, WPX = TM / PSW, NF = WPX / 16;
  static_assert(PT % NWV == 0 && PPW >= 1 && PPW <= 8 && NF >= 1 && (KSS == 1 || KSS == 2 || KSS == 4 || KSS == 8) && KS % KSS == 0 && (S & (S - 1)) == 0, "unsupported configuration");
  static_assert(!TAIL || (S == 1 && NF % 2 == 0), "the tail epilogue takes whole tiles per step and batches of 1, 2 or 4 rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cbw = w % CBW, psw = w / CBW;
  const int fr = lane & 15, fg = lane >> 4;

  // ---- tiles of this work-group: XCD x owns a contiguous range of pixel tiles; inside the XCD the work-groups are
  // (walker, 256-channel block) pairs, the walkers of one channel block take the range's tiles round robin
  const int TP = a.tiles_m, tiles_n = a.tiles_n;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, gx = gridDim.x >> 3;
  const int q8 = TP >> 3, r8 = TP & 7;
  const int xbase = (xcd < r8) ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  const int xcnt = q8 + (xcd < r8 ? 1 : 0);
  const int nwalk = gx / tiles_n;
  const int nt = idx % tiles_n, walker = idx / tiles_n;
  if (walker >= nwalk || walker >= xcnt) return;
  const int my_tiles = (xcnt - walker + nwalk - 1) / nwalk;
  const int first_tile = xbase + walker;
  const int n0 = nt * (CBW * 64) + cbw * 64;   // first channel of this wave's slice

  // ---- resident weights: block i (16 rows of the MFMA A operand), slab ks.  Row rho = i * 16 + fr of the slice holds channel
  // (i >> 1) * 32 + (fr >> 2) * 8 + (i & 1) * 4 + (fr & 3) (conv_tile.hip: the D layout then leaves a lane with two runs of 8
  // consecutive channels); lane (fr, fg) holds reduction channels ks * 32 + fg * 8 .. + 7 of that row
  s16x8 wr[KS][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + (i >> 1) * 32 + (fr >> 2) * 8 + (i & 1) * 4 + (fr & 3);
    const bf16_t* src = a.wt + (size_t)(n < a.N ? n : 0) * a.C + fg * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      s16x8 v = *reinterpret_cast<const s16x8*>(src + ks * 32);
      if (n >= a.N) v = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
      wr[ks][i] = v;
    }
  }
  // TAIL: mean / invstd of ONE channel per lane, the channel whose sums the lane ends up with (st_n below); the epilogue fetches
  // the 16 channels of a row by DPP broadcast (32 registers otherwise)
  float t_mu = 0.f, t_is = 0.f;
  if constexpr (TAIL) {
    const int tn = n0 + fg * 8 + (fr >> 3) * 32 + (fr & 7);
    t_mu = t.mean[tn];
    t_is = t.invstd[tn];
  }
  // the loads above must have landed before the first LDS-DMA is issued: a later compiler-generated wait for them would
  // otherwise have to drain the ring
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (TAIL) asm volatile("" : "+v"(t_mu), "+v"(t_is));
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(wr[ks][i]));

  // ---- LDS-DMA staging: piece q of this wave = piece q * NWV + w of the tile = RPP consecutive pixel rows; lane i moves
  // chunk position (i % CPR) of row (i / CPR), which holds source chunk position ^ swizzle(row)
  unsigned d_off[PPW];   // byte offset of the lane's source chunk inside a tile (first row of the tile = 0)
  int d_row[PPW];
#pragma unroll
  for (int q = 0; q < PPW; ++q) {
    const int row = (q * NWV + w) * RPP + lane / CPR;
    const int pos = lane % CPR;
    const int chunk = (pos & ~15) | ((pos ^ row_swz<RB>(row)) & (CPR < 16 ? CPR - 1 : 15));
    d_row[q] = row;
    d_off[q] = (unsigned)(((size_t)row * a.in_ld + chunk * 8) * 2);
  }
  const unsigned char* in_bytes = reinterpret_cast<const unsigned char*>(a.in);
  auto issue = [&](int g, int slot) {   // step g of this work-group = step g % S of its tile g / S
    const int ti = g / S, st = g % S;
    const int m0 = (first_tile + ti * nwalk) * TM;
    const unsigned char* tbase = in_bytes + (size_t)m0 * a.in_ld * 2 + st * RB;
#pragma unroll
    for (int q = 0; q < PPW; ++q) {
      const unsigned char* src = (m0 + d_row[q] < a.M) ? tbase + d_off[q] : reinterpret_cast<const unsigned char*>(a.zero);
      glds16(reinterpret_cast<const bf16_t*>(src), smem + slot * STAGE + (q * NWV + w) * 1024);
    }
  };

  // ---- fragment address of pixel fragment 0, slab 0 in slot 0; fragment j adds j * 16 * RB, slab ks XORs (ks * 4) into the
  // chunk index (the swizzle only touches the low four chunk bits and ks * 4 + fg < CPR)
  const unsigned lds0 = (unsigned)(size_t)U2_LDS_PTR(smem);
  const int pfrag0 = (psw * WPX + fr) * RB;
  const int pchunk0 = fg ^ row_swz<RB>(fr);

  f32x4 acc[4][NF];
  // BN column statistics of one channel per lane, over all tiles of the work-group
  float st_s = 0.f, st_ss = 0.f;
  const int st_n = n0 + fg * 8 + (fr >> 3) * 32 + (fr & 7);

  const int nslice = n0;
  const int nb = nslice + fg * 8;
  const bool okA = nb < a.N, okB = nb + 32 < a.N;
  f32x4 bia[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (a.bias) {
    if (okA)
      asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16\n\ts_waitcnt vmcnt(0)"
                   : "=&v"(bia[0]), "=&v"(bia[1]) : "v"(a.bias + nb) : "memory");
    if (okB)
      asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:16\n\ts_waitcnt vmcnt(0)"
                   : "=&v"(bia[2]), "=&v"(bia[3]) : "v"(a.bias + nb + 32) : "memory");
  }
  const bool do_stats = TAIL || (a.stats && !(a.abl & 2));

  // every memory operation of the epilogue is inline asm (conv_tile.hip: a compiler-visible global access inside the tile loop
  // makes the wait-count pass drain the LDS-DMA queue in front of the next fragment read)
  auto epilogue = [&](int ti) {
    const int m0 = (first_tile + ti * nwalk) * TM + psw * WPX;
    f32x2_t s2[8], ss2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s2[e] = f32x2_t{0.f, 0.f}; ss2[e] = f32x2_t{0.f, 0.f}; }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int m = m0 + j * 16 + fr;
      const bool row_ok = m < a.M;
      uint32_t pk[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v0 = acc[i][j][0] + bia[i][0], v1 = acc[i][j][1] + bia[i][1];
        float v2 = acc[i][j][2] + bia[i][2], v3 = acc[i][j][3] + bia[i][3];
        if (a.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
        pk[2 * i] = pack_bf16(v0, v1);
        pk[2 * i + 1] = pack_bf16(v2, v3);
      }
      if (do_stats && row_ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const f32x2_t v = {__uint_as_float(pk[e] << 16), __uint_as_float(pk[e] & 0xffff0000u)};
          s2[e] += v;
          ss2[e] = __builtin_elementwise_fma(v, v, ss2[e]);
        }
      }
      if (row_ok && !(a.abl & 1)) {
        bf16_t* dst = a.out + (size_t)m * a.out_ld + nb;
        const u32x4_t va = {pk[0], pk[1], pk[2], pk[3]}, vb = {pk[4], pk[5], pk[6], pk[7]};
        if (okA) asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(dst), "v"(va) : "memory");
        if (okB) asm volatile("global_store_dwordx4 %0, %1, off offset:64\n\ts_nop 1" ::"v"(dst), "v"(vb) : "memory");
      }
    }
    if (do_stats) {
      float s[16], ss[16];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[2 * e] = s2[e][0]; s[2 * e + 1] = s2[e][1]; ss[2 * e] = ss2[e][0]; ss[2 * e + 1] = ss2[e][1]; }
      st_s += row16_transpose_sum(s, fr);
      st_ss += row16_transpose_sum(ss, fr);
    }
  };

  // ---- TAIL epilogue.  The companions arrive in batches of TR rows (18 registers a row).  Loads return in order, so a wait for a batch also
  // waits for every LDS-DMA piece issued before it: batch 0 is requested right after the barrier, IN FRONT of the ring step
  // issued there, and its wait leaves that step in flight; the later batches wait for everything (the step is then older than
  // the MFMA phase plus a memory round trip).  The addresses of rows beyond M are clamped, so every load is issued and the
  // counts are exact; such rows get an all-zero mask, which makes their dz and both their terms zero.
  constexpr bool EARLY = NF <= 4;   // (NF = 8: the fragments and 128 accumulators leave no room beside the MFMA phase)
  constexpr int TR = NF >= 8 ? 4 : NF >= 4 ? 2 : 1;   // rows per batch (18 registers each)
  TailRow tr[TR];
  auto tail_issue = [&](int ti, int b) {
    const int m0 = (first_tile + ti * nwalk) * TM + psw * WPX;
#pragma unroll
    for (int r = 0; r < TR; ++r) {
      int m = m0 + (TR * b + r) * 16 + fr;
      m = m < a.M ? m : a.M - 1;
      // 32-bit byte offsets beside the scalar base pointers (the launcher checks M * N * 2 < 2^32): one address register for
      // g2, y and dz
      const unsigned off = ((unsigned)m * (unsigned)a.out_ld + (unsigned)nb) * 2u;
      const unsigned moff = (unsigned)m * (unsigned)(a.N >> 3) + (unsigned)(n0 >> 3);
      asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:64"
                   : "=&v"(tr[r].ga), "=&v"(tr[r].gb) : "v"(off), "s"(t.g2) : "memory");
      asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:64"
                   : "=&v"(tr[r].ya), "=&v"(tr[r].yb) : "v"(off), "s"(t.y) : "memory");
      asm volatile("global_load_dwordx2 %0, %1, %2" : "=&v"(tr[r].mk) : "v"(moff), "s"(t.bits) : "memory");
    }
  };
  auto tail_epilogue = [&](int ti, bool step_issued) {
    const int m0 = (first_tile + ti * nwalk) * TM + psw * WPX;
    f32x2_t s2[8], ss2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s2[e] = f32x2_t{0.f, 0.f}; ss2[e] = f32x2_t{0.f, 0.f}; }
    // g1 as the plain epilogue would have stored it, for the whole tile at once: half the accumulators' registers
    uint32_t g1p[NF][8];
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        g1p[j][2 * i] = pack_bf16(acc[i][j][0], acc[i][j][1]);
        g1p[j][2 * i + 1] = pack_bf16(acc[i][j][2], acc[i][j][3]);
      }
    // (tied down here: left to the scheduler the conversions sink to their uses and the accumulators stay live)
#pragma unroll
    for (int j = 0; j < NF; ++j)
      asm volatile("" : "+v"(g1p[j][0]), "+v"(g1p[j][1]), "+v"(g1p[j][2]), "+v"(g1p[j][3]), "+v"(g1p[j][4]), "+v"(g1p[j][5]),
                        "+v"(g1p[j][6]), "+v"(g1p[j][7]));
#pragma unroll
    for (int b = 0; b < NF / TR; ++b) {
      if (b > 0 || !EARLY) tail_issue(ti, b);
      // (every path ends in an unconditional wait: tools/check_inflight_moves.py follows the control flow, not the flag)
      if (EARLY && b == 0 && !step_issued) wait_vm<0>();
      if (EARLY && b == 0) wait_vm<PPW>();
      else wait_vm<0>();
#pragma unroll
      for (int r = 0; r < TR; ++r)
        asm volatile("" : "+v"(tr[r].ga), "+v"(tr[r].gb), "+v"(tr[r].ya), "+v"(tr[r].yb), "+v"(tr[r].mk)::"memory");
#pragma unroll
      for (int r = 0; r < TR; ++r) {
        const int j = TR * b + r;
        const int m = m0 + j * 16 + fr;
        const bool row_ok = m < a.M;
        // byte fg of the row's first / second 32 channels: the bits of this lane's two runs
        const uint32_t bitsA = row_ok ? (tr[r].mk[0] >> (fg * 8)) & 0xffu : 0u;
        const uint32_t bitsB = row_ok ? (tr[r].mk[1] >> (fg * 8)) & 0xffu : 0u;
        uint32_t pk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t gw = e < 4 ? tr[r].ga[e & 3] : tr[r].gb[e & 3];
          const uint32_t yw = e < 4 ? tr[r].ya[e & 3] : tr[r].yb[e & 3];
          const uint32_t bt = ((e < 4 ? bitsA : bitsB) >> (2 * (e & 3))) & 3u;
          const f32x2_t g1 = {__uint_as_float(g1p[j][e] << 16), __uint_as_float(g1p[j][e] & 0xffff0000u)};
          const f32x2_t g2 = {__uint_as_float(gw << 16), __uint_as_float(gw & 0xffff0000u)};
          const f32x2_t sum = g1 + g2;
          // colreduce_kernel<1, 3, true>: dz = bf16(g1 + g2) where the bit is set, else +0
          pk[e] = pack_bf16(sum[0], sum[1]) & (((bt & 1u) ? 0xffffu : 0u) | ((bt & 2u) ? 0xffff0000u : 0u));
          const f32x2_t dz = {__uint_as_float(pk[e] << 16), __uint_as_float(pk[e] & 0xffff0000u)};
          const f32x2_t yv = {__uint_as_float(yw << 16), __uint_as_float(yw & 0xffff0000u)};
          const f32x2_t mu = row_bcast_pair(t_mu, e), is = row_bcast_pair(t_is, e);
          s2[e] += dz;
          ss2[e] += dz * (yv - mu) * is;   // the reduce's expression and order; contraction is off
          // one channel pair after the other: the broadcasts of the next pair wait for this pair's sums (formed for a whole row,
          // or kept across rows, they and the unpacked operands are some hundred registers and the weights get spilled)
          asm volatile("" : "+v"(s2[e]), "+v"(ss2[e]), "+v"(t_mu), "+v"(t_is));
        }
        if (row_ok) {
          const unsigned off = ((unsigned)m * (unsigned)a.out_ld + (unsigned)nb) * 2u;
          const u32x4_t va = {pk[0], pk[1], pk[2], pk[3]}, vb = {pk[4], pk[5], pk[6], pk[7]};
          asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(off), "v"(va), "s"(a.out) : "memory");
          asm volatile("global_store_dwordx4 %0, %1, %2 offset:64\n\ts_nop 1" ::"v"(off), "v"(vb), "s"(a.out) : "memory");
        }
      }
    }
    float s[16], ss[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[2 * e] = s2[e][0]; s[2 * e + 1] = s2[e][1]; ss[2 * e] = ss2[e][0]; ss[2 * e + 1] = ss2[e][1]; }
    st_s += row16_transpose_sum(s, fr);
    st_ss += row16_transpose_sum(ss, fr);
  };

  // ---- pipeline: ring - 1 steps in flight; step g waits for its own pieces (counted: the pieces of the up to ring - 2 younger
  // steps stay in flight), the barrier publishes the step and frees the slot of step g - 1 for step g + ring - 1
  const int G = my_tiles * S;
  for (int sl = 0; sl < ring - 1 && sl < G; ++sl) issue(sl, sl);
  int slot = 0, g = 0;
  for (int ti = 0; ti < my_tiles; ++ti) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
   for (int st = 0; st < S; ++st, ++g) {
    {
      int nd = G - 1 - g;
      if (nd > ring - 2) nd = ring - 2;
      switch (nd) {
        case 0: wait_vm<0>(); break;
        case 1: wait_vm<PPW>(); break;
        case 2: wait_vm<2 * PPW>(); break;
        case 3: wait_vm<3 * PPW>(); break;
        case 4: wait_vm<4 * PPW>(); break;
        case 5: wait_vm<5 * PPW>(); break;
        default: wait_vm<6 * PPW>(); break;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (TAIL && EARLY) tail_issue(ti, 0);
    const bool step_issued = g + ring - 1 < G;
    if (step_issued) {
      int s2 = slot - 1;
      if (s2 < 0) s2 += ring;
      issue(g + ring - 1, s2);
    }
    const unsigned char* sb = smem + slot * STAGE + pfrag0;
    // the fragments of slab ks + 1 are requested in front of the MFMAs of slab ks (two register sets) where a slab is short:
    // with <= 4 pixel fragments a slab is <= 16 MFMAs per wave and an exposed LDS round trip per slab was most of the step
    constexpr bool DB = NF <= 4 && KSS > 1;
    s16x8 pf[DB ? 2 : 1][NF];
    if constexpr (DB) {
      const unsigned sba = lds0 + (unsigned)(slot * STAGE + pfrag0);
      lds_read_frags<NF, RB>(pf[0], sba + (unsigned)(pchunk0 << 4));
#pragma unroll
      for (int ks = 0; ks < KSS; ++ks) {
        const int cur = ks & 1;
        if (ks + 1 < KSS) {
          lds_read_frags<NF, RB>(pf[cur ^ 1], sba + (unsigned)((((ks + 1) * 4) ^ pchunk0) << 4));
          lds_wait_frags<NF, NF>(pf[cur]);
        } else {
          lds_wait_frags<0, NF>(pf[cur]);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[st * KSS + ks][i], pf[cur][j], acc[i][j], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < KSS; ++ks) {
#pragma unroll
        for (int j = 0; j < NF; ++j)
          pf[0][j] = *reinterpret_cast<const s16x8*>(sb + j * 16 * RB + (((ks * 4) ^ pchunk0) << 4));
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[st * KSS + ks][i], pf[0][j], acc[i][j], 0, 0, 0);
      }
    }
    slot = slot + 1 == ring ? 0 : slot + 1;
   }
    if constexpr (TAIL) tail_epilogue(ti, g + ring - 2 < G);   // (g was advanced past the tile's only step)
    else if (!(a.abl & 4)) epilogue(ti);
  }
  if (do_stats) wg_flush_column_sums<NWV>(a.stats, a.N, st_n, st_s, st_ss, w, lane, smem);
}

template <int KS, int TM, int PSW, int NWV, int KSS = KS, bool TAIL = false>
int launch_stream_cfg(ConvArgs& a, int N, int tiny, int forced, int code, hipStream_t s, const TailArgs& t = TailArgs{}) {
  constexpr int CBW = NWV / PSW;
  constexpr int STAGE = TM * KSS * 64;
  const int per_cu = NWV == 4 ? 2 : 1;
  const int lds_budget = (per_cu == 2 ? 80 : 160) * 1024;
  int ring = lds_budget / STAGE;
  if (ring > 8) ring = 8;
  if (ring < 2) return LAUNCH_NOT_SERVED;
  a.tiles_m = (a.M + TM - 1) / TM;
  a.tiles_n = (N + CBW * 64 - 1) / (CBW * 64);
  long long G = tiny ? 8LL * a.tiles_n : 256LL * per_cu;
  if ((G >> 3) < a.tiles_n) return LAUNCH_NOT_SERVED;   // (work-groups of an XCD beyond walkers x channel blocks stay idle)
  // at least ~6 pixel tiles per work-group: shorter-lived launches (stride-32 maps, ROI heads) stay on the tile kernels, whose
  // finer (tile, K) grain fills the chip better there
  if (!forced && !tiny && (long long)a.tiles_m * a.tiles_n < 6 * G) return LAUNCH_NOT_SERVED;
  static PerDeviceOnce attr_set;
  if (auto once_guard = attr_set.first()) {
    (void)hipFuncSetAttribute((const void*)conv_stream_kernel<KS, TM, PSW, NWV, KSS, TAIL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  }
  g_last_conv_kernel = code;
  hipLaunchKernelGGL((conv_stream_kernel<KS, TM, PSW, NWV, KSS, TAIL>), dim3((unsigned)G), dim3(NWV * 64), (size_t)ring * STAGE, s, a, ring, t);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return -1000 - (int)e;
  return LAUNCH_TAKEN;
}

}  // namespace

// What the conv word says to both streaming launchers: false = forbidden, or an explicit kernel selection keeps the launch on
// the older kernels.
static bool stream_allowed(const ConvVariant& v, bool& forced, int& tiny) {
  forced = v.stream == Choice::Force;
  tiny = v.tiny;
  return v.stream != Choice::Never && !v.explicit_kernel;
}

// Serves 1x1 / stride 1 / unpadded launches with C in {32, 64, 128, 256}, N % 8 == 0, not accumulating.
// g_last_conv_kernel code: 700 + C / 32 * 10 + (1, 2, 4 waves along the pixels -> 0, 1, 2).
int launch_conv_stream(ConvArgs& a, int N, int C, const ConvVariant& v, hipStream_t s) {
  bool forced;
  int tiny;
  if (!stream_allowed(v, forced, tiny)) return LAUNCH_NOT_SERVED;
  if (a.remap_out || a.accumulate || a.ntaps != 1 || a.wt_taps != 1 || a.pad_h != 0 || a.pad_w != 0 || a.mul != 1 ||
      a.Hin != a.Hout || a.Win != a.Wout)
    return LAUNCH_NOT_SERVED;
  if (!(C == 32 || C == 64 || C == 128 || C == 256) || (N & 7) || (a.out_ld & 7) || a.in_ld < C || a.M < 1) return LAUNCH_NOT_SERVED;
  if ((unsigned long long)a.M * a.in_ld * 2ull >= 0xffffffffull) return LAUNCH_NOT_SERVED;
  const int code = U2_K_STREAM + (C / 32) * 10;
  if (C == 64) {
    if (N > 128) return launch_stream_cfg<2, 128, 1, 4>(a, N, tiny, forced, code, s);
    if (N > 64) return launch_stream_cfg<2, 128, 2, 4>(a, N, tiny, forced, code + 1, s);
    return launch_stream_cfg<2, 128, 4, 4>(a, N, tiny, forced, code + 2, s);
  }
  if (C == 256) {
    if (N > 128) return launch_stream_cfg<8, 64, 2, 8>(a, N, tiny, forced, code, s);
    if (N > 64) return launch_stream_cfg<8, 64, 2, 4, 4>(a, N, tiny, forced, code + 1, s);
    return launch_stream_cfg<8, 64, 4, 4, 4>(a, N, tiny, forced, code + 2, s);
  }
  if (C == 128) {
    if (N > 128) return launch_stream_cfg<4, 64, 1, 4>(a, N, tiny, forced, code, s);
    if (N > 64) return launch_stream_cfg<4, 64, 2, 4>(a, N, tiny, forced, code + 1, s);
    return launch_stream_cfg<4, 64, 4, 4>(a, N, tiny, forced, code + 2, s);
  }
  if (N > 128) return launch_stream_cfg<1, 128, 1, 4>(a, N, tiny, forced, code, s);
  if (N > 64) return launch_stream_cfg<1, 128, 2, 4>(a, N, tiny, forced, code + 1, s);
  return launch_stream_cfg<1, 128, 4, 4>(a, N, tiny, forced, code + 2, s);
}


// The data gradient of a residual block's conv1 with the previous block's tail reduce in its epilogue (TAIL above): a.out is
// dz, a.stats the [2][N] sums.  Serves the three launches the res2-res4 bottlenecks make - (C, N) = (64, 256), (128, 512),
// (256, 1024), dense rows - under launch_conv_stream's variant rules and fill rule; everything else is "not served" (0) and
// nothing is written.  g_last_conv_kernel code: 705 + C / 32 * 10.
int launch_conv_stream_tail(ConvArgs& a, const TailArgs& t, int N, int C, const ConvVariant& v, hipStream_t s) {
  bool forced;
  int tiny;
  if (!stream_allowed(v, forced, tiny)) return LAUNCH_NOT_SERVED;
  if (a.remap_out || a.accumulate || a.relu || a.bias || a.ntaps != 1 || a.wt_taps != 1 || a.pad_h != 0 || a.pad_w != 0 ||
      a.mul != 1 || a.Hin != a.Hout || a.Win != a.Wout)
    return LAUNCH_NOT_SERVED;
  if (!((C == 64 && N == 256) || (C == 128 && N == 512) || (C == 256 && N == 1024))) return LAUNCH_NOT_SERVED;
  if (a.out_ld != N || a.in_ld < C || (a.in_ld & 7) || a.M < 1) return LAUNCH_NOT_SERVED;
  if ((unsigned long long)a.M * a.in_ld * 2ull >= 0xffffffffull || (unsigned long long)a.M * N * 2ull >= 0xffffffffull) return LAUNCH_NOT_SERVED;
  if (!a.stats || !a.out || !t.g2 || !t.y || !t.bits || !t.mean || !t.invstd) return LAUNCH_NOT_SERVED;
  const int code = U2_K_STREAM + U2_K_STREAM_TAIL + (C / 32) * 10;
  a.abl = 0;
  if (C == 64) return launch_stream_cfg<2, 128, 1, 4, 2, true>(a, N, tiny, forced, code, s, t);
  if (C == 128) return launch_stream_cfg<4, 64, 1, 4, 4, true>(a, N, tiny, forced, code, s, t);
  return launch_stream_cfg<8, 64, 2, 8, 8, true>(a, N, tiny, forced, code, s, t);
}

}  // namespace u2conv
