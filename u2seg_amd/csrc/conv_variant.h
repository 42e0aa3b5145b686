// The `variant` words of the convolution entry points (include/u2seg_hip.h, "the variant words"), decoded once into named
// fields.  Host only, no HIP includes: tests/native/variant_decode.cpp builds it with a plain C++ compiler.  This header and the
// public one are the only places that know a bit position.
#pragma once
#include "u2seg_hip.h"

namespace u2conv {

// a kernel family steered by a force / forbid pair of bits; the values are what conv_tile.hip's launchers take as `sk`
enum class Choice : int { Never = 0, Auto = 1, Force = 2 };

namespace variant_detail {
constexpr bool bit(unsigned w, unsigned mask) { return (w & mask) != 0; }
constexpr int field(unsigned w, int shift, unsigned mask) { return (int)((w >> shift) & mask); }
constexpr Choice choice(unsigned w, unsigned force, unsigned forbid) {
  return bit(w, forbid) ? Choice::Never : bit(w, force) ? Choice::Force : Choice::Auto;
}
constexpr Choice choice_force_first(unsigned w, unsigned force, unsigned forbid) {
  return bit(w, force) ? Choice::Force : bit(w, forbid) ? Choice::Never : Choice::Auto;
}
}  // namespace variant_detail

// the conv word
struct ConvVariant {
  // conv_igemm.hip
  bool reg_staging, bk32, tile_256x128;
  int ring;              // 0 = default, 1-3 = 2-4 stages
  Choice wide;           // conv_igemm256
  bool wide_stagger, wide_stagger_parity;
  // conv_tile.hip
  int tile_cfg;          // 0 = automatic, 1-7, U2_CV_TILE_CFG_NEVER
  Choice streamk;
  // every persistent family
  bool tiny;
  // conv_stream.hip / conv_halo.hip
  Choice stream, halo;
  bool halo_tile128;     // the same bit as stream == Force (the documented alias)
  int halo_sched;
  int abl;               // ConvArgs::abl
  bool explicit_kernel;  // any bit of U2_CV_EXPLICIT_MASK: stays off the streaming kernel
};

inline ConvVariant decode_conv_variant(unsigned w) {
  using namespace variant_detail;
  ConvVariant v;
  v.reg_staging = bit(w, U2_CV_REG_STAGING);
  v.bk32 = bit(w, U2_CV_BK32);
  v.tile_256x128 = bit(w, U2_CV_TILE_256X128);
  v.ring = field(w, U2_CV_RING_SHIFT, U2_CV_RING_MASK);
  v.wide = choice(w, U2_CV_WIDE_FORCE, U2_CV_WIDE_FORBID);
  v.wide_stagger = bit(w, U2_CV_WIDE_STAGGER);
  v.wide_stagger_parity = bit(w, U2_CV_WIDE_STAGGER_PARITY);
  v.tile_cfg = field(w, U2_CV_TILE_CFG_SHIFT, U2_CV_TILE_CFG_MASK);
  v.streamk = choice(w, U2_CV_STREAMK_FORCE, U2_CV_STREAMK_FORBID);
  v.tiny = bit(w, U2_CV_TINY_GRID);
  v.stream = choice(w, U2_CV_STREAM_FORCE, U2_CV_STREAM_FORBID);
  v.halo = choice(w, U2_CV_HALO_FORCE, U2_CV_HALO_FORBID);
  v.halo_tile128 = bit(w, U2_CV_HALO_TILE128);
  v.halo_sched = field(w, U2_CV_HALO_SCHED_SHIFT, U2_CV_HALO_SCHED_MASK);
  v.abl = field(w, U2_CV_ABL_SHIFT, U2_CV_ABL_MASK);
  v.explicit_kernel = bit(w, U2_CV_EXPLICIT_MASK);
  return v;
}

// the wgrad word
struct WgradVariant {
  // per-tap kernels (conv_wgrad.hip)
  bool reg_staging, scalar_gather;
  int fewer_splits, ring;
  Choice xcd, wide;      // force wins over forbid in both
  bool atomics, partials_force;
  // wgrad_halo.hip
  Choice halo;
  int halo_rounds;       // rounds of work-groups (the field + 1)
  // wgrad_stream.hip
  Choice stream;
  bool stream_tiny;
  int stream_cfg, stream_per_cu;
  bool per_tap_stream, per_tap_halo;  // any bit of U2_WG_PER_TAP_MASK_STREAM / _HALO: stays off that kernel
};

inline WgradVariant decode_wgrad_variant(unsigned w) {
  using namespace variant_detail;
  WgradVariant v;
  v.reg_staging = bit(w, U2_WG_REG_STAGING);
  v.scalar_gather = bit(w, U2_WG_SCALAR_GATHER);
  v.fewer_splits = field(w, U2_WG_FEWER_SPLITS_SHIFT, U2_WG_FEWER_SPLITS_MASK);
  v.ring = field(w, U2_WG_RING_SHIFT, U2_WG_RING_MASK);
  v.xcd = choice_force_first(w, U2_WG_XCD_FORCE, U2_WG_XCD_FORBID);
  v.wide = choice_force_first(w, U2_WG_WIDE_FORCE, U2_WG_WIDE_FORBID);
  v.atomics = bit(w, U2_WG_ATOMICS);
  v.partials_force = bit(w, U2_WG_PARTIALS_FORCE);
  v.halo = choice(w, U2_WG_HALO_FORCE, U2_WG_HALO_FORBID);
  v.halo_rounds = field(w, U2_WG_HALO_ROUNDS_SHIFT, U2_WG_HALO_ROUNDS_MASK) + 1;
  v.stream = choice(w, U2_WG_STREAM_FORCE, U2_WG_STREAM_FORBID);
  v.stream_tiny = bit(w, U2_WG_STREAM_TINY);
  v.stream_cfg = field(w, U2_WG_STREAM_CFG_SHIFT, U2_WG_STREAM_CFG_MASK);
  v.stream_per_cu = field(w, U2_WG_STREAM_PER_CU_SHIFT, U2_WG_STREAM_PER_CU_MASK);
  v.per_tap_stream = bit(w, U2_WG_PER_TAP_MASK_STREAM);
  v.per_tap_halo = bit(w, U2_WG_PER_TAP_MASK_HALO);
  return v;
}

// the fused 1x1 backward word
struct FusedBwdVariant {
  bool force, tiny, never;
  bool bn_two_groups, bn_wide;  // read by u2_conv1x1_bwd_fused_bn only
};

inline FusedBwdVariant decode_fused_bwd_variant(unsigned w) {
  using namespace variant_detail;
  FusedBwdVariant v;
  v.force = bit(w, U2_WD_FORCE);
  v.tiny = bit(w, U2_WD_TINY);
  v.never = bit(w, U2_WD_NEVER);
  v.bn_two_groups = bit(w, U2_WD_BN_TWO_GROUPS);
  v.bn_wide = bit(w, U2_WD_BN_WIDE);
  return v;
}

}  // namespace u2conv
