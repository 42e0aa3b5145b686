// Host-only check that csrc/conv_variant.h decodes the variant words of include/u2seg_hip.h exactly as the shifts and masks it
// replaced: no GPU, no HIP.  Built and run (with -fsanitize=address,undefined) by tests/test_conv_variant_host.py.
//   1. a word with only one field set differs from the all-zero decode in that field alone (plus the cross-field rule flags
//      that the header documents for the bit);
//   2. the composite numbers the tests and the self-test passed as literals decode to what they were written to mean.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "conv_variant.h"
#include "u2seg_hip.h"

using namespace u2conv;
using Fields = std::vector<std::pair<std::string, int>>;

static int fails = 0;

static Fields list(const ConvVariant& v) {
  return {{"reg_staging", v.reg_staging}, {"bk32", v.bk32}, {"tile_256x128", v.tile_256x128}, {"ring", v.ring},
          {"wide", (int)v.wide}, {"wide_stagger", v.wide_stagger}, {"wide_stagger_parity", v.wide_stagger_parity},
          {"tile_cfg", v.tile_cfg}, {"streamk", (int)v.streamk}, {"tiny", v.tiny}, {"stream", (int)v.stream},
          {"halo", (int)v.halo}, {"halo_tile128", v.halo_tile128}, {"halo_sched", v.halo_sched}, {"abl", v.abl},
          {"explicit_kernel", v.explicit_kernel}};
}
static Fields list(const WgradVariant& v) {
  return {{"reg_staging", v.reg_staging}, {"scalar_gather", v.scalar_gather}, {"fewer_splits", v.fewer_splits}, {"ring", v.ring},
          {"xcd", (int)v.xcd}, {"wide", (int)v.wide}, {"atomics", v.atomics}, {"partials_force", v.partials_force},
          {"halo", (int)v.halo}, {"halo_rounds", v.halo_rounds}, {"stream", (int)v.stream}, {"stream_tiny", v.stream_tiny},
          {"stream_cfg", v.stream_cfg}, {"stream_per_cu", v.stream_per_cu}, {"per_tap_stream", v.per_tap_stream},
          {"per_tap_halo", v.per_tap_halo}};
}
static Fields list(const FusedBwdVariant& v) {
  return {{"force", v.force}, {"tiny", v.tiny}, {"never", v.never}, {"bn_two_groups", v.bn_two_groups}, {"bn_wide", v.bn_wide}};
}
static Fields list_conv(unsigned w) { return list(decode_conv_variant(w)); }
static Fields list_wgrad(unsigned w) { return list(decode_wgrad_variant(w)); }
static Fields list_fused(unsigned w) { return list(decode_fused_bwd_variant(w)); }

// `got` must differ from `zero` in exactly the fields of `want` (name -> value)
static void expect(const char* what, unsigned word, const Fields& zero, const Fields& got, const Fields& want) {
  for (size_t i = 0; i < got.size(); ++i) {
    int expected = zero[i].second;
    bool listed = false;
    for (const auto& w : want)
      if (w.first == got[i].first) { expected = w.second; listed = true; }
    if (got[i].second != expected || (listed && expected == zero[i].second)) {
      printf("FAIL %s (word %#x): field %s = %d, expected %d%s\n", what, word, got[i].first.c_str(), got[i].second, expected,
             listed && expected == zero[i].second ? " (the expectation equals the zero decode: it checks nothing)" : "");
      ++fails;
    }
  }
  for (const auto& w : want) {
    bool known = false;
    for (const auto& g : got) known = known || g.first == w.first;
    if (!known) { printf("FAIL %s: no field named %s\n", what, w.first.c_str()); ++fails; }
  }
}

struct Case {
  const char* name;
  unsigned word;
  Fields want;
};

static void run(const char* word_name, Fields (*decode)(unsigned), const std::vector<Case>& cases) {
  const Fields zero = decode(0);
  for (const auto& c : cases) expect((std::string(word_name) + " " + c.name).c_str(), c.word, zero, decode(c.word), c.want);
}

int main() {
  const int NEVER = (int)Choice::Never, AUTO = (int)Choice::Auto, FORCE = (int)Choice::Force;
  // the all-zero words: the library's own choice everywhere
  for (const auto& f : list_conv(0))
    if (f.second != ((f.first == "wide" || f.first == "streamk" || f.first == "stream" || f.first == "halo") ? AUTO : 0)) {
      printf("FAIL conv word 0: %s = %d\n", f.first.c_str(), f.second); ++fails;
    }
  for (const auto& f : list_wgrad(0))
    if (f.second != ((f.first == "xcd" || f.first == "wide" || f.first == "halo" || f.first == "stream") ? AUTO : f.first == "halo_rounds" ? 1 : 0)) {
      printf("FAIL wgrad word 0: %s = %d\n", f.first.c_str(), f.second); ++fails;
    }
  for (const auto& f : list_fused(0))
    if (f.second != 0) { printf("FAIL fused word 0: %s = %d\n", f.first.c_str(), f.second); ++fails; }

  // ---- 1. one field at a time (explicit_kernel / per_tap_*: the cross-field rule flags of the header) ----
  const std::pair<std::string, int> EXPL{"explicit_kernel", 1};
  run("conv", list_conv, {
      {"REG_STAGING", U2_CV_REG_STAGING, {{"reg_staging", 1}, EXPL}},
      {"BK32", U2_CV_BK32, {{"bk32", 1}, EXPL}},
      {"TILE_256X128", U2_CV_TILE_256X128, {{"tile_256x128", 1}, EXPL}},
      {"RING", (unsigned)U2_CV_RING_MASK << U2_CV_RING_SHIFT, {{"ring", 3}, EXPL}},
      {"WIDE_FORCE", U2_CV_WIDE_FORCE, {{"wide", FORCE}, EXPL}},
      {"WIDE_FORBID", U2_CV_WIDE_FORBID, {{"wide", NEVER}, EXPL}},
      {"WIDE_STAGGER", U2_CV_WIDE_STAGGER, {{"wide_stagger", 1}, EXPL}},
      {"WIDE_STAGGER_PARITY", U2_CV_WIDE_STAGGER_PARITY, {{"wide_stagger_parity", 1}, EXPL}},
      {"TILE_CFG", (unsigned)U2_CV_TILE_CFG_MASK << U2_CV_TILE_CFG_SHIFT, {{"tile_cfg", U2_CV_TILE_CFG_NEVER}, EXPL}},
      {"TINY_GRID", U2_CV_TINY_GRID, {{"tiny", 1}}},
      {"STREAM_FORCE = HALO_TILE128 (the alias)", U2_CV_STREAM_FORCE, {{"stream", FORCE}, {"halo_tile128", 1}}},
      {"ABL", (unsigned)U2_CV_ABL_MASK << U2_CV_ABL_SHIFT, {{"abl", 63}}},
      {"ABL_NO_STORES", U2_CV_ABL_NO_STORES, {{"abl", 1}}},
      {"ABL_NO_STATS", U2_CV_ABL_NO_STATS, {{"abl", 2}}},
      {"ABL_NO_EPILOGUE", U2_CV_ABL_NO_EPILOGUE, {{"abl", 4}}},
      {"ABL_NT_STORES", U2_CV_ABL_NT_STORES, {{"abl", 8}}},
      {"ABL_NO_STATS_FLUSH", U2_CV_ABL_NO_STATS_FLUSH, {{"abl", 16}}},
      {"HALO_FORCE", U2_CV_HALO_FORCE, {{"halo", FORCE}}},
      {"HALO_FORBID", U2_CV_HALO_FORBID, {{"halo", NEVER}}},
      {"STREAM_FORBID", U2_CV_STREAM_FORBID, {{"stream", NEVER}}},
      {"STREAMK_FORCE", U2_CV_STREAMK_FORCE, {{"streamk", FORCE}}},
      {"STREAMK_FORBID", U2_CV_STREAMK_FORBID, {{"streamk", NEVER}}},
      {"HALO_SCHED", (unsigned)U2_CV_HALO_SCHED_MASK << U2_CV_HALO_SCHED_SHIFT, {{"halo_sched", 3}}},
      // the unnamed bits 1, 6, 7 carry nothing but the rule
      {"bit 1", 1u << 1, {EXPL}}, {"bit 6", 1u << 6, {EXPL}}, {"bit 7", 1u << 7, {EXPL}},
      {"bit 23 (top of ABL)", 1u << 23, {{"abl", 32}}},
      // forbid wins over force in every pair of the conv word
      {"WIDE both", U2_CV_WIDE_FORCE | U2_CV_WIDE_FORBID, {{"wide", NEVER}, EXPL}},
      {"HALO both", U2_CV_HALO_FORCE | U2_CV_HALO_FORBID, {{"halo", NEVER}}},
      {"STREAM both", U2_CV_STREAM_FORCE | U2_CV_STREAM_FORBID, {{"stream", NEVER}, {"halo_tile128", 1}}},
      {"STREAMK both", U2_CV_STREAMK_FORCE | U2_CV_STREAMK_FORBID, {{"streamk", NEVER}}},
  });
  const std::pair<std::string, int> PTS{"per_tap_stream", 1}, PTH{"per_tap_halo", 1};
  run("wgrad", list_wgrad, {
      {"REG_STAGING", U2_WG_REG_STAGING, {{"reg_staging", 1}, PTS, PTH}},
      {"SCALAR_GATHER", U2_WG_SCALAR_GATHER, {{"scalar_gather", 1}, PTS, PTH}},
      {"FEWER_SPLITS", (unsigned)U2_WG_FEWER_SPLITS_MASK << U2_WG_FEWER_SPLITS_SHIFT, {{"fewer_splits", 3}, PTS, PTH}},
      {"XCD_FORCE", U2_WG_XCD_FORCE, {{"xcd", FORCE}, PTS, PTH}},
      {"XCD_FORBID", U2_WG_XCD_FORBID, {{"xcd", NEVER}, PTS, PTH}},
      {"WIDE_FORCE", U2_WG_WIDE_FORCE, {{"wide", FORCE}, PTS, PTH}},
      {"RING", (unsigned)U2_WG_RING_MASK << U2_WG_RING_SHIFT, {{"ring", 3}, PTS, PTH}},
      {"WIDE_FORBID", U2_WG_WIDE_FORBID, {{"wide", NEVER}, PTS}},   // bit 11: outside the halo rule's mask
      {"HALO_FORCE", U2_WG_HALO_FORCE, {{"halo", FORCE}}},
      {"HALO_FORBID", U2_WG_HALO_FORBID, {{"halo", NEVER}}},
      {"HALO_ROUNDS", (unsigned)U2_WG_HALO_ROUNDS_MASK << U2_WG_HALO_ROUNDS_SHIFT, {{"halo_rounds", 4}}},
      {"ATOMICS", U2_WG_ATOMICS, {{"atomics", 1}}},
      {"PARTIALS_FORCE", U2_WG_PARTIALS_FORCE, {{"partials_force", 1}}},
      {"STREAM_FORCE", U2_WG_STREAM_FORCE, {{"stream", FORCE}}},
      {"STREAM_FORBID", U2_WG_STREAM_FORBID, {{"stream", NEVER}}},
      {"STREAM_TINY", U2_WG_STREAM_TINY, {{"stream_tiny", 1}}},
      {"STREAM_CFG", (unsigned)U2_WG_STREAM_CFG_MASK << U2_WG_STREAM_CFG_SHIFT, {{"stream_cfg", 7}}},
      {"STREAM_PER_CU", (unsigned)U2_WG_STREAM_PER_CU_MASK << U2_WG_STREAM_PER_CU_SHIFT, {{"stream_per_cu", 3}}},
      {"bit 2", 1u << 2, {PTS, PTH}}, {"bit 3", 1u << 3, {PTS, PTH}},
      // force wins in the two pairs of the per-tap kernels, forbid in the others
      {"XCD both", U2_WG_XCD_FORCE | U2_WG_XCD_FORBID, {{"xcd", FORCE}, PTS, PTH}},
      {"WIDE both", U2_WG_WIDE_FORCE | U2_WG_WIDE_FORBID, {{"wide", FORCE}, PTS, PTH}},
      {"HALO both", U2_WG_HALO_FORCE | U2_WG_HALO_FORBID, {{"halo", NEVER}}},
      {"STREAM both", U2_WG_STREAM_FORCE | U2_WG_STREAM_FORBID, {{"stream", NEVER}}},
  });
  run("fused", list_fused, {
      {"FORCE", U2_WD_FORCE, {{"force", 1}}},
      {"TINY", U2_WD_TINY, {{"tiny", 1}}},
      {"NEVER", U2_WD_NEVER, {{"never", 1}}},
      {"BN_TWO_GROUPS", U2_WD_BN_TWO_GROUPS, {{"bn_two_groups", 1}}},
      {"BN_WIDE", U2_WD_BN_WIDE, {{"bn_wide", 1}}},
  });

  // ---- 2. the numbers the tests and the self-test used to write out, with what they were written to mean ----
  run("conv legacy", list_conv, {
      {"15 << 12: never a tile kernel", 15u << 12, {{"tile_cfg", 15}, EXPL}},
      {"NEVER_TILE | 8 | 4 | 32: 256 x 128 tile, BK 32, 3 stages", (15u << 12) | 8 | 4 | 32,
       {{"tile_cfg", 15}, {"tile_256x128", 1}, {"bk32", 1}, {"ring", 2}, EXPL}},
      {"NEVER_TILE | 48: 4 stages", (15u << 12) | 48, {{"tile_cfg", 15}, {"ring", 3}, EXPL}},
      {"NEVER_TILE | 4 | 16 | 1", (15u << 12) | 4 | 16 | 1, {{"tile_cfg", 15}, {"bk32", 1}, {"ring", 1}, {"reg_staging", 1}, EXPL}},
      {"NEVER_TILE | 256 | 1024 | 2048: igemm256 staggered by parity", (15u << 12) | 256 | 1024 | 2048,
       {{"tile_cfg", 15}, {"wide", FORCE}, {"wide_stagger", 1}, {"wide_stagger_parity", 1}, EXPL}},
      {"512 | 4 | 16: no igemm256, BK 32, 2 stages", 512 | 4 | 16, {{"wide", NEVER}, {"bk32", 1}, {"ring", 1}, EXPL}},
      {"(3 << 12) | (1 << 16): configuration 3 on 8 work-groups", (3u << 12) | (1u << 16), {{"tile_cfg", 3}, {"tiny", 1}, EXPL}},
      {"(7 << 12) | (1 << 27) | (1 << 16): configuration 7, stream-K, 8 work-groups", (7u << 12) | (1u << 27) | (1u << 16),
       {{"tile_cfg", 7}, {"streamk", FORCE}, {"tiny", 1}, EXPL}},
      {"(7 << 12) | (1 << 28): configuration 7, whole tiles", (7u << 12) | (1u << 28), {{"tile_cfg", 7}, {"streamk", NEVER}, EXPL}},
      {"1 << 28: the product path's stream-K forbid", 1u << 28, {{"streamk", NEVER}}},
      {"(1 << 24) | (1 << 16): halo kernel on 8 work-groups", (1u << 24) | (1u << 16), {{"halo", FORCE}, {"tiny", 1}}},
      {"(1 << 24) | (1 << 17) | (1 << 16): halo kernel, 128-channel tiles", (1u << 24) | (1u << 17) | (1u << 16),
       {{"halo", FORCE}, {"halo_tile128", 1}, {"stream", FORCE}, {"tiny", 1}}},
      {"(1 << 17) | (1 << 16): streaming kernel on 8 work-groups per block", (1u << 17) | (1u << 16),
       {{"stream", FORCE}, {"halo_tile128", 1}, {"tiny", 1}}},
      {"3 << 29: both halo schedule switches (bit 30 through an unsigned shift)", 3u << 29, {{"halo_sched", 3}}},
  });
  run("wgrad legacy", list_wgrad, {
      {"3: register staging, scalar gathers", 3, {{"reg_staging", 1}, {"scalar_gather", 1}, PTS, PTH}},
      {"256 | 64: 256-wide tiles, XCD-grouped", 256 | 64, {{"wide", FORCE}, {"xcd", FORCE}, PTS, PTH}},
      {"128: never XCD-grouped", 128, {{"xcd", NEVER}, PTS, PTH}},
      {"16 / 32: splits halved once / twice", 32, {{"fewer_splits", 2}, PTS, PTH}},
      {"1 << 9 / 2 << 9: ring of 3 / 4", 2u << 9, {{"ring", 2}, PTS, PTH}},
      {"2048: never the 256-wide tiles", 2048, {{"wide", NEVER}, PTS}},
      {"131072 | 256: reduction pass, 256-wide tiles", 131072 | 256, {{"partials_force", 1}, {"wide", FORCE}, PTS, PTH}},
      {"65536: atomics", 65536, {{"atomics", 1}}},
      {"4096: halo kernel", 4096, {{"halo", FORCE}}},
      {"8192: never the halo kernel", 8192, {{"halo", NEVER}}},
      {"4096 | (1 << 17) | (1 << 14): halo kernel, partial blocks, two rounds", 4096 | (1u << 17) | (1u << 14),
       {{"halo", FORCE}, {"partials_force", 1}, {"halo_rounds", 2}}},
      {"4096 | (1 << 16): halo kernel, atomics", 4096 | (1u << 16), {{"halo", FORCE}, {"atomics", 1}}},
      {"1 << 19: never the streaming kernel", 1u << 19, {{"stream", NEVER}}},
      {"(1 << 18) | (1 << 20) | (4 << 21): streaming kernel, 8 ranges, block 4", (1u << 18) | (1u << 20) | (4u << 21),
       {{"stream", FORCE}, {"stream_tiny", 1}, {"stream_cfg", 4}}},
      {"(1 << 18) | (2 << 21) | (1 << 24): streaming kernel, block 2, one work-group per CU", (1u << 18) | (2u << 21) | (1u << 24),
       {{"stream", FORCE}, {"stream_cfg", 2}, {"stream_per_cu", 1}}},
  });
  run("fused legacy", list_fused, {
      {"1 | 2: forced, 8 pixel ranges", 1 | 2, {{"force", 1}, {"tiny", 1}}},
      {"4: never", 4, {{"never", 1}}},
      {"3 | 8: forced, 8 ranges, the 4-wave block", 3 | 8, {{"force", 1}, {"tiny", 1}, {"bn_two_groups", 1}}},
      {"1 | 16: forced, the N <= 512 block", 1 | 16, {{"force", 1}, {"bn_wide", 1}}},
  });
  // what u2_conv1x1_bwd_fused_bn used to hand on as (variant & 1) | ((variant >> 2) & 2) | ((variant >> 2) & 4)
  for (unsigned w = 0; w < 32; ++w) {
    const FusedBwdVariant v = decode_fused_bwd_variant(w);
    const unsigned packed = (w & 1) | ((w >> 2) & 2) | ((w >> 2) & 4);
    if ((unsigned)v.force != (packed & 1) || (unsigned)v.bn_two_groups != ((packed >> 1) & 1) || (unsigned)v.bn_wide != ((packed >> 2) & 1) ||
        (unsigned)v.tiny != ((w >> 1) & 1) || (unsigned)v.never != ((w >> 2) & 1)) {
      printf("FAIL fused word %u against the old packing\n", w); ++fails;
    }
  }
  printf("VARIANT_DECODE %s (%d failures)\n", fails ? "FAILED" : "OK", fails);
  return fails ? 1 : 0;
}
