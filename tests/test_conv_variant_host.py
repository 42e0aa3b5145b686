"""The variant words and kernel codes of include/u2seg_hip.h, without a GPU: the values the binding parses are pinned to the
numbers recorded command lines carry (profiles/, tools/exp/), the fields of a word do not overlap, the constant block leaves the
prototype table alone, and csrc/conv_variant.h decodes the words as the shifts and masks it replaced (tests/native/
variant_decode.cpp, built with the host compiler and -fsanitize=address,undefined)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from u2seg_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The pin: today's values, written out.  These numbers are in recorded command lines; a change here breaks their meaning.
PINNED = {
    # the conv word
    "U2_CV_REG_STAGING": 1, "U2_CV_BK32": 4, "U2_CV_TILE_256X128": 8, "U2_CV_RING_SHIFT": 4, "U2_CV_RING_MASK": 3,
    "U2_CV_WIDE_FORCE": 256, "U2_CV_WIDE_FORBID": 512, "U2_CV_WIDE_STAGGER": 1024, "U2_CV_WIDE_STAGGER_PARITY": 2048,
    "U2_CV_TILE_CFG_SHIFT": 12, "U2_CV_TILE_CFG_MASK": 15, "U2_CV_TILE_CFG_NEVER": 15, "U2_CV_TINY_GRID": 1 << 16,
    "U2_CV_STREAM_FORCE": 1 << 17, "U2_CV_HALO_TILE128": 1 << 17, "U2_CV_ABL_SHIFT": 18, "U2_CV_ABL_MASK": 63,
    "U2_CV_ABL_NO_STORES": 1 << 18, "U2_CV_ABL_NO_STATS": 1 << 19, "U2_CV_ABL_NO_EPILOGUE": 1 << 20, "U2_CV_ABL_NT_STORES": 1 << 21,
    "U2_CV_ABL_NO_STATS_FLUSH": 1 << 22, "U2_CV_HALO_FORCE": 1 << 24, "U2_CV_HALO_FORBID": 1 << 25, "U2_CV_STREAM_FORBID": 1 << 26,
    "U2_CV_STREAMK_FORCE": 1 << 27, "U2_CV_STREAMK_FORBID": 1 << 28, "U2_CV_HALO_SCHED_SHIFT": 29, "U2_CV_HALO_SCHED_MASK": 3,
    "U2_CV_EXPLICIT_MASK": 0xffff,
    # the wgrad word
    "U2_WG_REG_STAGING": 1, "U2_WG_SCALAR_GATHER": 2, "U2_WG_FEWER_SPLITS_SHIFT": 4, "U2_WG_FEWER_SPLITS_MASK": 3,
    "U2_WG_XCD_FORCE": 64, "U2_WG_XCD_FORBID": 128, "U2_WG_WIDE_FORCE": 256, "U2_WG_RING_SHIFT": 9, "U2_WG_RING_MASK": 3,
    "U2_WG_WIDE_FORBID": 2048, "U2_WG_HALO_FORCE": 4096, "U2_WG_HALO_FORBID": 8192, "U2_WG_HALO_ROUNDS_SHIFT": 14,
    "U2_WG_HALO_ROUNDS_MASK": 3, "U2_WG_ATOMICS": 65536, "U2_WG_PARTIALS_FORCE": 131072, "U2_WG_STREAM_FORCE": 1 << 18,
    "U2_WG_STREAM_FORBID": 1 << 19, "U2_WG_STREAM_TINY": 1 << 20, "U2_WG_STREAM_CFG_SHIFT": 21, "U2_WG_STREAM_CFG_MASK": 7,
    "U2_WG_STREAM_PER_CU_SHIFT": 24, "U2_WG_STREAM_PER_CU_MASK": 3, "U2_WG_PER_TAP_MASK_STREAM": 0xfff,
    "U2_WG_PER_TAP_MASK_HALO": 0x7ff,
    # the fused 1x1 backward word
    "U2_WD_FORCE": 1, "U2_WD_TINY": 2, "U2_WD_NEVER": 4, "U2_WD_BN_TWO_GROUPS": 8, "U2_WD_BN_WIDE": 16,
    # u2_conv_last_kernel
    "U2_K_TILE": 100, "U2_K_IGEMM256": 256, "U2_K_IGEMM256_STAGGER": 1024, "U2_K_HALO": 300, "U2_K_HALO_N64": 301,
    "U2_K_STREAMK": 500, "U2_K_STREAM": 700, "U2_K_STREAM_TAIL": 5, "U2_K_IGEMM": 1000000, "U2_K_WGRAD": 2000,
    "U2_K_WGRAD_XCD": 100, "U2_K_WGRAD256": 2256, "U2_K_WGRAD_STREAM": 2700, "U2_K_WDGRAD": 2750, "U2_K_WDGRAD_BN": 2760,
    "U2_K_WGRAD_HALO": 2900,
}
# Names that are not fields of their own: values of a field, the bits inside the ABL field, the cross-field rule masks.
NOT_FIELDS = {"U2_CV_TILE_CFG_NEVER", "U2_CV_EXPLICIT_MASK", "U2_WG_PER_TAP_MASK_STREAM", "U2_WG_PER_TAP_MASK_HALO"}
ABL_BITS = ["U2_CV_ABL_NO_STORES", "U2_CV_ABL_NO_STATS", "U2_CV_ABL_NO_EPILOGUE", "U2_CV_ABL_NT_STORES", "U2_CV_ABL_NO_STATS_FLUSH"]
# The one documented alias: bit 17 of the conv word, read by two kernel families.
ALIASES = [("U2_CV_STREAM_FORCE", "U2_CV_HALO_TILE128")]


def word_fields(table, prefix):
    """{field name: mask in the word} of one variant word: X_SHIFT / X_MASK pairs become X."""
    out = {}
    for name, value in table.items():
        if not name.startswith(prefix) or name in NOT_FIELDS or name in ABL_BITS or name.endswith("_MASK"):
            continue
        if name.endswith("_SHIFT"):
            out[name[:-6]] = table[name[:-6] + "_MASK"] << value
        else:
            out[name] = value
    return out


def test_constants_are_the_recorded_values():
    table = _hip.constants()
    variant_names = {k: v for k, v in table.items() if re.match(r"U2_(CV|WG|WD|K)_", k)}
    assert variant_names == PINNED
    assert _hip.K.CV_STREAMK_FORBID == 1 << 28   # what layers/functional.py passes outside the bottom-up backbone
    from u2seg_amd.layers import functional
    assert functional._NO_STREAMK == 1 << 28


@pytest.mark.parametrize("prefix", ["U2_CV_", "U2_WG_", "U2_WD_"])
def test_fields_of_a_word_are_disjoint(prefix):
    fields = word_fields(_hip.constants(), prefix)
    assert fields
    names = sorted(fields)
    for i, a in enumerate(names):
        assert 0 < fields[a] < 1 << 31, "%s reaches bit 31" % a
        for b in names[i + 1:]:
            if (a, b) in ALIASES or (b, a) in ALIASES:
                assert fields[a] == fields[b]
            else:
                assert fields[a] & fields[b] == 0, "%s and %s overlap" % (a, b)


def test_abl_bits_and_rule_masks_lie_where_the_header_says():
    t = _hip.constants()
    abl = t["U2_CV_ABL_MASK"] << t["U2_CV_ABL_SHIFT"]
    for k, name in enumerate(ABL_BITS):
        assert t[name] == 1 << (t["U2_CV_ABL_SHIFT"] + k) and t[name] & abl   # ConvArgs::abl bit k
    conv, wgrad = word_fields(t, "U2_CV_"), word_fields(t, "U2_WG_")
    # bits 0-15 of the conv word: exactly the igemm and tile-configuration fields
    assert {n for n, m in conv.items() if m & t["U2_CV_EXPLICIT_MASK"]} == {
        "U2_CV_REG_STAGING", "U2_CV_BK32", "U2_CV_TILE_256X128", "U2_CV_RING", "U2_CV_WIDE_FORCE", "U2_CV_WIDE_FORBID",
        "U2_CV_WIDE_STAGGER", "U2_CV_WIDE_STAGGER_PARITY", "U2_CV_TILE_CFG"}
    per_tap = {"U2_WG_REG_STAGING", "U2_WG_SCALAR_GATHER", "U2_WG_FEWER_SPLITS", "U2_WG_XCD_FORCE", "U2_WG_XCD_FORBID",
               "U2_WG_WIDE_FORCE", "U2_WG_RING", "U2_WG_WIDE_FORBID"}
    assert {n for n, m in wgrad.items() if m & t["U2_WG_PER_TAP_MASK_STREAM"]} == per_tap
    assert {n for n, m in wgrad.items() if m & t["U2_WG_PER_TAP_MASK_HALO"]} == per_tap - {"U2_WG_WIDE_FORBID"}
    assert t["U2_CV_TILE_CFG_NEVER"] <= t["U2_CV_TILE_CFG_MASK"]


def test_constant_parser_takes_literals_and_shifts_only(tmp_path):
    good = tmp_path / "good.h"
    good.write_text("/* c */\n#define U2_A 7\n#define U2_B 0x10u /* c */\n#define U2_C (1u << 30)\n# define U2_D ( 3 << 0x4 )\n#define OTHER f(x)\n")
    assert _hip.constants(str(good)) == {"U2_A": 7, "U2_B": 16, "U2_C": 1 << 30, "U2_D": 48}
    for bad in ("U2_A | 1", "(U2_A << 2)", "__import__('os')", "(1 << 2) + 1", "1 << 2", "-1"):
        h = tmp_path / "bad.h"
        h.write_text("#define U2_A 1\n#define U2_X %s\n" % bad)
        with pytest.raises(ValueError):
            _hip.constants(str(h))


def test_prototype_table_is_untouched_by_the_constant_block(tmp_path):
    """declared_symbols() returns what it returned before the block existed: the same table with every #define line taken out,
    and the convolution entry points with the signatures the library exports."""
    decl = _hip.declared_symbols()
    stripped = tmp_path / "stripped.h"
    stripped.write_text(re.sub(r"^[ \t]*#[ \t]*define[ \t]+U2_\w+[ \t].*$", "", open(_hip._HEADER).read(), flags=re.M))
    bare = _hip.declared_symbols(str(stripped))
    assert list(bare) == list(decl) and bare == decl
    p, i, q = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert decl["u2_conv_igemm"] == (i, [p] * 5 + [i] * 18 + [p])
    assert decl["u2_conv_wgrad"] == (i, [p] * 3 + [i] * 15 + [p])
    assert decl["u2_conv_wgrad_into"] == (i, [p] * 3 + [i] * 16 + [q, i, i, i, p])
    assert decl["u2_conv1x1_bwd_fused"] == (i, [p] * 5 + [i] * 9 + [q, i, i, p])
    assert decl["u2_conv1x1_bwd_fused_bn"] == (i, [p] * 9 + [i] * 9 + [q, i, i, p])
    assert decl["u2_conv_dgrad_tail"] == (i, [p] * 9 + [i] * 8 + [p])
    assert decl["u2_conv_last_kernel"] == (i, [])
    assert decl["u2_abi_version"] == (i, [])


def test_decoder_equals_the_shifts_it_replaced(tmp_path):
    """tests/native/variant_decode.cpp: the host-only header against every field and against the composite numbers the tests
    used to write as literals, under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded into python)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "variant_decode")
    # the sanitizer runtimes linked statically: the program then runs whatever else the environment preloads
    static = ["-static-libsan"] if "clang" in os.path.basename(os.path.realpath(cxx)) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined"] + static + ["-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "u2seg_amd", "csrc"), os.path.join(ROOT, "tests", "native", "variant_decode.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert out.returncode == 0 and "VARIANT_DECODE OK" in out.stdout, out.stdout
