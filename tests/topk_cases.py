"""Inputs of tests/test_gpu_topk_rows.py: rows built to land where the radix selection of u2seg_amd/csrc/select.hip decides.
Plain torch / numpy on the CPU; nothing here touches the HIP library.  Every builder asserts its own premise (the digit of the
k-th key, the early exit, the tie run that straddles k, the decoys that beat every real value, the seam positions), so that an
edit cannot quietly turn a case into a random one; tests/test_topk_cases_host.py runs the builders without a GPU.

A case is a dict in the terms of the C ABI (U2TopkSeg of include/u2seg_hip.h): `store` is the flat value storage, element i of
row r lives at store[offset + r * row_stride + (i // group) * pitch + i % group].  expect(case) is topk_rows_ref on it."""
import numpy as np
import torch

from tests import float64_refs as R

BF16 = torch.bfloat16
MAX_K = 16384
QNAN32 = 0x7FC00000


# ----------------------------------------------------------------------------------------------------------------------------
# bit patterns, and the ordered key of select.hip's header comment
# ----------------------------------------------------------------------------------------------------------------------------
def f32_from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def bf16_from_bits(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).view(np.int16).copy()).view(BF16)


def from_bits(bits, bf16):
    return bf16_from_bits(bits) if bf16 else f32_from_bits(bits)


def bits_of(t):
    if t.dtype == BF16:
        return t.contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.uint64)
    return t.contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)


def ordered_key(bits, largest, bf16):
    """The value half of the 64-bit key (larger = ranked earlier), on `width`-bit patterns: -0 -> +0, NaN -> quiet NaN, then the
    usual sign fold, complemented for ascending order.  bf16 keys are NOT shifted up here: they are 16-bit numbers."""
    w = 16 if bf16 else 32
    u64 = np.uint64
    sign, full = u64(1 << (w - 1)), u64((1 << w) - 1)
    inf, qnan = u64(0x7F80 << (w - 16)), u64(0x7FC0 << (w - 16))
    u = np.asarray(bits, dtype=u64)
    u = np.where(u == sign, u64(0), u)
    u = np.where((u & (sign - u64(1))) > inf, qnan, u)
    asc = np.where((u & sign) != 0, ~u & full, u | sign)
    return asc if largest else (~asc & full)


def bits_from_key(key, largest, bf16):
    """Inverse of ordered_key on the keys it can produce."""
    w = 16 if bf16 else 32
    u64 = np.uint64
    sign, full = u64(1 << (w - 1)), u64((1 << w) - 1)
    key = np.asarray(key, dtype=u64)
    asc = key if largest else (~key & full)
    return np.where((asc & sign) != 0, asc & (sign - u64(1)), ~asc & full)


def key64(bits, idx, largest, bf16):
    """(ordered value : ~index), the key the selection ranks by.  bf16: value bits 63..48, bits 47..32 zero."""
    vk = ordered_key(bits, largest, bf16) << np.uint64(48 if bf16 else 32)
    return vk | (np.uint64(0xFFFFFFFF) - np.asarray(idx, dtype=np.uint64))


def sweep_trace(keys, k, bf16):
    """What the most-significant-digit selection has to do for these participants' keys, from the contract alone: per sweep
    (8 bits from the top; bf16 skips the 16 zero bits; then the three index bytes) the digit of the k-th key and whether the
    keys whose bits so far are >= the k-th key's number exactly k - then nothing is left to separate and the sweeps end.
    Returns None when no more than k keys take part (everything is taken), else the list of (digit, exits)."""
    keys = np.sort(np.asarray(keys, dtype=np.uint64))[::-1]
    if len(keys) <= k:
        return None
    kth = keys[k - 1]
    shifts = ([56, 48] if bf16 else [56, 48, 40, 32]) + [16, 8, 0]
    trace = []
    for s in shifts:
        s = np.uint64(s)
        exits = int(((keys >> s) >= (kth >> s)).sum()) == k
        trace.append((int((kth >> s) & np.uint64(255)), exits))
        if exits:
            break
    return trace


# ----------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------
def make_case(name, store, rows, n, k, largest, dtype=None, row_stride=None, group=1, pitch=1, offset=0, mask=None, mask_value=1,
              idx_in=None, cnt=None, cnt_group=1, idx_mod=1, idx_mul=0, want_vals=True, want_cnt=True, expect=None):
    store = store.reshape(-1).contiguous()
    assert store.dtype in (torch.float32, BF16)
    if dtype is None:
        dtype = 1 if store.dtype == BF16 else 0
    assert (dtype == 1) == (store.dtype == BF16)
    span = -(-n // group) * pitch      # whole pixels: the 8-byte path loads four columns of the last pixel
    if row_stride is None:
        row_stride = span
    # nothing the kernel may touch lies outside the storage
    assert rows >= 0 and n >= 1 and pitch >= group >= 1 and offset + max(rows - 1, 0) * row_stride + span <= store.numel(), name
    if mask is not None:
        assert mask.dtype == torch.int8 and tuple(mask.shape) == (rows, n), name
    if idx_in is not None:
        assert idx_in.dtype == torch.int32 and tuple(idx_in.shape) == (rows, n), name
        assert int(idx_in.min()) >= 0 and int(idx_in.max()) + (idx_mod - 1) * idx_mul < 1 << 24, name
    if cnt is not None:
        assert n % cnt_group == 0 and cnt.dtype == torch.int32 and tuple(cnt.shape) == (rows, n // cnt_group), name
        assert int(cnt.min()) >= 0 and int(cnt.max()) <= cnt_group, name
    return dict(name=name, store=store, rows=rows, n=n, k=k, largest=int(largest), dtype=dtype, row_stride=row_stride, group=group,
                pitch=pitch, offset=offset, mask=mask, mask_value=mask_value, idx_in=idx_in, cnt=cnt, cnt_group=cnt_group,
                idx_mod=idx_mod, idx_mul=idx_mul, want_vals=want_vals, want_cnt=want_cnt, expect=expect)


def case_rows(c):
    """[rows, span] view of the storage the case's rows start in."""
    span = -(-c["n"] // c["group"]) * c["pitch"]
    return torch.as_strided(c["store"], (c["rows"], span), (c["row_stride"], 1), c["offset"])


def expect(c):
    """(values, indices, counts) the kernel must return for the case."""
    if c["expect"] is not None:
        return c["expect"]
    return R.topk_rows_ref(case_rows(c), c["k"], bool(c["largest"]), mask=c["mask"], mask_value=c["mask_value"], group=c["group"],
                           pitch=c["pitch"], n=c["n"], idx_in=c["idx_in"], cnt=c["cnt"], cnt_group=c["cnt_group"],
                           idx_mod=c["idx_mod"], idx_mul=c["idx_mul"])


def case_keys(c, row=0):
    """The 64-bit keys of the participants of one row (contiguous, position-indexed cases only)."""
    assert c["group"] == 1 and c["pitch"] == 1 and c["idx_in"] is None and c["cnt"] is None
    bf16 = c["dtype"] != 0
    v = case_rows(c)[row]
    bits = bits_of(v) >> np.uint64(16) if c["dtype"] == 2 else bits_of(v)
    keys = key64(bits, np.arange(c["n"]), c["largest"], bf16)
    if c["mask"] is not None:
        keys = keys[(c["mask"][row] == c["mask_value"]).numpy()]
    return keys


def quantised(shape, gen, bf16, step=4.0, scale=2.0):
    """Normal values rounded to 1 / step and clamped to +-15: ties abound (bf16 rounds once more, which only adds ties)."""
    v = (torch.randn(shape, generator=gen) * scale).mul(step).round().div(step).clamp(-15, 15)
    return v.to(BF16) if bf16 else v


# ---- (a) digit edges of the k-th key ---------------------------------------------------------------------------------------
def _key_of(digits):
    out = 0
    for d in digits:
        out = (out << 8) | d
    return out


def digit_edge_case(name, bf16, largest, target, exit_at=None, n=3000, seed=0):
    """One row whose k-th key has the value digits `target` (one byte per value sweep, in key space).
    exit_at None: the k-th value is shared by three adjacent elements with k on the middle one, so no sweep can end the
    selection before the last index byte: every sweep runs and sweep s has to pick bucket target[s].
    exit_at e: the k-th value is unique and no worse key shares its first e + 1 digits, but for every earlier sweep one does:
    the bucket chosen in sweep e holds exactly `want` keys and the selection ends there.
    The row has n elements plus what brings k to a power of two."""
    rng = np.random.default_rng(seed)
    d = len(target)
    assert d == (2 if bf16 else 4)
    keys = []

    def valid(key):
        bits = bits_from_key([key], largest, bf16)
        ok = int(ordered_key(bits, largest, bf16)[0]) == key
        return ok and not bool(np.isnan(from_bits(bits, bf16).float().numpy()[0]))

    def add(prefix, lo, hi):
        """a few valid keys with the given leading digits, the next digit in [lo, hi], the rest random; the ends are tried first"""
        found = 0
        for t in range(60):
            nxt = lo if t == 0 else hi if t == 1 else int(rng.integers(lo, hi + 1))
            rest = [int(x) for x in rng.integers(0, 256, d - len(prefix) - 1)]
            key = _key_of(list(prefix) + [nxt] + rest)
            if valid(key) and found < 4:
                keys.append(key)
                found += 1

    assert valid(_key_of(target)), name
    for s in range(d):
        if target[s] < 255:
            add(target[:s], target[s] + 1, 255)               # better keys that part from the target in sweep s
        if target[s] > 0 and (exit_at is None or s <= exit_at):
            add(target[:s], 0, target[s] - 1)                 # worse keys that share the first s digits
    tkey = _key_of(target)
    assert tkey not in keys
    ties = 3 if exit_at is None else 1
    fill = bits_of(quantised((n - len(keys) - ties,), torch.Generator().manual_seed(seed), bf16, step=64.0, scale=1.0))
    assert not (ordered_key(fill, largest, bf16) == tkey).any()
    bits = np.concatenate([bits_from_key(keys, largest, bf16), fill])
    rng.shuffle(bits)
    at = 1000
    bits = np.concatenate([bits[:at], bits_from_key([tkey] * ties, largest, bf16), bits[at:]])
    k = int((ordered_key(bits, largest, bf16) > tkey).sum()) + (2 if ties == 3 else 1)
    # k is brought to a power of two with infinities of the winning sign at the row's end: the survivors' LDS list then has no
    # spare slot, and a threshold that lets a single key too many through loses a key it should have kept
    pad = (1 << (k - 1).bit_length()) - k
    best = bits_of(torch.tensor([float("inf") if largest else float("-inf")]).to(BF16 if bf16 else torch.float32))
    bits = np.concatenate([bits, np.repeat(best, pad)])
    n, k = n + pad, k + pad
    assert k & (k - 1) == 0 and n < 8192
    c = make_case(name, from_bits(bits, bf16), 1, n, k, largest)
    trace = sweep_trace(case_keys(c), k, bf16)
    if exit_at is None:
        assert len(trace) == d + 3 and [t[0] for t in trace[:d]] == list(target), (name, trace)
        assert not any(t[1] for t in trace[:-1]) and trace[-1][1], (name, trace)
    else:
        assert len(trace) == exit_at + 1 and trace[-1][1] and [t[0] for t in trace] == list(target[: exit_at + 1]), (name, trace)
    c["trace"] = trace
    return c


def digit_edge_cases():
    """Buckets 0 and 255 in every value sweep with all sweeps running, a mid-bucket target with all sweeps running, and the
    early exit in every value sweep; fp32 and bf16, both directions."""
    out = []
    for bf16 in (False, True):
        tag = "bf16" if bf16 else "fp32"
        edges = [(0x00, 0xFF), (0xFF, 0x00)] if bf16 else [(0x00, 0xFF, 0x00, 0xFF), (0xFF, 0x00, 0xFF, 0x00)]
        mid = (0x60, 0x5A) if bf16 else (0x60, 0x5A, 0x33, 0x77)
        for largest in (1, 0):
            for j, t in enumerate(edges + [mid]):
                out.append(digit_edge_case("digits %s largest %d all sweeps %s" % (tag, largest, bytes(t).hex()), bf16, largest,
                                           list(t), None, seed=10 + j))
            for e in range(len(mid)):
                out.append(digit_edge_case("digits %s largest %d exit in sweep %d" % (tag, largest, e), bf16, largest, list(mid), e,
                                           seed=20 + e))
    seen = {(c["dtype"], s, t[0]) for c in out if len(c["trace"]) > 3 for s, t in enumerate(c["trace"][: 2 if c["dtype"] else 4])}
    for dtype, sweeps in ((0, 4), (1, 2)):
        for s in range(sweeps):
            assert (dtype, s, 0) in seen and (dtype, s, 255) in seen
    return out


# ---- (b) tie runs straddling k ---------------------------------------------------------------------------------------------
def tie_run_case(name, bf16, largest, n, run_lo, run_hi, k_at, seed=0):
    """The k-th value is shared by the elements run_lo .. run_hi - 1 and the k-th element is index k_at of that run; a few
    better values are scattered over the row, everything else is worse."""
    gen = torch.Generator().manual_seed(seed)
    sgn = 1.0 if largest else -1.0
    v = -sgn * (2.0 + torch.randint(0, 3, (n,), generator=gen).float())      # worse: three tied levels
    better = torch.randperm(n, generator=gen)[:9]
    better = better[(better < run_lo) | (better >= run_hi)]
    v[better] = sgn * (1.0 + torch.randint(0, 2, (len(better),), generator=gen).float())
    v[run_lo:run_hi] = 0.25 * sgn
    k = len(better) + (k_at - run_lo + 1)
    assert run_lo <= k_at < run_hi - 1 and 1 <= k <= MAX_K      # the run goes on past the k-th element
    c = make_case(name, v.to(BF16) if bf16 else v, 1, n, k, largest)
    ev, ei, ec = expect(c)
    assert int(ec[0]) == k and int(ei[0, k - 1]) == k_at and float(ev[0, k - 1]) == 0.25 * sgn, name
    c["trace"] = sweep_trace(case_keys(c), k, bf16)
    return c


def tie_run_cases():
    out = []
    runs = [("inside one 256-block", 3000, 300, 340, (300, 320, 338)),
            ("across a multiple of 256", 3000, 500, 530, (511, 512, 520)),
            ("across 65536", 70000, 65500, 65600, (65535, 65536, 65580))]
    j = 0
    for what, n, lo, hi, ats in runs:
        assert (what != "inside one 256-block" or lo // 256 == (hi - 1) // 256) and \
               (what != "across a multiple of 256" or (lo // 256 != (hi - 1) // 256 and lo // 65536 == (hi - 1) // 65536)) and \
               (what != "across 65536" or (lo < 65536 < hi and n == 70000))
        for at in ats:
            for bf16 in (False, True):
                largest = (j // 2 + int(bf16)) % 2
                out.append(tie_run_case("tie run %s, k-th at %d, %s, largest %d" % (what, at, "bf16" if bf16 else "fp32", largest),
                                        bf16, largest, n, lo, hi, at, seed=j))
                j += 1
    # how many index sweeps the run needs: all three inside a block, two across a multiple of 256 when the k-th element is
    # the last of its block, one across 65536 likewise
    index_sweeps = {}
    for c in out:
        vs = 2 if c["dtype"] else 4
        index_sweeps.setdefault(len(c["trace"]) - vs, []).append(c["name"])
    assert set(index_sweeps) == {1, 2, 3}, index_sweeps
    return out


ALL_EQUAL_N = 17000
ALL_EQUAL_KS = (1, 255, 256, 257, 4464, 16384)


def all_equal_cases():
    """Rows of one value (bf16 zeros, an fp32 constant, zeros of mixed sign in both types): the answer is 0 .. k - 1 in both
    directions, the value +0.0 for every zero."""
    gen = torch.Generator().manual_seed(5)
    n = ALL_EQUAL_N
    signs = torch.randint(0, 2, (n,), generator=gen)
    mixed = f32_from_bits(signs.numpy().astype(np.uint32) << 31)
    stores = [("bf16 zeros", torch.zeros(n, dtype=BF16)), ("fp32 constant", torch.full((n,), 1.5)),
              ("fp32 zeros of mixed sign", mixed), ("bf16 zeros of mixed sign", mixed.to(BF16))]
    assert int(signs.sum()) not in (0, n) and int((bits_of(stores[3][1]) == 0x8000).sum()) == int(signs.sum())
    out = []
    for what, store in stores:
        for k in ALL_EQUAL_KS:
            for largest in (1, 0):
                c = make_case("all equal, %s, k %d, largest %d" % (what, k, largest), store, 1, n, k, largest)
                ev, ei, ec = expect(c)
                assert torch.equal(ei[0], torch.arange(k, dtype=torch.int32)) and int(ec[0]) == k
                assert bool((ev.view(torch.int32) == (0 if "zeros" in what else f32_from_bits([0x3FC00000]).view(torch.int32))).all())
                out.append(c)
    return out


# ---- (c) value classes -----------------------------------------------------------------------------------------------------
SPECIAL_BITS32 = [0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x00000000, 0x80000000,
                  0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0xFFA50000,
                  0x3F800000, 0xBF800000, 0x00800000, 0x80800000]
SPECIAL_BITS16 = [0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x0001, 0x8001, 0x0000, 0x8000,
                  0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF, 0x7FA0, 0xFFA5,
                  0x3F80, 0xBF80, 0x0080, 0x8080]


def value_class_cases():
    """+-inf, +-max, +-smallest denormal, +-0, NaNs of both signs and several payloads, a few ordinary values; each three times
    (one row of 60) and forty times (2400: more than two blocks of threads), shuffled; unmasked and under a mask that lets some
    of the infinities and NaNs take part and keeps others out; k cuts inside the NaN run, at its end, inside the zeros, and
    takes the whole row."""
    out = []
    for bf16 in (False, True):
        special = SPECIAL_BITS16 if bf16 else SPECIAL_BITS32
        for reps in (3, 40):
            rng = np.random.default_rng(reps + int(bf16))
            bits = np.repeat(np.asarray(special, dtype=np.uint64), reps)
            rng.shuffle(bits)
            n = len(bits)
            store = from_bits(bits, bf16)
            isnan = torch.isnan(store.float())
            nans = int(isnan.sum())
            assert nans == 8 * reps and int(torch.isinf(store.float()).sum()) == 2 * reps
            assert int((bits >> np.uint64(15 if bf16 else 31))[isnan.numpy()].sum()) == 4 * reps    # half the NaNs carry the sign bit
            mask = torch.from_numpy(rng.integers(0, 2, (1, n)).astype(np.int8)) * 3
            for m in (None, mask):
                for largest in (1, 0):
                    if m is not None:
                        # a real infinity of the padding's sign takes part, another one does not; so with the NaNs
                        pad = float("-inf") if largest else float("inf")
                        same = (store.float() == pad).nonzero()[:, 0]
                        m = m.clone()
                        m[0, same[0]], m[0, same[1]] = 3, 0
                        nn = isnan.nonzero()[:, 0]
                        m[0, nn[0]], m[0, nn[1]] = 3, 0
                        assert bool((m[0][store.float() == pad] == 3).any()) and bool((m[0][store.float() == pad] != 3).any())
                    part_nans = nans if m is None else int((isnan & (m[0] == 3)).sum())
                    for k in sorted({1, part_nans - 1, part_nans, part_nans + 1, n // 2, n - 1, n}):
                        out.append(make_case("value classes %s n %d %s largest %d k %d" % (
                            "bf16" if bf16 else "fp32", n, "masked" if m is not None else "unmasked", largest, k),
                            store, 1, n, k, largest, mask=m, mask_value=3))
    return out


# ---- (d) k and n edges -----------------------------------------------------------------------------------------------------
EDGE_KS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 16383, 16384)
EDGE_NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193)


def k_n_edge_cases():
    """Every k of EDGE_KS on every n of EDGE_NS (k < n, k = n and k > n all occur), types and directions alternating: two
    unmasked rows, and three rows under a mask - every element, about half (fewer than k for the larger k), none."""
    out = []
    j = 0
    stores = {}
    for n in EDGE_NS:
        for bf16 in (False, True):
            gen = torch.Generator().manual_seed(n * 2 + int(bf16))
            mask = torch.randint(0, 2, (3, n), generator=gen).to(torch.int8)
            mask[0], mask[2] = 1, 0
            if n > 1:
                mask[1, 0], mask[1, 1] = 1, 0
            stores[n, bf16] = (quantised((3, n), gen, bf16), mask)
    for k in EDGE_KS:
        for n in EDGE_NS:
            bf16, largest = bool(j & 1), (j >> 1) & 1
            j += 1
            store, mask = stores[n, bf16]
            tag = "k %d n %d %s largest %d" % (k, n, "bf16" if bf16 else "fp32", largest)
            out.append(make_case("edges unmasked " + tag, store, 2, n, k, largest))
            out.append(make_case("edges masked " + tag, store, 3, n, k, largest, mask=mask))
    ks_ns = {(c["k"] < c["n"], c["k"] == c["n"], c["k"] > c["n"]) for c in out}
    assert len(ks_ns) == 3
    assert any(c["mask"] is not None and 0 < int((c["mask"][1] == 1).sum()) < c["k"] < c["n"] for c in out)
    for combo in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert any((c["dtype"], c["largest"]) == combo and c["k"] == 16384 for c in out)
    # the optional outputs
    store, mask = stores[1025, False]
    for k in (5, 1025, 2000):
        out.append(make_case("edges no values k %d" % k, store, 3, 1025, k, 1, mask=mask, want_vals=False))
        out.append(make_case("edges no counts k %d" % k, store, 3, 1025, k, 0, mask=mask, want_cnt=False))
    return out


# ---- (e) the (group, pitch) view -------------------------------------------------------------------------------------------
def view_case(name, bf16, largest, group, pitch, nq, rem, offset, k, seed, rows=2):
    """n = nq * group + rem elements per row behind the (group, pitch) view, base pointer `offset` elements into the storage,
    rows pitch-aligned plus two elements apart (so that with offset 0 the first row starts on an 8-byte boundary and the second
    does not).  Everything the view does not address - the columns >= group, the rest of a last partial pixel, the gaps - holds
    decoys that beat every real value: +inf and NaN for descending order, -inf for ascending."""
    gen = torch.Generator().manual_seed(seed)
    n = nq * group + rem
    assert 0 <= rem < group and n >= 1
    span = -(-n // group) * pitch
    row_stride = span + 2
    total = offset + rows * row_stride + 8
    store = torch.full((total,), float("inf") if largest else float("-inf"))
    if largest:
        store[::2] = float("nan")
    real = quantised((rows, n), gen, bf16)
    i = torch.arange(n)
    at = (i // group) * pitch + i % group
    is_real = torch.zeros(total, dtype=torch.bool)
    for r in range(rows):
        store[offset + r * row_stride + at] = real[r].float()
        is_real[offset + r * row_stride + at] = True
    store = store.to(BF16) if bf16 else store
    c = make_case(name, store, rows, n, k, largest, row_stride=row_stride, group=group, pitch=pitch, offset=offset)
    decoys = store[~is_real].float()
    assert int(is_real.sum()) == rows * n and bool(torch.equal(case_rows(c)[:, at].float(), real.float()))
    assert bool((torch.isnan(decoys) | (decoys == float("inf"))).all() if largest else (decoys == float("-inf")).all())
    assert bool(torch.isfinite(real.float()).all()) and len(decoys) >= 8
    c["real"] = real
    return c


VIEW_NQ = (1, 1023, 1025, 4095, 4096, 4097)


def view_cases():
    """bf16: group 1 .. 5 at pitch 8 and 32, pixel counts around one block of threads and around the grouped path's
    4 x 1024 pixels per trip, n a multiple of group and not, base pointer on an 8-byte boundary and one element past it (pairs
    of cases with the same logical rows: the answers must agree).  fp32 with a view on a few of them."""
    out = []
    j = 0
    for group in (1, 2, 3, 4, 5):
        for pitch in (8, 32):
            for nq in VIEW_NQ:
                for rem in ((0,) if group == 1 else (0, group - 1)):
                    largest, k = (j >> 1) & 1, (1, 7, 300, 2 * group)[j % 4]
                    j += 1
                    for offset in (0, 1):
                        out.append(view_case("view bf16 group %d pitch %d nq %d rem %d offset %d largest %d k %d" % (
                            group, pitch, nq, rem, offset, largest, k), True, largest, group, pitch, nq, rem, offset, k, seed=j))
    for group, pitch in ((3, 8), (5, 8), (15, 16), (4, 4)):
        for nq in (1025, 4097):
            largest = (j >> 1) & 1
            j += 1
            for offset in (0, 1):
                out.append(view_case("view fp32 group %d pitch %d nq %d offset %d largest %d" % (group, pitch, nq, offset, largest),
                                     False, largest, group, pitch, nq, 0, offset, 33, seed=j))
    for a, b in zip(out[::2], out[1::2]):        # twins: the same rows, the base pointer aligned and one element further
        assert (a["offset"], b["offset"], a["k"], a["largest"]) == (0, 1, b["k"], b["largest"]) and torch.equal(a["real"], b["real"])
    return out


BIG_VIEWS = ((3, 4, True, 1), (5, 8, True, 0), (15, 16, False, 1))      # (group, pitch, bf16, largest)


def big_view_case(group, pitch, bf16, largest, log2n=24, extra=6):
    """One row of n = 2^log2n - 1 elements (a multiple of 3, 5 and 15 for log2n = 12 and 24) behind a (group, pitch) view:
    a constant background, and distinct better values planted on the first and the last element and on both sides of the
    multiples of `group` next to n / 4, n / 2, 3 n / 4 and n, each pixel next to them carrying a decoy in its first padding column.
    k = planted + extra: the answer is the planted values in order, then the first `extra` background elements - known by
    construction, so nothing long is sorted.  Returns the case with `expect` filled in."""
    n = (1 << log2n) - 1
    assert n % group == 0 and pitch > group
    nq = n // group
    sgn = 1.0 if largest else -1.0
    store = torch.full((nq * pitch,), -4.0 * sgn)
    spots = {0, 1, n - 1, n - 2}
    for centre in (1 << (log2n - 2), 1 << (log2n - 1), 3 << (log2n - 2), n - 4 * group):
        m = centre // group * group
        spots |= {m - group - 1, m - group, m - 1, m, m + 1, m + group - 1, m + group}
    for q in (nq // 3, nq // 3 * 2 + 1):
        spots |= {q * group, q * group + group - 1}
    spots = sorted(spots)
    assert 0 <= spots[0] and spots[-1] == n - 1 and len(spots) >= 24 and extra < spots[2]
    # distinct values, exact in bf16, in an order unrelated to the position; one pair tied to bring the index in
    levels = torch.randperm(len(spots), generator=torch.Generator().manual_seed(group)).tolist()
    assert len(spots) < 64
    levels[3] = levels[5]
    planted = [(sgn * (1.0 + lv * 0.0625), i) for lv, i in zip(levels, spots)]
    for val, i in planted:
        store[(i // group) * pitch + i % group] = val
        store[(i // group) * pitch + group] = sgn * float("inf")          # decoy in the first padding column of that pixel
    planted.sort(key=lambda t: (-sgn * t[0], t[1]))
    k = len(planted) + extra
    background = [i for i in range(extra + 4) if i not in spots][:extra]
    ev = torch.tensor([[p[0] for p in planted] + [-4.0 * sgn] * extra])
    ei = torch.tensor([[p[1] for p in planted] + background], dtype=torch.int32)
    store = store.to(BF16) if bf16 else store
    assert bool(torch.equal(store.float(), store.float().to(BF16).float()))
    return make_case("big view group %d pitch %d %s n 2^%d - 1" % (group, pitch, "bf16" if bf16 else "fp32", log2n), store, 1, n, k,
                     largest, group=group, pitch=pitch, expect=(ev, ei, torch.tensor([k], dtype=torch.int32)))


# ---- (f) carried indices and counts ----------------------------------------------------------------------------------------
def carried_cases():
    gen = torch.Generator().manual_seed(17)
    out = []
    n = 3000
    perm = torch.randperm(n, generator=gen).to(torch.int32)
    perm2 = (torch.randperm(1 << 16, generator=gen)[: 2 * n].reshape(2, n) * 200 + 77).to(torch.int32)   # sparse, up to 1.3e7
    assert bool((perm[1:] < perm[:-1]).any()) and bool((perm[1:] > perm[:-1]).any())
    for bf16 in (False, True):
        v = quantised((2, n), gen, bf16, step=1.0)      # about ten distinct values: the carried index decides nearly everything
        for largest in (1, 0):
            tag = "%s largest %d" % ("bf16" if bf16 else "fp32", largest)
            out.append(make_case("carried permutation " + tag, v, 2, n, 700, largest, idx_in=torch.stack([perm, perm.flip(0)])))
            out.append(make_case("carried sparse indices " + tag, v, 2, n, 257, largest, idx_in=perm2))
    # counts: groups of cnt_group candidates of which only the first cnt are real; the last groups hold 0, 1 and a full count
    for cnt_group, groups in ((64, 40), (1000, 3), (1, 300), (7, 411)):
        n = cnt_group * groups
        cnt = torch.randint(0, cnt_group + 1, (2, groups), generator=gen).to(torch.int32)
        cnt[:, -3], cnt[:, -2], cnt[:, -1] = 0, 1 if cnt_group > 1 else 0, cnt_group
        cnt[1, 0] = cnt_group
        idx = (torch.randperm(1 << 20, generator=gen)[: 2 * n].reshape(2, n)).to(torch.int32)
        for bf16 in (False, True):
            v = quantised((2, n), gen, False, step=1.0)   # the values a merge launch reads are fp32 storage
            for k in (5, cnt_group, min(int(cnt[0].sum()), MAX_K)):
                largest = int(k != 5)
                out.append(make_case("counts group %d x %d %s k %d" % (cnt_group, groups, "as bf16" if bf16 else "fp32", k),
                                     v.to(BF16).float() if bf16 else v, 2, n, k, largest, dtype=2 if bf16 else 0, idx_in=idx, cnt=cnt,
                                     cnt_group=cnt_group))
        out.append(make_case("counts without indices, group %d x %d" % (cnt_group, groups), v, 2, n, 9, 1, cnt=cnt, cnt_group=cnt_group))
    # rows that are segments of a longer row: 2 long rows of 3 segments each
    seg_n = 1500
    v = quantised((6, seg_n), gen, True)
    for largest in (1, 0):
        out.append(make_case("segments of a longer row, largest %d" % largest, v, 6, seg_n, 40, largest, idx_mod=3, idx_mul=seg_n))
    c = out[-1]
    assert int(expect(c)[1].max()) >= 2 * seg_n
    return out


def wide_pairs():
    """fp32 storage of bf16 values read as dtype 2 (two value sweeps) and as dtype 0 (four): the answers must be equal."""
    gen = torch.Generator().manual_seed(23)
    out = []
    for n, k in ((3000, 100), (5000, 4464), (300, 300)):
        v = quantised((2, n), gen, True).float()
        v[0, :8] = f32_from_bits([b << 16 for b in SPECIAL_BITS16[:8]])
        assert bool(((bits_of(v) & 0xFFFF) == 0).all())
        for largest in (1, 0):
            out.append((make_case("wide as dtype 2, n %d largest %d" % (n, largest), v, 2, n, k, largest, dtype=2),
                        make_case("wide as dtype 0, n %d largest %d" % (n, largest), v, 2, n, k, largest, dtype=0)))
    return out


def mixed_launch_cases():
    """Eight segments for ONE launch: k = 2 next to k = 16384 (the survivors' LDS capacity differs per segment), the three
    dtypes, masks, a view, carried indices, and in the middle a segment without rows and one with k = 0."""
    gen = torch.Generator().manual_seed(29)
    v32 = quantised((3, 20000), gen, False)
    v16 = quantised((2, 9000), gen, True)
    mask = torch.randint(0, 2, (3, 20000), generator=gen).to(torch.int8)
    view = view_case("mixed: view", True, 1, 3, 32, 1500, 0, 0, 50, seed=31)
    idx = torch.randperm(9000, generator=gen).to(torch.int32)[None].repeat(2, 1)
    out = [make_case("mixed: k 2", v32, 3, 20000, 2, 1),
           make_case("mixed: k 16384", v32, 3, 20000, 16384, 0, mask=mask),
           make_case("mixed: bf16 k 3", v16, 2, 9000, 3, 0),
           make_case("mixed: no rows", v16, 0, 9000, 5, 1),
           make_case("mixed: k 0", v16, 2, 9000, 0, 1),
           view,
           make_case("mixed: dtype 2 carried k 1000", v16.float(), 2, 9000, 1000, 1, dtype=2, idx_in=idx),
           make_case("mixed: k 2 again", v32, 3, 20000, 2, 0, mask=mask, mask_value=0)]
    assert len(out) == 8 and out[0]["k"] == 2 and out[1]["k"] == 16384
    return out


# ---- (h) the wrapper's two-launch path -------------------------------------------------------------------------------------
def seam_specs():
    """Rows long enough to be cut by layers/select.py (n >= 32768) with the runs that decide the answer laid across the seams
    of the cut: (spec for F.topk_rows, expected segment count).  The row count decides the cut as well (rows * s <= 256)."""
    gen = torch.Generator().manual_seed(37)
    out = []
    n = 32768
    for rows, k, segs, bf16, largest in ((1, 64, 8, False, 1), (40, 64, 4, False, 0), (2, 5000, 2, True, 1), (100, 7, 2, True, 0)):
        sgn = 1.0 if largest else -1.0
        v = quantised((rows, n), gen, False, step=2.0) - 20.0 * sgn            # the crowd: far worse than what follows
        seg_n = n // segs
        for s in range(1, segs):
            seam = s * seg_n
            v[:, seam - 6: seam + 6] = 3.0 * sgn                                # a tie run across every seam
            v[0, seam - 8: seam - 6] = float("nan")                             # NaNs on both sides of a seam, both signs
            v[0, seam + 6] = f32_from_bits([0xFFC00000])[0]
        if rows > 1:
            v[-1, : seg_n] = 3.0 * sgn                                          # a run longer than k inside one segment
        v[0, 5] = -0.0
        mask = None
        if rows == 2:
            mask = (torch.rand((rows, n), generator=gen) > 0.3).to(torch.int8)
            mask[0, seg_n - 3: seg_n + 3] = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.int8)
        v = v.to(BF16) if bf16 else v
        # premise: the k-th element of the first row lies in a run that crosses a seam, or (large k) runs across seams lie above it
        _, ei, _ = R.topk_rows_ref(v[:1], k, bool(largest), mask=None if mask is None else mask[:1])
        picked = set(ei[0].tolist())
        assert any(s * seg_n - 1 in picked and s * seg_n in picked for s in range(1, segs)), (rows, k)
        out.append((dict(vals=v, k=k, largest=bool(largest), mask=mask, mask_value=1), segs))
    # the (3, 32) view of a bf16 map
    hw, a = 11000, 3
    m = quantised((2, hw, 32), gen, True)
    m[..., a:] = float("inf")
    for s in (2 * hw // 8, 5 * hw // 8):                                            # pixels: a tie run of 12 anchors across two seams
        m[:, s - 2: s + 2, :a] = 9.0
    assert hw % 8 == 0
    out.append((dict(vals=m, k=20, largest=True, group=a, pitch=32, n=hw * a), 8))
    return out


# ---- (i) the RPN composition at toy size -----------------------------------------------------------------------------------
RPN_LEVELS = ((13, 21), (7, 11), (4, 6))
RPN_A, RPN_B, RPN_PRE, RPN_POST = 3, 2, 100, 50


def rpn_inputs():
    """Three levels of 32-wide bf16 objectness maps (A = 3 valid columns, +inf decoys behind them) with logits quantised to 1/2,
    the keep mask of the decode step and the alive mask of NMS as fixed pseudo-random functions of the position, and the
    sampler's keys and labels over all anchors."""
    gen = torch.Generator().manual_seed(41)
    maps = []
    for h, w in RPN_LEVELS:
        m = quantised((RPN_B, h * w, 32), gen, True, step=2.0, scale=1.5)
        m[..., RPN_A:] = float("inf")
        maps.append(m)
    ks = [min(h * w * RPN_A, RPN_PRE) for h, w in RPN_LEVELS]
    kmax = max(ks)
    nl = len(RPN_LEVELS)
    keep = (torch.rand((RPN_B * nl, kmax), generator=gen) > 0.2).to(torch.int8)
    for lv, k in enumerate(ks):
        keep[lv::nl, k:] = 0                                                             # row = image * L + level; past a level's k: padding
    alive = (torch.rand((RPN_B * nl, kmax), generator=gen) > 0.4).to(torch.int8)
    anchors = sum(h * w * RPN_A for h, w in RPN_LEVELS)
    keys = torch.rand((RPN_B, anchors), generator=gen).mul(64).floor().div(64)          # tied random keys
    labels = torch.randint(-1, 2, (RPN_B, anchors), generator=gen).to(torch.int8)
    labels[1, 40:] = labels[1, 40:].clamp(max=0)                                         # fewer positives than the draw asks for
    assert ks == [100, 100, 72] and int((labels[1] == 1).sum()) < 24 <= int((labels[0] == 1).sum())
    return dict(maps=maps, ks=ks, kmax=kmax, keep=keep, alive=alive, keys=keys, labels=labels)


def rpn_chain(inp, topk, topk_multi):
    """proposal selection and sampling in the order of modeling/rpn.py, on whatever implementation `topk` / `topk_multi` are
    (F.topk_rows / F.topk_rows_multi on the device, topk_rows_ref here): per-level top-k read from the maps -> scores
    [B * L, kmax] -> masked full sort -> masked top-k over an image's L rows; then the two sampler draws.  Returns every
    intermediate result, on the CPU."""
    dev = inp["maps"][0].device
    b, nl, kmax = RPN_B, len(RPN_LEVELS), inp["kmax"]
    tops = topk_multi([dict(vals=m, k=k, largest=True, group=RPN_A, pitch=32, n=m.shape[1] * RPN_A) for m, k in zip(inp["maps"], inp["ks"])])
    scores = torch.full((b, nl, kmax), float("-inf"), device=dev)
    for lv, (v, _, _) in enumerate(tops):
        scores[:, lv, : v.shape[1]] = v.to(dev)
    scores = scores.reshape(b * nl, kmax).contiguous()
    sv, order, counts = topk(scores, kmax, largest=True, mask=inp["keep"], mask_value=1)
    s_scores = torch.gather(scores, 1, order.to(dev).long()).contiguous()
    post = topk(s_scores.view(b, nl * kmax), RPN_POST, largest=True, mask=inp["alive"].view(b, nl * kmax), mask_value=1, want_vals=False)
    a = inp["keys"].shape[1]
    draws = topk_multi([dict(vals=inp["keys"], k=min(24, a), largest=False, mask=inp["labels"], mask_value=1, want_vals=False),
                        dict(vals=inp["keys"], k=min(48, a), largest=False, mask=inp["labels"], mask_value=0, want_vals=False)])
    res = dict(("level %d" % lv, t) for lv, t in enumerate(tops))
    res.update({"score sort": (sv, order, counts), "post top-k": post, "positive draw": draws[0], "negative draw": draws[1]})
    return dict((name, tuple(None if t is None else t.cpu() for t in r)) for name, r in res.items())


def ref_topk(vals, k, largest=True, mask=None, mask_value=1, group=1, pitch=1, n=None, want_vals=True):
    v, i, c = R.topk_rows_ref(vals, k, largest, mask=mask, mask_value=mask_value, group=group, pitch=pitch, n=n)
    return (v if want_vals else None), i, c


def ref_topk_multi(specs):
    return [ref_topk(**sp) for sp in specs]
