"""Named cases for the stable LSD radix sort of (u32 key, u32 value) pairs and the one-workgroup scan of csrc/gs_binning.hip
(rs_hist_kernel, rs_rowscan_kernel, rs_scatter_kernel, rs_small_sort_kernel, scan_sums_kernel), with their expected outputs
from numpy alone.  tests/test_sort_cases_cpu.py shows that every case has the property it is named for;
tests/test_gpu_sort.py runs them through gs_debug_sort_pairs / gs_debug_scan_sums and compares exactly.

THE OPERATION.  n = min(n_dev, n_bound) pairs are ordered stably by the key's bits [0, end_bit): 8-bit passes
(ceil(end_bit / 8) of them), or ONE 9-bit pass (digit_bits = 9, end_bit <= 9) after which the 512 digit totals are the
numbers of keys per digit.  The result lies in half start_buf ^ (passes & 1) of the ping-pong buffers (start_buf ^ 1 after the
9-bit pass).  Two forms:
  "pairs": keys and values are given; whole keys and values travel together.
  "depth": the first pass reads the keys from a buffer of the caller's that stays intact, value = index, keys 0xFFFFFFFF are
           dropped and n_kept is the number of the others.  Up to 16 384 keys one workgroup sorts everything (the dropped keys
           land at the tail, n_kept does not count them); beyond, the first pass filters and only the first n_kept outputs
           are specified.

THE REFERENCE.  order = np.argsort(keys[:n] & (2**end_bit - 1), kind="stable"); expected keys = keys[:n][order], expected
values = vals[:n][order] ("pairs") or order itself ("depth", over the survivors).  For keys below 2**end_bit this is
np.argsort(keys[:n], kind="stable").

WHAT THE CALLERS HAND THE SORT (read at the four call sites):
  * depth order (gs_api.hip, forward_bin_stage): end_bit 32, any 32-bit key - below 2**end_bit trivially;
  * Morton sort (gs_knn.hip): end_bit 32, 30-bit codes - below 2**end_bit;
  * slot sort (gs_encoding.hip): end_bit = bit length of n_slots, keys are slots < n_slots or the sentinel n_slots itself -
    below 2**end_bit;
  * region partition (gs_tilebin.hip): end_bit = bits of the region count, but key = region id | tile mask << 16: the region id
    is below 2**end_bit, the KEY IS NOT.  The partition relies on the sort ordering by the low end_bit bits only and carrying
    the bits above them along untouched (and on the 9-bit pass counting digits of key & 511).
So "keys below 2**end_bit" holds for three callers out of four.  The cases the sort's contract is stated on keep their keys
below 2**end_bit; the group "partition" adds keys with a 16-bit mask above bit 16, as tb_emit_kernel writes them, for which
only the masked reference above is right.

Key and value arrays hold n_bound words; words [n, n_bound) of the inputs are POISON, as are the workspace and the outputs
before the call, so "nothing is written past the count" can be asserted in either final half.  The over-count cases (n_dev =
n_bound + 37) carry OVER_HEADROOM more valid random words behind n_bound: a kernel that failed to clamp would read them - and
sort them in, which the comparison sees - without leaving the allocation."""
import functools
import zlib
from collections import namedtuple

import numpy as np

POISON = 0xA5A5A5A5
ALL_ONES = 0xFFFFFFFF
TILE = 4096            # keys per workgroup of the multi-pass kernels (RS_TILE)
SMALL_MAX = 16384      # the one-workgroup sort takes the depth form up to here (RS_SMALL_MAX)
ROWSCAN_CHUNK = 2048   # tiles per loop trip of rs_rowscan_kernel (GS_BLOCK * 8)
OVER = 37
OVER_HEADROOM = 8192   # words of valid keys behind n_bound in the over-count cases
GS_E_SHAPE = -2

Case = namedtuple("Case", "name keys vals n_dev n_bound end_bit start_buf digit_bits form meta")
# keys: uint32 [n_bound (+ OVER_HEADROOM)]; vals: the same shape, or None in the depth form
# meta: group, and the properties tests/test_sort_cases_cpu.py verifies: "stable" (ties whose order shows), "multipass"
# (every pass decides the order of some pair), "tile_edge", "n_kept", "drop_tile"

COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 20481)
BIG_N = 8388609        # 2049 tiles: the second trip of rs_rowscan_kernel's loop
END_BITS = (1, 7, 8, 9, 12, 16, 17, 24, 30, 32)
PATTERNS = ("uniform", "zeros", "allmax", "alternating", "ascending", "descending", "equal_digits", "depthlike")


def passes_of(end_bit, digit_bits=8):
    return 1 if digit_bits == 9 else (end_bit + 7) // 8


def final_half(case):
    """the half of the ping-pong buffers the callers read after the sort"""
    return case.start_buf ^ (1 if case.digit_bits == 9 else (passes_of(case.end_bit) & 1))


def path_of(case):
    """which kernels the case reaches"""
    if case.form == "depth" and case.n_bound <= SMALL_MAX:
        return "small"
    return "9bit" if case.digit_bits == 9 else "multipass"


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _mask(end_bit):
    return np.uint32((1 << end_bit) - 1)


def pattern_keys(pattern, n, end_bit, rng):
    top = (1 << end_bit) - 1
    if pattern == "uniform":
        k = rng.randint(0, 1 << 32, size=n, dtype=np.uint64) & top
    elif pattern == "zeros":
        k = np.zeros(n, np.uint64)
    elif pattern == "allmax":
        k = np.full(n, top, np.uint64)
    elif pattern == "alternating":   # two values that differ in every byte they have
        a, b = 0x5A3C96E1 & top, 0xA5C3691E & top
        k = np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint64)
    elif pattern in ("ascending", "descending"):   # monotone with ties where n > 2**end_bit
        k = (np.arange(n, dtype=np.uint64) * np.uint64(top)) // np.uint64(max(n - 1, 1))
        if pattern == "descending":
            k = k[::-1]
    elif pattern == "equal_digits":   # every digit value (as) equally often (as n allows) in every byte, independently
        k = np.zeros(n, np.uint64)
        for byte in range(4):
            k |= rng.permutation(np.arange(n, dtype=np.uint64) % 256) << np.uint64(8 * byte)
        if end_bit == 9:   # the 9-bit pass: every one of the 512 digits equally often
            k = rng.permutation(np.arange(n, dtype=np.uint64) % 512)
        k &= top
    elif pattern == "depthlike":      # float32 bit patterns of view depths: a handful of values in the high byte
        k = rng.uniform(0.2, 100.0, size=n).astype(np.float32).view(np.uint32).astype(np.uint64) & top
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(k).astype(np.uint32)


def plant_pass_pairs(keys, where, end_bit, rng):
    """for every 8-bit pass, two keys (at positions out of `where`) that differ in that pass's digit alone: the pass decides
    their order, no lower one does"""
    npass = passes_of(end_bit)
    if where.size < 2 * npass + 2:
        return False
    pos = rng.permutation(where)[:2 * npass]
    for p in range(npass):
        i, j = pos[2 * p], pos[2 * p + 1]
        keys[j] = keys[i] ^ np.uint32(1 << (8 * p))
    return True


def _arbitrary_vals(n, rng):
    """values are payload, not a permutation: any u32, the all-ones word and zero among them"""
    v = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if n:
        v[0] = ALL_ONES
        v[n // 2] = 0
        v[n - 1] = ALL_ONES
    return v


def _make(name, group, form, pattern, n_dev, n_bound, end_bit, start_buf=0, digit_bits=8, drop=None, high_bits=False,
          below=None, **meta):
    """drop: share of all-ones keys (depth form), or ("first" | "last", count) for a run of them;
    high_bits: a random non-zero 16-bit mask above bit 16, as the region partition's keys carry;
    below: keys are taken modulo this (510 regions at 1080p)"""
    rng = _rng(name)
    n = min(n_dev, n_bound)
    over = n_dev > n_bound
    valid = n_bound + OVER_HEADROOM if over else n   # words that hold real keys
    keys = pattern_keys(pattern, valid, end_bit, rng)
    if below is not None:
        keys = (keys % np.uint32(below)).astype(np.uint32)
    meta = dict(meta, group=group, pattern=pattern)
    equal_tile = meta.get("equal_tile")
    if equal_tile is not None:
        keys[equal_tile * TILE:(equal_tile + 1) * TILE] = 0x12345678
    if high_bits:
        keys |= rng.randint(1, 1 << 16, size=valid).astype(np.uint32) << np.uint32(16)
    if form == "depth" and drop is not None:
        if isinstance(drop, tuple):
            where, cnt = drop
            sel = np.zeros(valid, bool)
            if where == "first":
                sel[:cnt] = True
            else:
                sel[n - cnt:n] = True
            keys[keys == ALL_ONES] = ALL_ONES - 1   # (the run is the only all-ones keys)
        else:
            sel = rng.random_sample(valid) < drop if 0.0 < drop < 1.0 else np.full(valid, drop >= 1.0)
        keys[sel] = ALL_ONES
    if pattern in ("uniform", "depthlike") and digit_bits == 8:
        free = np.ones(n, bool)   # where a planted key disturbs nothing the case is named for
        if form == "depth":
            free &= keys[:n] != ALL_ONES
        if equal_tile is not None:
            free[equal_tile * TILE:(equal_tile + 1) * TILE] = False
        if plant_pass_pairs(keys, np.flatnonzero(free), end_bit, rng):
            meta["multipass"] = True
    size =n_bound + (OVER_HEADROOM if over else 0)
    kbuf = np.full(size, POISON, np.uint32)
    kbuf[:valid] = keys
    vbuf = None
    if form == "pairs":
        vbuf = np.full(size, POISON, np.uint32)
        vbuf[:valid] = _arbitrary_vals(valid, rng)
    return Case(name, kbuf, vbuf, n_dev, n_bound, end_bit, start_buf, digit_bits, form, meta)


# ---- the matrix: name -> keyword arguments of _make ----------------------------------------------------------------------
SPECS = {}


def _spec(name, **kw):
    assert name not in SPECS, name
    SPECS[name] = kw


for _n in COUNTS:
    _edge = dict(tile_edge=True) if _n >= TILE - 1 and min(_n % TILE, TILE - _n % TILE) <= 1 else {}
    # 32-bit uniform pairs: the multi-pass kernels at every per-wave slice (256 / 512 / 1024 keys) and tile edge
    _spec("count_pairs_%d" % _n, group="count", form="pairs", pattern="uniform", n_dev=_n, n_bound=_n, end_bit=32, **_edge)
    # depth form, 30 % dropped: the one-workgroup sort up to 16 384, the filtering first pass beyond
    _spec("count_depth_%d" % _n, group="count", form="depth", pattern="depthlike", n_dev=_n, n_bound=_n, end_bit=32, drop=0.3,
          **_edge)
    # the 9-bit one-pass form, keys below 510 as at 1080p: ties everywhere (stability), digit totals = region counts
    _spec("count_9bit_%d" % _n, group="count", form="pairs", pattern="uniform", n_dev=_n, n_bound=_n, end_bit=9, digit_bits=9,
          below=510, stable=_n > 510, **_edge)

# 2049 tiles in a single 8-bit pass: the second trip of rs_rowscan_kernel's loop carries the first trip's row sums
_spec("tiles_2049", group="big", form="pairs", pattern="uniform", n_dev=BIG_N, n_bound=BIG_N, end_bit=8, stable=True, tile_edge=True)

# count against bound  (bound_zero_depth_multi: with no key at all the first pass must still store n_kept = 0 - the later
# passes take it for their count; rs_scatter_kernel used to return before the store and leave whatever the word held)
_spec("bound_zero_pairs", group="bound", form="pairs", pattern="uniform", n_dev=0, n_bound=5000, end_bit=16)
_spec("bound_zero_9bit", group="bound", form="pairs", pattern="uniform", n_dev=0, n_bound=5000, end_bit=9, digit_bits=9)
_spec("bound_zero_depth_small", group="bound", form="depth", pattern="depthlike", n_dev=0, n_bound=5000, end_bit=32, n_kept=0)
_spec("bound_zero_depth_multi", group="bound", form="depth", pattern="depthlike", n_dev=0, n_bound=20000, end_bit=32, n_kept=0)
_spec("bound_far_pairs", group="bound", form="pairs", pattern="uniform", n_dev=4097, n_bound=40000, end_bit=16, start_buf=1,
      tile_edge=True)
_spec("bound_far_9bit", group="bound", form="pairs", pattern="uniform", n_dev=4097, n_bound=40000, end_bit=9, digit_bits=9,
      below=510, stable=True, tile_edge=True)
_spec("bound_far_depth", group="bound", form="depth", pattern="depthlike", n_dev=4097, n_bound=40000, end_bit=32, drop=0.3,
      tile_edge=True)
_spec("over_depth_small_1000", group="over", form="depth", pattern="depthlike", n_dev=1000 + OVER, n_bound=1000, end_bit=32, drop=0.3)
_spec("over_depth_small_16384", group="over", form="depth", pattern="depthlike", n_dev=16384 + OVER, n_bound=16384, end_bit=32, drop=0.3)
_spec("over_depth_multi_20481", group="over", form="depth", pattern="depthlike", n_dev=20481 + OVER, n_bound=20481, end_bit=32, drop=0.3)
_spec("over_pairs_1000", group="over", form="pairs", pattern="uniform", n_dev=1000 + OVER, n_bound=1000, end_bit=32)
_spec("over_pairs_4096", group="over", form="pairs", pattern="uniform", n_dev=4096 + OVER, n_bound=4096, end_bit=16)

# key patterns on the three paths and the 9-bit form; counts are multiples of 256 / 512 (equal_digits is then exactly equal)
# that end a quarter-slice into a further tile
for _p in PATTERNS:
    _ties = _p in ("zeros", "allmax", "alternating")
    _spec("pattern_pairs_%s" % _p, group="pattern", form="pairs", pattern=_p, n_dev=20736, n_bound=20736, end_bit=32, stable=_ties)
    _spec("pattern_depth_small_%s" % _p, group="pattern", form="depth", pattern=_p, n_dev=4352, n_bound=4352, end_bit=32,
          stable=_p in ("zeros", "alternating"), **(dict(n_kept=0) if _p == "allmax" else {}))
    _spec("pattern_depth_multi_%s" % _p, group="pattern", form="depth", pattern=_p, n_dev=20736, n_bound=20736, end_bit=32,
          stable=_p in ("zeros", "alternating"), **(dict(n_kept=0) if _p == "allmax" else {}))
    _spec("pattern_9bit_%s" % _p, group="pattern", form="pairs", pattern=_p, n_dev=8704, n_bound=8704, end_bit=9, digit_bits=9,
          stable=True)
# one tile of 4096 equal keys between two random ones
_spec("pattern_one_tile_equal", group="pattern", form="pairs", pattern="uniform", n_dev=3 * TILE, n_bound=3 * TILE, end_bit=32,
      equal_tile=1, stable=True, tile_edge=True)

# pass structure: 1 .. 4 passes, whole and partial top digits, both start halves
for _e in END_BITS:
    for _s in (0, 1):
        _spec("passes_e%d_s%d" % (_e, _s), group="passes", form="pairs", pattern="uniform", n_dev=9001, n_bound=9001, end_bit=_e,
              start_buf=_s, stable=_e <= 12)
for _e in (1, 5, 9):
    for _s in (0, 1):
        _spec("passes_9bit_e%d_s%d" % (_e, _s), group="passes", form="pairs", pattern="uniform", n_dev=9001, n_bound=9001,
              end_bit=_e, start_buf=_s, digit_bits=9, stable=True)

# keys as the region partition writes them: region id below 2**end_bit, a tile mask above bit 16 that must travel along
_spec("partition_e7", group="partition", form="pairs", pattern="uniform", n_dev=9001, n_bound=12000, end_bit=7, high_bits=True, stable=True)
_spec("partition_9bit", group="partition", form="pairs", pattern="uniform", n_dev=9001, n_bound=12000, end_bit=9, digit_bits=9,
      below=510, high_bits=True, stable=True)
_spec("partition_e11_s1", group="partition", form="pairs", pattern="uniform", n_dev=9001, n_bound=12000, end_bit=11, start_buf=1,
      high_bits=True, stable=True)

# the depth form on both sides of the one-workgroup / multi-pass switch
for _n in (SMALL_MAX, SMALL_MAX + 1):
    for _share, _tag in ((0.0, "0"), (0.8, "80"), (1.0, "100")):
        _spec("drop_%s_%d" % (_tag, _n), group="drop", form="depth", pattern="depthlike", n_dev=_n, n_bound=_n, end_bit=32,
              drop=_share, **(dict(n_kept=_n) if _share == 0.0 else dict(n_kept=0) if _share == 1.0 else {}))
_spec("drop_first_tile_16384", group="drop", form="depth", pattern="depthlike", n_dev=SMALL_MAX, n_bound=SMALL_MAX, end_bit=32,
      drop=("first", TILE), n_kept=SMALL_MAX - TILE, drop_tile=0)
_spec("drop_last_tile_16384", group="drop", form="depth", pattern="depthlike", n_dev=SMALL_MAX, n_bound=SMALL_MAX, end_bit=32,
      drop=("last", TILE), n_kept=SMALL_MAX - TILE, drop_tile=3)
_spec("drop_first_tile_20481", group="drop", form="depth", pattern="depthlike", n_dev=20481, n_bound=20481, end_bit=32,
      drop=("first", TILE), n_kept=20481 - TILE, drop_tile=0)
_spec("drop_last_tile_20480", group="drop", form="depth", pattern="depthlike", n_dev=5 * TILE, n_bound=5 * TILE, end_bit=32,
      drop=("last", TILE), n_kept=4 * TILE, drop_tile=4)
_spec("drop_last_tile_20481", group="drop", form="depth", pattern="depthlike", n_dev=20481, n_bound=20481, end_bit=32,
      drop=("last", 1), n_kept=20480, drop_tile=5)

NAMES = list(SPECS)
LARGE = ("tiles_2049",)


@functools.lru_cache(maxsize=8)
def build(name):
    case = _make(name, **SPECS[name])
    for a in (case.keys, case.vals):
        if a is not None:
            a.setflags(write=False)
    return case


def sort_key(case, keys):
    """the bits the sort orders by, in the narrowest type (numpy's stable sort of 8- and 16-bit integers is a radix sort)"""
    k = keys & _mask(case.end_bit)
    return k.astype(np.uint8) if case.end_bit <= 8 else k.astype(np.uint16) if case.end_bit <= 16 else k


def expected(case, reverse_ties=False):
    """dict: n, n_cmp (leading outputs that are specified), keys / vals [n_cmp], n_kept (depth form), totals (9-bit form).
    reverse_ties: the order a sort would give that reverses equal keys (to show that a case tells the two apart)."""
    n = min(case.n_dev, case.n_bound)
    k = case.keys[:n]
    out = dict(n=n)

    def order_of(sk):
        if reverse_ties:
            return len(sk) - 1 - np.argsort(sk[::-1], kind="stable")
        return np.argsort(sk, kind="stable")

    if case.form == "pairs":
        order = order_of(sort_key(case, k))
        out.update(n_cmp=n, keys=k[order], vals=case.vals[:n][order])
        if case.digit_bits == 9:
            out["totals"] = np.bincount((k & np.uint32(511)).astype(np.int64), minlength=512).astype(np.uint32)
        return out
    surv = np.flatnonzero(k != ALL_ONES)
    order = surv[order_of(k[surv])]
    out["n_kept"] = int(surv.size)
    if path_of(case) == "small":   # the dropped keys are sorted along, to the tail, in index order
        dropped = np.flatnonzero(k == ALL_ONES)
        order = np.concatenate([order, dropped[::-1] if reverse_ties else dropped])
    out.update(n_cmp=int(order.size), keys=k[order], vals=order.astype(np.uint32))
    return out


# ---- scan_sums_kernel: in-place exclusive scan of sums[0, nb), total at sums[nb] ----
SCAN_NB = (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 5000)
SCAN_CASES = [("nb%d" % nb, nb, False) for nb in SCAN_NB] + [("nb5000_total_above_2p31", 5000, True)]


def scan_case(name):
    """(input [nb + 1] uint32 with POISON in the total's slot, expected [nb + 1] uint64)"""
    _, nb, big = next(c for c in SCAN_CASES if c[0] == name)
    rng = _rng("scan_" + name)
    v = rng.randint(500000, 700000, size=nb) if big else rng.randint(0, 1 << 16, size=nb)
    buf = np.full(nb + 1, POISON, np.uint32)
    buf[:nb] = v
    exp = np.zeros(nb + 1, np.uint64)
    exp[1:] = np.cumsum(v.astype(np.uint64))
    return buf, exp
