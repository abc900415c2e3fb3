"""The radix-sort cases (tests/sort_cases.py) on the host: every case has the property it is named for, so that none can quietly
stop discriminating, and the numpy expectation is what it claims to be.  No kernel runs here (and none is ever run mutated:
a wrong offset in this sort writes out of bounds)."""
import numpy as np
import pytest

import sort_cases as sc

SMALL_NAMES = [n for n in sc.NAMES if n not in sc.LARGE]


def tagged(tag):
    return [n for n in sc.NAMES if sc.SPECS[n].get(tag) not in (None, False)]


def test_the_matrix_covers_what_it_must():
    specs = sc.SPECS
    assert 140 <= len(sc.NAMES) <= 160, len(sc.NAMES)

    def have(**want):
        return [n for n, s in specs.items() if all(s.get(k, {"start_buf": 0, "digit_bits": 8}.get(k)) == v for k, v in want.items())]

    for n in sc.COUNTS:   # every count, on the multi-pass, the small / dropping and the 9-bit path
        assert have(group="count", n_dev=n, n_bound=n, form="pairs", digit_bits=8)
        assert have(group="count", n_dev=n, n_bound=n, form="depth")
        assert have(group="count", n_dev=n, n_bound=n, digit_bits=9)
    assert set(sc.COUNTS) >= {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 16383, 16384,
                              16385, 20481}
    assert have(n_dev=8388609, end_bit=8, digit_bits=8)
    assert have(n_dev=0, n_bound=5000) and have(n_dev=4097, n_bound=40000)
    over = [s for s in specs.values() if s["n_dev"] == s["n_bound"] + 37]
    assert all(s["n_bound"] >= 1000 for s in over)
    assert {(s["form"], s["n_bound"] <= sc.SMALL_MAX) for s in over} >= {("depth", True), ("depth", False), ("pairs", True)}
    for p in sc.PATTERNS:
        assert have(group="pattern", pattern=p, form="pairs", digit_bits=8) and have(group="pattern", pattern=p, form="depth")
    for e in (1, 7, 8, 9, 12, 16, 17, 24, 30, 32):
        for s in (0, 1):
            assert have(group="passes", end_bit=e, start_buf=s, digit_bits=8)
    for e in (1, 5, 9):
        assert have(group="passes", end_bit=e, digit_bits=9)
    for n in (sc.SMALL_MAX, sc.SMALL_MAX + 1):
        assert len(have(group="drop", n_dev=n)) >= 3
    # the paths: each is reached by many cases
    paths = [sc.path_of(sc.Case(n, None, None, s["n_dev"], s["n_bound"], s["end_bit"], s.get("start_buf", 0), s.get("digit_bits", 8),
                                s["form"], None)) for n, s in specs.items()]
    assert min(paths.count(p) for p in ("small", "multipass", "9bit")) >= 30, {p: paths.count(p) for p in set(paths)}


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_well_formed(name):
    c = sc.build(name)
    n = min(c.n_dev, c.n_bound)
    over = c.n_dev > c.n_bound
    assert c.keys.dtype == np.uint32 and c.keys.size == c.n_bound + (sc.OVER_HEADROOM if over else 0)
    assert c.n_dev <= c.keys.size, "an unclamped kernel would leave the key array"
    assert 1 <= c.end_bit <= 32 and c.start_buf in (0, 1) and c.digit_bits in (8, 9) and c.form in ("pairs", "depth")
    if c.form == "pairs":
        assert c.vals.dtype == np.uint32 and c.vals.shape == c.keys.shape
    else:
        assert c.vals is None and c.end_bit == 32 and c.digit_bits == 8
    if not over:
        assert bool((c.keys[n:] == sc.POISON).all())
    # the sort orders by the digits of its passes, bits [0, passes * digit_bits); the reference by bits [0, end_bit): the bits
    # between are zero in every case, as they are at every call site (region id < 2**16, tile mask from bit 16 up)
    covered = sc.passes_of(c.end_bit, c.digit_bits) * c.digit_bits
    if covered > c.end_bit:
        between = np.uint32(((1 << min(covered, 32)) - 1) ^ ((1 << c.end_bit) - 1))
        assert not bool((c.keys[:n] & between).any())
    if c.meta["group"] == "partition":
        assert bool(((c.keys[:n] >> np.uint32(16)) != 0).all()) and int(c.keys[:n].max()) >= 1 << c.end_bit
    elif c.end_bit < 32:   # the contract's own range
        assert n == 0 or int(c.keys[:n].max()) < 1 << c.end_bit
    if c.digit_bits == 9 and c.meta["group"] != "passes" and c.meta["group"] != "pattern" and n:
        assert int((c.keys[:n] & np.uint32(0xFFFF)).max()) < 510


@pytest.mark.parametrize("name", SMALL_NAMES)
def test_expectation_is_a_stable_sort(name):
    """independent of np.argsort: the expected pairs are a permutation of the input pairs, ordered by the sort key, and pairs
    of equal sort key appear in input order (checked through the input positions, recovered from the pairs themselves)"""
    c = sc.build(name)
    e = sc.expected(c)
    n, m = e["n"], e["n_cmp"]
    mask = np.uint32((1 << c.end_bit) - 1)
    sk = (e["keys"] & mask).astype(np.int64)
    assert bool((np.diff(sk) >= 0).all())
    if c.form == "depth":
        pos = e["vals"].astype(np.int64)
        assert e["n_kept"] == int((c.keys[:n] != sc.ALL_ONES).sum())
        assert np.array_equal(np.sort(pos[:e["n_kept"]]), np.flatnonzero(c.keys[:n] != sc.ALL_ONES))
        assert m == (n if sc.path_of(c) == "small" else e["n_kept"])
        assert np.array_equal(c.keys[pos], e["keys"])
    else:
        assert m == n
        # positions: match (key, value) pairs back to the input by sorting both sides on (key, value, position)
        a = np.lexsort((np.arange(n), c.vals[:n], c.keys[:n]))
        b = np.lexsort((np.arange(n), e["vals"], e["keys"]))
        assert np.array_equal(c.keys[:n][a], e["keys"][b]) and np.array_equal(c.vals[:n][a], e["vals"][b])
        pos = np.empty(n, np.int64)
        pos[b] = a
    same = np.diff(sk) == 0
    assert bool((np.diff(pos)[same] > 0).all()), "equal keys out of input order"
    if "totals" in e:
        assert int(e["totals"].sum()) == n and e["totals"].size == 512


@pytest.mark.parametrize("name", tagged("stable"))
def test_stability_cases_tell_a_tie_reversing_sort_apart(name):
    c = sc.build(name)
    good, bad = sc.expected(c), sc.expected(c, reverse_ties=True)
    assert np.array_equal(good["keys"] & np.uint32((1 << c.end_bit) - 1), bad["keys"] & np.uint32((1 << c.end_bit) - 1))
    assert not np.array_equal(good["vals"], bad["vals"])


def test_there_are_stability_cases_on_every_path():
    paths = {sc.path_of(sc.build(n)) for n in tagged("stable") if n not in sc.LARGE}
    assert paths == {"small", "multipass", "9bit"}


def multipass_names():
    return [n for n in sc.NAMES if sc.SPECS[n]["pattern"] in ("uniform", "depthlike") and sc.SPECS[n].get("digit_bits", 8) == 8
            and min(sc.SPECS[n]["n_dev"], sc.SPECS[n]["n_bound"]) >= 16 and sc.SPECS[n].get("n_kept") != 0]


@pytest.mark.parametrize("name", multipass_names())
def test_every_pass_of_a_multipass_case_decides_some_pair(name):
    """for every pass, two keys differ in that pass's digit and in no lower one: counted as distinct values of the key's low
    8 (p + 1) bits against distinct values of its low 8 p bits"""
    c = sc.build(name)
    assert c.meta.get("multipass") is True
    n = min(c.n_dev, c.n_bound)
    k = c.keys[:n]
    if c.form == "depth":
        k = k[k != sc.ALL_ONES]
    assert k.size >= 2
    npass = sc.passes_of(c.end_bit)
    for p in range(npass):
        lo = np.uint32((1 << (8 * p)) - 1)
        hi = np.uint32((1 << min(8 * (p + 1), 32)) - 1)
        groups = np.unique(k & lo).size
        finer = np.unique(k & hi).size
        assert finer > groups, "pass %d decides nothing" % p
    grp = c.meta["group"]
    assert grp != "passes" or npass == (c.end_bit + 7) // 8


def test_multipass_cases_include_every_pass_count_and_path():
    got = {(sc.passes_of(sc.SPECS[n]["end_bit"]), sc.SPECS[n]["form"]) for n in multipass_names()}
    assert got >= {(1, "pairs"), (2, "pairs"), (3, "pairs"), (4, "pairs"), (4, "depth")}


def test_the_2049_tile_case_reaches_the_second_rowscan_chunk():
    c = sc.build("tiles_2049")
    n = min(c.n_dev, c.n_bound)
    tiles = -(-n // sc.TILE)
    assert tiles == 2049 > sc.ROWSCAN_CHUNK and sc.passes_of(c.end_bit) == 1
    d = (c.keys[:n] & np.uint32(0xFF)).astype(np.int64)
    late = d[sc.ROWSCAN_CHUNK * sc.TILE:]
    assert late.size >= 1                                     # some digit has a count in a tile of index >= 2048 ...
    before = np.bincount(d[:sc.ROWSCAN_CHUNK * sc.TILE], minlength=256)
    assert int(before[late[0]]) > 0                           # ... whose offset there is the first chunk's carry
    e = sc.expected(c)
    assert bool((np.diff(e["keys"].astype(np.int64)) >= 0).all()) and e["n_cmp"] == n
    assert not np.array_equal(e["vals"], sc.expected(c, reverse_ties=True)["vals"])


@pytest.mark.parametrize("name", tagged("tile_edge"))
def test_tile_edge_cases_sit_on_a_tile_edge(name):
    c = sc.build(name)
    n = min(c.n_dev, c.n_bound)
    r = n % sc.TILE
    assert n >= sc.TILE - 1 and r in (0, 1, sc.TILE - 1), n


def test_tile_edges_are_met_from_both_sides():
    ns = {min(sc.SPECS[n]["n_dev"], sc.SPECS[n]["n_bound"]) for n in tagged("tile_edge")}
    assert ns >= {4095, 4096, 4097, 8192, 16383, 16384, 16385, 20481}


@pytest.mark.parametrize("name", [n for n in sc.NAMES if "n_kept" in sc.SPECS[n]])
def test_drop_cases_keep_what_they_say(name):
    c = sc.build(name)
    e = sc.expected(c)
    assert c.form == "depth" and e["n_kept"] == c.meta["n_kept"]
    if "drop_tile" in c.meta:   # the all-ones keys fill exactly that tile (or what the count leaves of it)
        n = min(c.n_dev, c.n_bound)
        t = c.meta["drop_tile"]
        gone = np.flatnonzero(c.keys[:n] == sc.ALL_ONES)
        assert np.array_equal(gone, np.arange(t * sc.TILE, min((t + 1) * sc.TILE, n)))


def test_drop_shares_on_both_sides_of_the_switch():
    for n in (sc.SMALL_MAX, sc.SMALL_MAX + 1):
        path = "small" if n <= sc.SMALL_MAX else "multipass"
        for tag, lo, hi in (("0", 1.0, 1.0), ("80", 0.17, 0.23), ("100", 0.0, 0.0)):
            c = sc.build("drop_%s_%d" % (tag, n))
            assert sc.path_of(c) == path
            assert lo <= sc.expected(c)["n_kept"] / n <= hi


def test_pattern_cases_are_what_they_are_named():
    for form in ("pairs", "depth_multi"):
        def k(p):
            c = sc.build("pattern_%s_%s" % (form, p))
            return c.keys[:c.n_bound]
        assert int(k("zeros").max()) == 0 and int(k("allmax").min()) == sc.ALL_ONES
        assert np.unique(k("alternating")).size == 2 and bool((k("alternating")[::2] != k("alternating")[1::2]).all())
        assert bool((np.diff(k("ascending").astype(np.int64)) > 0).all())
        assert bool((np.diff(k("descending").astype(np.int64)) < 0).all())
        for byte in range(4):
            cnt = np.bincount(((k("equal_digits") >> np.uint32(8 * byte)) & np.uint32(0xFF)).astype(np.int64), minlength=256)
            assert int(cnt.min()) == int(cnt.max()) == k("equal_digits").size // 256
        top = np.unique(k("depthlike") >> np.uint32(24))
        assert 2 <= top.size <= 8, top
    k9 = sc.build("pattern_9bit_equal_digits")
    cnt = np.bincount(k9.keys[:k9.n_bound].astype(np.int64), minlength=512)
    assert int(cnt.min()) == int(cnt.max()) == k9.n_bound // 512
    c = sc.build("pattern_one_tile_equal")
    assert np.unique(c.keys[sc.TILE:2 * sc.TILE]).size == 1 and np.unique(c.keys[:sc.TILE]).size > 4000


def test_values_are_payload():
    c = sc.build("count_pairs_4097")
    v = c.vals[:c.n_bound]
    assert int((v == sc.ALL_ONES).sum()) >= 2 and int((v == 0).sum()) >= 1
    assert not np.array_equal(np.sort(v), np.arange(v.size))


def test_final_half_rule():
    for name, want in (("passes_e8_s0", 1), ("passes_e8_s1", 0), ("passes_e16_s0", 0), ("passes_e17_s0", 1), ("passes_e17_s1", 0),
                       ("passes_e32_s0", 0), ("passes_e32_s1", 1), ("passes_9bit_e9_s0", 1), ("passes_9bit_e1_s1", 0),
                       ("count_depth_4096", 0)):
        assert sc.final_half(sc.build(name)) == want, name


@pytest.mark.parametrize("name", [c[0] for c in sc.SCAN_CASES])
def test_scan_cases(name):
    buf, exp = sc.scan_case(name)
    nb = buf.size - 1
    assert exp[0] == 0 and int(exp[nb]) == int(buf[:nb].astype(np.uint64).sum()) and int(exp[nb]) < 1 << 32
    assert bool((buf[:nb] < (1 << 16)).all()) or 1 << 31 < int(exp[nb]) < 1 << 32
    if "2p31" in name:
        assert 1 << 31 < int(exp[nb]) < 1 << 32
    assert buf[nb] == sc.POISON


def test_scan_sizes():
    assert {c[1] for c in sc.SCAN_CASES} == {1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 5000}
