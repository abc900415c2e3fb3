"""tests/encoding_cases.py checks itself, without a GPU: the exact cases reach every path of the segmented reduction and are
exact in any summation order, a dropped / doubled / misplaced entry changes the expected bits, the fp32 restatement stays
inside every derived bar, and the pass-count cases take 1, 2, 2, 3 and 4 sort passes."""
import numpy as np
import pytest
import torch

import encoding_cases as ec
import encoding_reference as ref


def test_segment_class_on_hand_made_segments():
    assert ec.segment_class(0, 1) == ("inside",) and ec.segment_class(256, 300) == ("inside",)
    assert ec.segment_class(10, 256) == ("inside",)                      # ends on a boundary, no whole chunk
    assert ec.segment_class(255, 257) == ("straddle",) and ec.segment_class(1, 511) == ("straddle",)
    assert ec.segment_class(256, 512) == ("one_chunk",)
    assert ec.segment_class(200, 512) == ("head_chunks",) and ec.segment_class(512, 800) == ("chunks_tail",)
    assert ec.segment_class(200, 513) == ("head_chunks_tail",)
    assert ec.segment_class(0, 512) == ("multi_chunk",)
    assert ec.segment_class(1, 770) == ("head_chunks_tail", "multi_chunk")
    assert ec.segment_class(0, 700) == ("chunks_tail", "multi_chunk")
    assert ec.segment_classes([0, 256], [256, 300]) == dict(dict.fromkeys(ec.CLASSES, 0), one_chunk=1, inside=1)


def test_layout_is_emit_plus_stable_sort():
    """Two points in one cell and one outside, L = 1, D = 2: entry e = (b << 2) + corner, equal keys keep emission order."""
    x = torch.tensor([[0.3, 0.6], [1.5, 0.5], [0.3, 0.6]])
    offs = ref.grid_offsets(2, 1, 2.0, 5, 19, True)
    lay = ec.layout(x, offs, 2.0, 5, 1, True)
    assert lay.N == 12 and lay.keys.tolist()[4:8] == [offs[-1]] * 4
    assert lay.slot.tolist() == [11, 12, 16, 17] and lay.lo.tolist() == [0, 2, 4, 6] and lay.hi.tolist() == [2, 4, 6, 8]
    assert lay.order.tolist() == [0, 8, 1, 9, 2, 10, 3, 11, 4, 5, 6, 7]


def test_exact_cases_reach_every_segment_class():
    total = dict.fromkeys(ec.CLASSES, 0)
    for name in ec.EXACT:
        for k, n in ec.exact_classes(name).items():
            total[k] += n
    assert all(total[k] > 0 for k in ec.CLASSES), total
    # ... and every class is named by the id of a case that reaches it
    ids = [ec.exact_id(n) for n in ec.EXACT]
    for k in ec.CLASSES:
        assert any(k in i.split("-")[-1].split("+") for i in ids), k


@pytest.mark.parametrize("C", (1, 2, 4, 8))
def test_each_channel_count_sees_whole_chunks(C):
    seen = dict.fromkeys(ec.CLASSES, 0)
    for name, case in ec.EXACT.items():
        if case.C == C:
            for k, n in ec.exact_classes(name).items():
                seen[k] += n
    assert seen["multi_chunk"] > 0 and seen["one_chunk"] > 0 and seen["head_chunks_tail"] > 0, seen


def test_sentinel_variant_shares_the_last_real_chunk():
    shared = []
    for name, case in ec.EXACT.items():
        if case.variant != "sentinel":
            continue
        t, lay, _ = ec.exact_expectation(name)
        n_real = int(lay.hi.max())
        assert lay.N > n_real and int((lay.keys == t.offsets[-1]).sum()) == lay.N - n_real
        # interleaved: an outside point sits between inside points
        inside = ~((t.x < 0) | (t.x > 1)).any(dim=1)
        assert bool((~inside[:-1] & inside[1:]).any()) or t.x.shape[0] == 2
        if n_real % ec.CHUNK:
            shared.append(name)
    assert any(n.startswith("g700-") for n in shared) and any(n.startswith("g100_412_300-") for n in shared), shared


def test_hash_variant_is_hashed_and_noac_is_shifted():
    t, _, _ = ec.exact_expectation("g700-C4-hash")
    assert t.gridtype == 0 and t.offsets == [0, 16] and 5 * 5 > 16
    t, lay, _ = ec.exact_expectation("g64_192_256-C2-noac")
    assert not t.align and torch.equal(t.x[0], torch.tensor([(1 - 0.25) / 4, 0.0]))
    assert lay.slot.tolist() == sorted({i + di + 6 * (j + dj) for (i, j) in ec.EXACT_CELLS[:3] for di in (0, 1) for dj in (0, 1)})


def _is_exact(v64, step=8.0):
    scaled = v64 * step
    return bool((scaled == scaled.round()).all()) and float(scaled.abs().max()) < 2 ** 24 \
        and torch.equal(v64.float().double(), v64)


@pytest.mark.parametrize("name", list(ec.EXACT), ids=[ec.exact_id(n) for n in ec.EXACT])
def test_exact_case_is_exact_in_any_order(name):
    t, lay, (out, gemb, gin) = ec.exact_expectation(name)
    assert float(t.emb.abs().max()) < 64 and float(t.g.abs().max()) < 64 and float(t.g.abs().min()) >= 1
    _, w = ec.entries(t.x, t.offsets, t.pls, t.H, t.gridtype, t.align)
    inside = ~((t.x < 0) | (t.x > 1)).any(dim=1)
    assert torch.equal(w[inside], torch.tensor([0.375, 0.125, 0.375, 0.125], dtype=torch.float64).expand(int(inside.sum()), 1, 4))
    assert _is_exact(out) and _is_exact(gemb) and _is_exact(gin, 1.0)
    c32 = ec.sorted_contributions(t, lay)
    fwd, rev = ec.slot_sums(t, lay, c32), ec.slot_sums(t, lay, c32, reverse=True)
    want = gemb.float().numpy()
    assert np.array_equal(fwd, want) and np.array_equal(rev, want)
    assert np.array_equal(ec.slot_sums(t, lay, ec.sorted_contributions(t, lay, np.float64), dtype=np.float64), gemb.numpy())


def _mutated(t, lay, c, kind, seg):
    """The expected gradient when the reduction drops the segment's first entry, counts it twice, or hands its last entry
    to the next slot."""
    lo, hi = lay.lo.clone(), lay.hi.clone()
    extra = None
    if kind == "drop":
        lo[seg] += 1
    elif kind == "twice":
        extra = c[int(lo[seg])]
    else:
        hi[seg] -= 1
        lo[seg + 1] -= 1
    out = ec.slot_sums(t, lay._replace(lo=lo, hi=hi), c, dtype=np.float64)
    if extra is not None:
        out[int(lay.slot[seg])] += extra
    return out.astype(np.float32)


@pytest.mark.parametrize("kind", ("drop", "twice", "move"))
@pytest.mark.parametrize("name", ("g700-C2-tiled-ac", "g100_412_300-C1-sentinel", "g255_257-C8-hash"))
def test_exact_case_is_sensitive(name, kind):
    t, lay, (_, gemb, _) = ec.exact_expectation(name)
    c = ec.sorted_contributions(t, lay, np.float64)
    want = gemb.float().numpy()
    for seg in range(lay.slot.numel() - 1):
        assert int(lay.hi[seg]) == int(lay.lo[seg + 1])          # neighbours in sorted order
        got = _mutated(t, lay, c, kind, seg)
        assert not np.array_equal(got[int(lay.slot[seg])], want[int(lay.slot[seg])]), (name, kind, seg)


@pytest.mark.parametrize("name", list(ec.FORM))
def test_form_case_restatement_is_inside_the_bars(name):
    e = ec.form_expectation(name)
    r_out, r_emb, r_in = e.r32
    ok = e.bar_out > 0                                            # (zero elements exempt here, not on the GPU)
    assert bool(((r_out - e.out).abs()[ok] <= e.bar_out[ok]).all())
    ok = e.bar_emb > 0
    assert bool(((r_emb - e.gemb).abs()[ok] <= e.bar_emb[ok]).all())
    assert bool((e.gemb[e.n_s == 0] == 0).all()) and bool((e.bar_emb[e.n_s == 0] == 0).all())
    assert e.bar_in <= 1e-4 * float(e.gin.abs().max())
    if FORM_KIND(name) != "outside":
        assert float(e.gin.abs().max()) > 0 and int(e.n_s.sum()) == int(e.inside.sum()) * e.t.L << e.t.D
    assert bool((e.out[~e.inside] == 0).all()) and bool((e.gin[~e.inside] == 0).all())


def FORM_KIND(name):
    return ec.FORM[name].kind


def test_form_cases_cover_every_instantiation_and_degenerate_call():
    names = set(ec.FORM)
    for D in (2, 3, 4, 5):
        for C in (1, 2, 4, 8):
            assert {"D%dC%d-hash-smooth-noac" % (D, C), "D%dC%d-tiled-linear-ac" % (D, C)} <= names
    c = ec.FORM["BL255-tiled-linear-ac"]
    assert c.B * c.L == 255
    c = ec.FORM["BL513-tiled-linear-ac"]
    assert c.B * c.L == 2 * 256 + 1
    assert ec.FORM["L64-hash-smooth-noac"].L == 64 and ec.FORM["L64-hash-smooth-noac"].pls == 1.02
    assert ec.FORM["pls1-hash-smooth-noac"].pls == 1.0 and ec.FORM["L1-hash-smooth-noac"].L == 1
    assert not bool(ec.form_expectation("all_outside-hash-smooth-noac").inside.any())
    x = ec.form_tensors(ec.FORM["D4C2-hash-smooth-noac"]).x
    assert torch.equal(x, ec.points(2000, 4, sum(map(ord, "D4C2-hash-smooth-noac"))))


@pytest.mark.parametrize("name", [n for n in ec.FORM if n.startswith("edges")])
def test_edge_rows_decide_as_stated(name):
    e = ec.form_expectation(name)
    t = e.t
    vals = ec.edge_values(t.L, t.pls, t.H)
    f = np.float32
    assert [float(v) for v in vals[:7]] == [0.0, 0.0, 1.0, float(f(1) - f(2.0 ** -24)), float(f(1) + f(2.0 ** -23)),
                                           -float(f(2.0 ** -149)), float(f(2.0 ** -149))]
    assert np.signbit(vals[1]) and not np.signbit(vals[0])
    want = torch.tensor([not (v < 0 or v > 1) for v in vals]).repeat(t.D)
    assert torch.equal(e.inside, want) and int((~want).sum()) == 2 * t.D
    assert bool(np.signbit(t.x[1, 0].numpy()))
    # a row the oracle places inside has a non-zero output, so the GPU's zeros tell its decision
    assert bool((e.out[e.inside] != 0).any(dim=1).all())
    # cell faces of level 0 (scale 4) are exact: frac == 0 there
    sc0 = ref.level_geometry(t.L, t.pls, t.H)[0][0]
    assert sc0 == 4.0 and all(float(f(v) * f(sc0)) == round(float(f(v) * f(sc0))) for v in vals[7:10])


def test_pass_count_cases():
    assert [ec.sort_passes(c.offsets[-1]) for c in ec.PASSES.values()] == [1, 2, 2, 3, 4]
    assert [c.offsets[-1] for c in ec.PASSES.values()] == [248, 256, 65528, 65536, 17 << 20]
    for name, c in ec.PASSES.items():
        assert c.passes == ec.sort_passes(c.offsets[-1]) and name.startswith("passes%d-" % c.passes)
    assert ec.sort_passes(255) == 1 and ec.sort_passes((1 << 24) - 1) == 3 and ec.sort_passes(1 << 24) == 4


@pytest.mark.parametrize("name", [n for n in ec.PASSES if not n.startswith("passes4")])
def test_pass_count_case_uses_the_high_key_bits(name):
    """The touched slots span the table, so a sort that stopped one pass short would leave them out of order."""
    e = ec.expect(ec.pass_tensors(ec.PASSES[name]))
    touched = torch.nonzero(e.n_s).flatten()
    n = e.t.offsets[-1]
    assert int(touched.max()) >= n - n // 8 and int(touched.min()) < n // 8
    ok = e.bar_emb > 0
    assert bool(((e.r32[1] - e.gemb).abs()[ok] <= e.bar_emb[ok]).all())


def test_four_pass_case_sparse_expectation_matches_the_oracle_on_a_small_table():
    """sparse_expectation's construction, on the 65536-slot case where the dense oracle is cheap."""
    name = "passes3-slots65536"
    s, e = ec.sparse_expectation(name), ec.expect(ec.pass_tensors(ec.PASSES[name]))
    assert float((s.out - e.out).abs().max()) < 1e-12 and float((s.bar_out - e.bar_out).abs().max()) < 1e-18
    assert torch.equal(s.slots, torch.nonzero(e.n_s).flatten())
    assert float((s.gemb - e.gemb[s.slots]).abs().max()) < 1e-12
    assert float((s.bar_emb - e.bar_emb[s.slots]).abs().max()) < 1e-18
    big = ec.sparse_expectation("passes4-slots17x2^20")
    assert int(big.slots.max()) >= 1 << 24 and big.t.offsets[-1] == 17 << 20


@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_column_bars_catch_a_wrong_band(degree):
    e = ec.sh_expectation("scaled", degree)
    top = float(e.out.abs().max())
    assert bool((e.bar_out <= 1e-4 * top).all())
    if degree >= 2:
        # a band-1 sign or constant error stays inside 1e-4 of the tensor's largest entry at high degree, never inside its column's bar
        for col in (1, 2, 3):
            assert float((2 * e.out[:, col]).abs().max()) > e.bar_out[col]
            assert float((0.01 * e.out[:, col]).abs().max()) > e.bar_out[col]
    if degree == 8:
        assert float((0.01 * e.out[:, 1]).abs().max()) < 1e-4 * top
    axes = ec.sh_expectation("axes", degree)
    assert axes.v.shape == (11, 3) and bool((axes.v[-1] == 0).all())
    # at the poles and the zero vector every column with m != 0 vanishes
    for l in range(degree):
        for m in range(-l, l + 1):
            if m:
                assert bool((axes.out[6:, l * l + l + m] == 0).all())
    for name, B in (("B0", 0), ("B1", 1), ("B255", 255), ("B257", 257)):
        assert ec.sh_expectation(name, degree).out.shape == (B, degree * degree)
