"""The Blender kernels (csrc/gs_dng_blender.hip through gsplat_amd/dng_blender.py) on the GPU against
tests/blender_reference.py's torch restatements on the CPU, over the case table of tests/blender_cases.py (proven in
tests/test_blender_cpu.py).

  mask, count, target      EXACT (the unmasked target is one fp32 subtraction)
  white-rule decisions, counts, zeroed statistics   EXACT; rows that did not fire keep their bits
  new opacity, colour_out  within 1 fp32 ulp of the float64 twin.  Derived: the kernel evaluates in double (every operation
                           within a few 1e-16 relative, four orders of magnitude under half an fp32 ulp, and neither formula
                           cancels: the opacity's result is at most log(0.1 / 0.9), the colour is compared after the + 0.5) and
                           rounds ONCE, so it lands on one of the two fp32 neighbours of the float64 value: under 1 ulp.
                           A colour that clamps to 0 is 0 on both sides.  Non-finite cases match torch.
The SH rows hold SH_MARGIN to the threshold (asserted for EVERY row in tests/test_blender_cpu.py), so the decision of the
rounded colour is the float64 decision and no row is exempt.
The observed worst distances go to the file BLENDER_PARITY_OUT names, when it is set (profiles/blender_parity.json holds a whole
run's)."""
import json
import os

import pytest
import torch

import blender_cases as bc
import blender_reference as br
from gsplat_amd import dng_blender, synthetic
from gsplat_amd.trainer import GaussianModelLite

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PARITY = {}


def _record(key, value):
    """the worst distances seen, into the file BLENDER_PARITY_OUT names - only when it is set, so that a plain or partial run of
    the suite leaves the committed profiles/blender_parity.json (written by a whole run of this file) alone"""
    PARITY[key] = max(PARITY.get(key, 0.0), float(value))
    out = os.environ.get("BLENDER_PARITY_OUT")
    if not out:
        return
    try:
        with open(out, "w") as f:
            json.dump(dict(unit="fp32 ulp of the float64 value, worst over the case table", bar=1.0, observed=PARITY), f, indent=1,
                      sort_keys=True)
    except OSError:
        pass


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ulps(got, want64):
    """|got - want| in fp32 ulps of want, over the finite entries; the others must agree as torch's (inf by sign, NaN by place)"""
    got, want64 = got.detach().cpu().double(), want64.double()
    fin = want64.isfinite()
    assert torch.equal(got.isnan(), want64.isnan())
    inf = want64.isinf()
    assert torch.equal(got[inf], want64[inf])
    if not bool(fin.any()):
        return 0.0
    return float(((got[fin] - want64[fin]).abs() / br.spacing(want64[fin])).max())


# ---------------------------------------------------------------------------------------------------------------- target
@pytest.mark.parametrize("H,W", bc.IMAGE_SIZES)
@pytest.mark.parametrize("kind", bc.IMAGE_KINDS)
def test_mask_count_and_target_are_the_restatements(hip, H, W, kind):
    gt, mono = bc.image(H, W, kind), bc.mono_image(H, W)
    want_mask = br.background_mask(gt, bc.BG_THR)
    want_target = br.depth_target(mono, want_mask)
    g, m = gt.to(DEV), mono.to(DEV)
    mask, target, count = dng_blender.blender_background_mask(g, bc.BG_THR, mono=m, return_count=True)
    assert mask.dtype == torch.bool and mask.shape == (1, H, W) and target.shape == (H, W) and count.dtype == torch.int32
    assert torch.equal(mask.cpu(), want_mask), int((mask.cpu() != want_mask).sum())
    assert int(count[0]) == int(want_mask.sum())
    assert same_bits(target, want_target)
    assert same_bits(g, gt) and same_bits(m, mono)                  # new tensors: the inputs are left alone
    assert target.data_ptr() != m.data_ptr()
    if kind == "white":
        assert int(count[0]) == H * W and bool((bits(target) == 0).all())
    if kind == "none":
        assert int(count[0]) == 0
    # without a mono map: the mask alone, the same one; a [1,H,W] map gives a [1,H,W] target
    only = dng_blender.blender_background_mask(g, bc.BG_THR)
    assert torch.is_tensor(only) and torch.equal(only, mask)
    mask2, count2 = dng_blender.blender_background_mask(g, bc.BG_THR, return_count=True)
    assert torch.equal(mask2, mask) and int(count2[0]) == int(count[0])
    _, target3 = dng_blender.blender_background_mask(g, bc.BG_THR, mono=m[None])
    assert target3.shape == (1, H, W) and same_bits(target3[0], want_target)


def test_target_of_more_pixels_than_one_sweep_of_the_grid(hip):
    """256 workgroups x 1024 pixels is one sweep: 600 x 500 makes the workgroups go round again"""
    H, W = 600, 500
    gt, mono = bc.image(H, W, "mixed"), bc.mono_image(H, W)
    want_mask = br.background_mask(gt, bc.BG_THR)
    mask, target, count = dng_blender.blender_background_mask(gt.to(DEV), bc.BG_THR, mono=mono.to(DEV), return_count=True)
    assert torch.equal(mask.cpu(), want_mask) and int(count[0]) == int(want_mask.sum())
    assert same_bits(target, br.depth_target(mono, want_mask))


def test_binding_refuses_what_the_kernels_do_not_take(hip):
    gt = bc.image(3, 5).to(DEV)
    with pytest.raises(ValueError):
        dng_blender.blender_background_mask(gt[:2], bc.BG_THR)
    with pytest.raises(ValueError):
        dng_blender.blender_background_mask(gt, bc.BG_THR, mono=torch.zeros((4, 4), device=DEV))
    with pytest.raises(RuntimeError):
        dng_blender.blender_background_mask(gt.cpu(), bc.BG_THR)
    with pytest.raises(RuntimeError):
        dng_blender.blender_background_mask(gt.double(), bc.BG_THR)
    with pytest.raises(TypeError):
        dng_blender.blender_background_mask(gt, bc.BG_THR, out=gt)      # in-place aliasing is not offered
    colour, stat, opacity = (t.to(DEV) for t in bc.rule_rows(65))
    with pytest.raises(ValueError):
        dng_blender.white_rule(colour, stat[:64], opacity, bc.WHITE_THR)
    with pytest.raises(ValueError):
        dng_blender.white_rule(colour, torch.zeros((65, 2), device=DEV)[:, :1], opacity, bc.WHITE_THR)   # not contiguous
    xyz, features, campos, s, o, _ = (t.to(DEV) if torch.is_tensor(t) else t for t in bc.sh_rows(65, 9))
    with pytest.raises(ValueError):
        dng_blender.white_rule_sh(xyz, features, 3, campos, s, o, bc.WHITE_THR)            # degree 3 needs 16 coefficients
    with pytest.raises(ValueError):
        dng_blender.white_rule_sh(xyz, features[:, :5].contiguous(), 1, campos, s, o, bc.WHITE_THR)
    assert same_bits(s, bc.sh_rows(65, 9)[3]) and same_bits(o, bc.sh_rows(65, 9)[4])      # nothing was edited


def test_error_paths_return_their_codes_with_nothing_launched(hip):
    from gsplat_amd._lib import hip_api
    api = hip_api()
    size, target, rule, rule_sh = (api.raw(n) for n in ("blender_tmp_bytes", "blender_target", "dng_white_rule", "dng_white_rule_sh"))
    assert size(0) == 0 and size(-1) == 0 and size(1 << 31) == 0 and size(1) > 0
    assert size(256 * 1024) == size(100 * 256 * 1024)               # the grid is capped, so is the scratch
    one = 16  # any non-null address: the checks below return before anything is launched
    assert target(one, one, 0, 4, 0.5, one, one, one, one, None) == -2
    assert target(one, one, 4, -1, 0.5, one, one, one, one, None) == -2
    assert target(one, one, 1 << 16, 1 << 15, 0.5, one, one, one, one, None) == -2          # H W = 2^31
    assert target(None, one, 4, 4, 0.5, one, one, one, one, None) == -1
    assert target(one, one, 4, 4, 0.5, None, one, one, one, None) == -1
    assert target(one, one, 4, 4, 0.5, one, None, one, one, None) == -1
    assert target(one, one, 4, 4, 0.5, one, one, None, one, None) == -1
    assert target(one, None, 4, 4, 0.5, one, one, one, one, None) == -1                      # a target needs the mono map
    assert rule(one, one, one, 0, 0.5, 0.1, one, None) == -2 and rule(one, one, one, 1 << 31, 0.5, 0.1, one, None) == -2
    for k in range(3):
        a = [one, one, one]
        a[k] = None
        assert rule(a[0], a[1], a[2], 8, 0.5, 0.1, one, None) == -1
    assert rule(one, one, one, 8, 0.5, 0.1, None, None) == -1
    assert rule_sh(one, one, one, 16, 3, one, one, one, 0, 0.5, 0.1, None, one, None) == -2
    # (46340 and up: (degree + 1)^2 no longer fits an int32 - refused before it is formed)
    for M, deg in ((0, 0), (5, 1), (25, 4), (16, 4), (9, 3), (4, 2), (1, 1), (4, -1), (16, 46340), (16, 65535), (16, 2 ** 31 - 1)):
        assert rule_sh(one, one, one, M, deg, one, one, one, 8, 0.5, 0.1, None, one, None) == -2, (M, deg)
    assert rule_sh(None, one, one, 16, 3, one, one, one, 8, 0.5, 0.1, None, one, None) == -1
    assert rule_sh(one, None, None, 16, 3, one, one, one, 8, 0.5, 0.1, None, one, None) == -1  # no rows in either form
    assert rule_sh(one, one, None, 16, 3, one, one, one, 8, 0.5, 0.1, None, one, None) == -1   # split without rest
    assert rule_sh(one, one, one, 16, 3, None, one, one, 8, 0.5, 0.1, None, one, None) == -1
    assert rule_sh(one, one, one, 16, 3, one, None, one, 8, 0.5, 0.1, None, one, None) == -1
    assert rule_sh(one, one, one, 16, 3, one, one, None, 8, 0.5, 0.1, None, one, None) == -1
    assert rule_sh(one, one, one, 16, 3, one, one, one, 8, 0.5, 0.1, None, None, None) == -1
    torch.cuda.synchronize()                                         # nothing was launched: nothing can have faulted


# ---------------------------------------------------------------------------------------------------------------- white rule
@pytest.mark.parametrize("P", bc.RULE_P)
def test_white_rule_rows_counts_and_opacity(hip, P):
    colour, stat, opacity = bc.rule_rows(P)
    ws, wo = stat.clone(), opacity.clone()
    n = br.white_rule(colour, ws, wo, bc.WHITE_THR, 0.1)
    fires = (colour.min(-1, keepdim=True).values > bc.WHITE_THR)
    c, s, o = colour.to(DEV), stat.to(DEV), opacity.to(DEV)
    counts = dng_blender.white_rule(c, s, o, bc.WHITE_THR, 0.1)
    assert counts.dtype == torch.int32 and counts.shape == (1,) and int(counts[0]) == n == int(fires.sum())
    assert same_bits(s, ws)                                         # zeroed (+0.0) where fired, the same bits elsewhere
    assert same_bits(o.cpu()[~fires], opacity[~fires])              # rows that did not fire: untouched
    assert same_bits(c, colour)
    if n:
        d = ulps(o.cpu()[fires], br.new_opacity64(opacity)[fires])
        print("white rule P %4d: %d rows fired, new opacity - float64 = %.3f ulp at worst" % (P, n, d))
        _record("white_rule_opacity", d)
        assert d <= 1.0
        # the non-finite rows as torch's fp32 statement has them
        w, g = wo[fires], o.cpu()[fires]
        assert torch.equal(g.isnan(), w.isnan()) and torch.equal(g.isinf(), w.isinf())
        assert torch.equal(g[g.isinf()], w[w.isinf()])
    # [P] views of the same memory
    s1, o1 = stat.reshape(-1).to(DEV), opacity.reshape(-1).to(DEV)
    counts1 = dng_blender.white_rule(c, s1, o1, bc.WHITE_THR)
    assert int(counts1[0]) == n and same_bits(s1, s.reshape(-1)) and same_bits(o1, o.reshape(-1))


def test_white_rule_other_threshold_and_factor(hip):
    colour, stat, opacity = bc.rule_rows(257)
    for thr, factor in ((0.5, 0.25), (0.0, 0.9), (2.0, 0.1)):
        ws, wo = stat.clone(), opacity.clone()
        n = br.white_rule(colour, ws, wo, thr, factor)
        fires = (colour.min(-1, keepdim=True).values > thr)
        s, o = stat.to(DEV), opacity.to(DEV)
        counts = dng_blender.white_rule(colour.to(DEV), s, o, thr, factor)
        assert int(counts[0]) == n and same_bits(s, ws) and same_bits(o.cpu()[~fires], opacity[~fires])
        if n:
            assert ulps(o.cpu()[fires], br.new_opacity64(opacity, factor)[fires]) <= 1.0
    assert n == 0                                                    # nothing is whiter than 2


def test_white_rule_leaves_the_moments_of_a_flat_adam_alone(hip):
    P = 257
    m = GaussianModelLite(synthetic.trained_like(P, seed=4), DEV, api=hip.api)
    o = m.optimizer
    g = torch.Generator().manual_seed(8)
    o.exp_avg.copy_(torch.randn(o.exp_avg.shape, generator=g))
    o.exp_avg_sq.copy_(torch.rand(o.exp_avg_sq.shape, generator=g))
    m.xyz_gradient_accum.copy_(torch.rand((P, 1), generator=g) + 0.1)
    colour, _, _ = bc.rule_rows(P)
    before = dict(m=o.exp_avg.clone(), v=o.exp_avg_sq.clone(), flat=m.flat.detach().clone().cpu(), accum=m.xyz_gradient_accum.clone().cpu())
    raw = m.params["opacity"].detach()
    assert raw.data_ptr() == m.params["opacity"].data_ptr()
    counts = dng_blender.white_rule(colour.to(DEV), m.xyz_gradient_accum, raw, bc.WHITE_THR)
    fires = colour.min(-1).values > bc.WHITE_THR
    assert int(counts[0]) == int(fires.sum()) > 0
    assert same_bits(o.exp_avg, before["m"]) and same_bits(o.exp_avg_sq, before["v"])
    assert same_bits(m.xyz_gradient_accum, torch.where(fires[:, None], torch.zeros(()), before["accum"]))
    changed = bits(m.flat) != bits(before["flat"])
    off = int(raw.data_ptr() - m.flat.data_ptr()) // 4
    rows = torch.zeros_like(changed)
    rows[off:off + P] = fires
    assert not bool((changed & ~rows).any()) and int(changed.sum()) > 0  # the opacity rows that fired alone moved


# ---------------------------------------------------------------------------------------------------------------- SH form
@pytest.mark.parametrize("P", bc.RULE_P)
@pytest.mark.parametrize("M,d", bc.SH_FORMS)
def test_white_rule_sh_split_and_packed(hip, P, M, d):
    xyz, features, campos, stat, opacity, centre = bc.sh_rows(P, M)
    c64 = br.sh_colour64(xyz, features, d, campos)
    fires = c64.min(-1).values > float(bc.f32(bc.WHITE_THR))        # (SH_MARGIN away: the rounded colour decides the same)
    if centre is not None and d > 0:
        assert not bool(fires[centre]) and bool(c64[centre].isnan().all())
    n = int(fires.sum())
    f = fires[:, None]
    X, F, C = xyz.to(DEV), features.to(DEV), campos.to(DEV)
    got = {}
    for form in ("packed", "split"):
        shs = F if form == "packed" else (F[:, :1].contiguous(), F[:, 1:].contiguous())
        s, o = stat.to(DEV), opacity.to(DEV)
        counts, colour = dng_blender.white_rule_sh(X, shs, d, C, s, o, bc.WHITE_THR, 0.1, return_colour=True)
        assert int(counts[0]) == n, (form, int(counts[0]), n)
        assert colour.shape == (P, 3)
        dc = ulps(colour, c64)
        _record("white_rule_sh_colour", dc)
        assert dc <= 1.0, (form, dc)
        assert torch.equal(colour.cpu().min(-1).values > bc.WHITE_THR, fires)
        assert same_bits(s, torch.where(f, torch.zeros(()), stat))
        assert same_bits(o.cpu()[~f], opacity[~f])
        if n:
            do = ulps(o.cpu()[f], br.new_opacity64(opacity)[f])
            _record("white_rule_sh_opacity", do)
            assert do <= 1.0
        # without colour_out: the same edits and count
        s2, o2 = stat.to(DEV), opacity.to(DEV)
        counts2 = dng_blender.white_rule_sh(X, shs, d, C, s2, o2, bc.WHITE_THR, 0.1)
        assert torch.is_tensor(counts2) and int(counts2[0]) == n and same_bits(s2, s) and same_bits(o2, o)
        got[form] = (colour, s, o)
    for a, b in zip(got["packed"], got["split"]):
        assert same_bits(a, b)                                      # one result, whichever way the rows are held
    assert same_bits(F, features) and same_bits(X, xyz)
    # the coefficients above the active degree are not read into the result
    if (d + 1) ** 2 < M:
        F2 = F.clone()
        F2[:, (d + 1) ** 2:, :] = float("nan")
        s, o = stat.to(DEV), opacity.to(DEV)
        counts3, colour3 = dng_blender.white_rule_sh(X, F2, d, C, s, o, bc.WHITE_THR, 0.1, return_colour=True)
        assert int(counts3[0]) == n and same_bits(colour3, got["packed"][0]) and same_bits(o, got["packed"][2])


def test_white_rule_sh_is_white_rule_on_its_own_colour(hip):
    P, M, d = 1023, 16, 3
    xyz, features, campos, stat, opacity, _ = bc.sh_rows(P, M)
    s, o = stat.to(DEV), opacity.to(DEV)
    counts, colour = dng_blender.white_rule_sh(xyz.to(DEV), features.to(DEV), d, campos.to(DEV), s, o, bc.WHITE_THR, return_colour=True)
    s2, o2 = stat.to(DEV), opacity.to(DEV)
    counts2 = dng_blender.white_rule(colour, s2, o2, bc.WHITE_THR)
    assert int(counts[0]) == int(counts2[0]) > 0 and same_bits(s, s2) and same_bits(o, o2)
