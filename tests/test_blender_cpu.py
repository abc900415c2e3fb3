"""tests/blender_cases.py proven (each case has the property it is named for), tests/blender_reference.py's restatements held
to train_blender.py's literal statements on CPU torch, and the fp32 restatements' own distance to their float64 twins put on
record - the figures the GPU tests' bars are read against."""
import math

import pytest
import torch

import blender_cases as bc
import blender_reference as br


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("H,W", bc.IMAGE_SIZES)
def test_images_have_the_pixels_they_are_named_for(H, W):
    below, at, above = bc.around(bc.BG_THR)
    assert below < at < above and at == float(torch.tensor(254 / 255, dtype=torch.float32))
    gt = bc.image(H, W, "mixed")
    assert gt.dtype == torch.float32 and gt.shape == (3, H, W) and gt.is_contiguous()
    mask = br.background_mask(gt, bc.BG_THR)
    assert mask.shape == (1, H, W) and mask.dtype == torch.bool
    flat, m = gt.view(3, -1), mask.view(-1)
    spots = bc.edge_pixels(H, W)
    assert "at" in spots
    if H * W >= 15:
        assert set(spots) == {"at", "above", "below", "nan", "nan_white"}
    want = dict(at=False, above=True, below=False, nan=False, nan_white=False)
    for name, i in spots.items():
        assert bool(m[i]) is want[name], name
        if name in ("at", "above", "below"):
            assert float(flat[:, i].min()) == dict(at=at, above=above, below=below)[name]
            assert int((flat[:, i] == 1.0).sum()) == 2             # the other two channels are white
        if name == "nan":
            assert int(flat[:, i].isnan().sum()) == 1 and int((flat[:, i] == 1.0).sum()) == 2
        if name == "nan_white":
            assert bool(flat[:, i].isnan().all())
    if H * W >= 15:
        assert 0 < int(mask.sum()) < H * W
    assert int(br.background_mask(bc.image(H, W, "white"), bc.BG_THR).sum()) == H * W
    assert int(br.background_mask(bc.image(H, W, "none"), bc.BG_THR).sum()) == 0


def test_the_comparison_is_fp32_and_strict():
    """torch compares an fp32 tensor against the Python double 254/255 in fp32: the pixel at float32(254/255) is NOT above it,
    although float32(254/255) > 254/255 as real numbers"""
    _, at, above = bc.around(bc.BG_THR)
    assert at > 254 / 255                                           # the rounding went up: a float64 comparison would mask it
    x = torch.tensor([at, above], dtype=torch.float32)
    assert (x > 254 / 255).tolist() == [False, True]
    assert (x.double() > 254 / 255).tolist() == [True, True]
    _, at, above = bc.around(bc.WHITE_THR)
    x = torch.tensor([at, above], dtype=torch.float32)
    assert (x > 253 / 255).tolist() == [False, True]


@pytest.mark.parametrize("H,W", bc.IMAGE_SIZES)
@pytest.mark.parametrize("kind", bc.IMAGE_KINDS)
def test_target_restatements_are_the_literal_statements(H, W, kind):
    gt_image, stored = bc.image(H, W, kind), bc.mono_image(H, W)
    # train_blender.py:87, :96-97, the statements as written
    bg_mask = (gt_image.min(0, keepdim=True).values > 254 / 255)
    depth_mono = 255.0 - stored
    depth_mono = depth_mono[None]
    depth_mono[bg_mask] = 0
    assert torch.equal(br.background_mask(gt_image, bc.BG_THR), bg_mask)
    assert same_bits(br.depth_target(stored, bg_mask), depth_mono[0])
    mask, count, target = br.target_elementwise(gt_image, stored, bc.BG_THR)
    assert torch.equal(mask, bg_mask) and count == int(bg_mask.sum())
    assert same_bits(target, depth_mono[0])
    assert bool((bits(target)[bg_mask[0]] == 0).all())             # +0.0 by sign bit
    assert same_bits(stored, bc.mono_image(H, W))                   # the stored map is left alone


# ---------------------------------------------------------------------------------------------------------------- white rule
@pytest.mark.parametrize("P", bc.RULE_P)
def test_rule_rows_have_the_rows_they_are_named_for(P):
    colour, stat, opacity = bc.rule_rows(P)
    below, at, above = bc.around(bc.WHITE_THR)
    assert colour.shape == (P, 3) and stat.shape == (P, 1) and opacity.shape == (P, 1)
    assert bool((stat > 0).all())
    mn = colour.min(-1).values
    for i, (v, fires) in enumerate(((below, False), (at, False), (above, True))):
        if 7 * i < P:
            assert float(mn[7 * i]) == v and bool(mn[7 * i] > 253 / 255) is fires
    for k, v in enumerate(bc.SPECIAL_OPACITIES):
        if 3 + 5 * k < P:
            got = float(opacity[3 + 5 * k, 0])
            assert (math.isnan(got) and math.isnan(v)) or (got == v and math.copysign(1, got) == math.copysign(1, v))
            assert bool(mn[3 + 5 * k] > 253 / 255)                  # a special opacity sits on a row that fires
    if P >= 63:
        assert float(opacity[3 + 5 * 4, 0]) == bc.DENORMAL and 0 < bc.DENORMAL < 1.1754944e-38
        assert bool(colour[40].isnan().any()) and int((colour[40] == 1.0).sum()) == 2
        n = int((mn > 253 / 255).sum())
        assert P // 3 < n < P


@pytest.mark.parametrize("P", bc.RULE_P)
def test_white_rule_restatements_are_the_literal_statements(P):
    color, stat, opacity = bc.rule_rows(P)
    xyz_gradient_accum, _opacity = stat.clone(), opacity.clone()
    # train_blender.py:208-211, the statements as written
    white_mask = color.min(-1, keepdim=True).values > 253 / 255
    xyz_gradient_accum[white_mask] = 0
    _opacity[white_mask] = br.inverse_sigmoid(torch.sigmoid(_opacity[white_mask]) * 0.1)
    s, o = stat.clone(), opacity.clone()
    n = br.white_rule(color, s, o, bc.WHITE_THR, 0.1)
    assert n == int(white_mask.sum()) and same_bits(s, xyz_gradient_accum) and same_bits(o, _opacity)
    fires, s2, o2 = br.white_rule_elementwise(color, stat, opacity, bc.WHITE_THR, 0.1)
    assert torch.equal(fires, white_mask.reshape(-1)) and same_bits(s2, xyz_gradient_accum) and same_bits(o2, _opacity)
    assert same_bits(o[~white_mask], opacity[~white_mask])          # rows that did not fire keep their bits
    assert bool((bits(s)[white_mask] == 0).all())
    if P > 40:
        assert not bool(white_mask[40])                             # a NaN channel fires nothing


def test_special_opacities_as_torch_gives_them():
    o = torch.tensor(bc.SPECIAL_OPACITIES, dtype=torch.float32)
    got = br.inverse_sigmoid(torch.sigmoid(o) * 0.1)
    twin = br.new_opacity64(o)
    assert float(got[5]) == float("-inf") == float(twin[5])         # -inf: the sigmoid is 0
    assert math.isnan(float(got[6])) and math.isnan(float(twin[6]))
    assert bool(got[:5].isfinite().all()) and bool(twin[:5].isfinite().all())
    err = ((got[:5].double() - twin[:5]).abs() / br.spacing(twin[:5])).max()
    print("special opacities: fp32 restatement - float64 twin = %.3f ulp at worst" % float(err))
    assert float(err) <= 2.0


def test_opacity_formula_fp32_distance_to_float64():
    """For the record: torch's fp32 log(x / (1 - x)) of 0.1 sigmoid(o) against the float64 twin over 600 000 values of o in
    [-20, 20].  The figure is the RESTATEMENT's own distance, not the kernel's (the kernel evaluates in double and is held to
    1 ulp in tests/test_gpu_blender_kernels.py).  Observed: 1.26 ulp at worst, 0.28 on average - not within 1 ulp.  The bar
    asserted here is derived, not observed: x <= 0.1, so the quotient
    q = x / (1 - x) carries at most 1 (sigmoid) + 0.5 + 0.5 + 0.5 ulp = 2.5 x 6e-8 relative error, which log turns into
    1.5e-7 ABSOLUTE - 0.63 of the spacing 2.4e-7 of a result that is never above -2.197 - plus log's own rounding: under
    2 ulp."""
    o = torch.linspace(-20.0, 20.0, 600_000, dtype=torch.float32)
    got = br.inverse_sigmoid(torch.sigmoid(o) * 0.1)
    twin = br.new_opacity64(o)
    err = (got.double() - twin).abs() / br.spacing(twin)
    print("opacity formula: fp32 - float64 = %.3f ulp at worst, %.3f on average, over %d values" % (float(err.max()), float(err.mean()), o.numel()))
    assert float(err.max()) <= 2.0
    assert float(twin.max()) <= math.log(0.1 / 0.9) + 1e-6


# ---------------------------------------------------------------------------------------------------------------- SH rows
@pytest.mark.parametrize("P", bc.RULE_P)
@pytest.mark.parametrize("M", (1, 4, 9, 16))
def test_sh_rows_hold_their_margin_at_every_active_degree(P, M):
    xyz, features, campos, stat, opacity, centre = bc.sh_rows(P, M)
    assert features.shape == (P, M, 3) and bool((features != 0).all())     # the inactive coefficients too
    thr = float(bc.f32(bc.WHITE_THR))
    for (MM, d) in bc.SH_FORMS:
        if MM != M:
            continue
        c64 = br.sh_colour64(xyz, features, d, campos)
        mn = c64.min(-1).values
        far = (mn - thr).abs() > bc.SH_MARGIN
        if centre is not None:
            assert bool(xyz[centre].eq(campos).all())
        if centre is not None and d > 0:
            assert bool(c64[centre].isnan().all())                  # on the camera centre: 0 / 0
            far[centre] = True                                      # (a NaN is on neither side: it never fires)
            assert int(c64.isnan().any(-1).sum()) == 1
        else:
            assert not bool(c64.isnan().any())                      # degree 0 does not look at the direction
        assert bool(far.all()), (M, d, int((~far).sum()))           # EVERY row: none is exempt from the decision check
        c32 = br.sh_colour(xyz, features, d, campos)
        fires32 = c32.min(-1).values > bc.WHITE_THR
        fires64 = mn > thr
        assert torch.equal(fires32, fires64)
        if P >= 63:
            assert 0 < int(fires64.sum()) < P
        assert bool((c64[~c64.isnan()] >= 0).all())
        ok = ~c64.isnan()
        err = ((c32.double() - c64).abs() / br.spacing(c64))[ok]
        print("sh colour P %4d M %2d degree %d: fp32 restatement - float64 twin = %.2f ulp at worst (%.2e absolute)"
              % (P, M, d, float(err.max()), float((c32.double() - c64).abs()[ok].max())))
        assert float((c32.double() - c64).abs()[ok].max()) < bc.SH_MARGIN / 10   # the margin is many times fp32's own error


def test_inactive_coefficients_do_not_reach_the_colour():
    xyz, features, campos, _, _, _ = bc.sh_rows(65, 16)
    for d in range(4):
        na = (d + 1) ** 2
        other = features.clone()
        other[:, na:, :] = 1e6
        a, b = br.sh_colour(xyz, features, d, campos), br.sh_colour(xyz, other, d, campos)
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a[~a.isnan()], b[~b.isnan()])
        assert same_bits(br.sh_colour(xyz, features[:, :na].contiguous(), d, campos).nan_to_num(7.0), a.nan_to_num(7.0))


@pytest.mark.parametrize("M,d", bc.SH_FORMS)
def test_white_rule_sh_restatement_is_the_literal_statements(M, d):
    P = 257
    xyz, features, campos, stat, opacity, centre = bc.sh_rows(P, M)
    # gaussian_renderer/__init__.py:351-355 and train_blender.py:367-370, the statements as written (max_sh_degree from M)
    shs_view = features.transpose(1, 2).reshape(-1, 3, M)
    dir_pp = (xyz - campos.repeat(features.shape[0], 1))
    dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
    color = torch.clamp_min(br.eval_sh(d, shs_view, dir_pp_normalized) + 0.5, 0.0)
    white_mask = color.min(-1, keepdim=True).values > 253 / 255
    accum, _opacity = stat.clone(), opacity.clone()
    accum[white_mask] = 0
    _opacity[white_mask] = br.inverse_sigmoid(torch.sigmoid(_opacity[white_mask]) * 0.1)
    s, o = stat.clone(), opacity.clone()
    n, colour = br.white_rule_sh(xyz, features, d, campos, s, o, bc.WHITE_THR, 0.1)
    assert n == int(white_mask.sum()) and same_bits(s, accum) and same_bits(o, _opacity)
    assert same_bits(colour.nan_to_num(7.0), color.nan_to_num(7.0))
    if d > 0:
        assert not bool(white_mask[centre]) and bool(color[centre].isnan().all())
    else:
        assert not bool(color.isnan().any())                        # degree 0 does not look at the direction
