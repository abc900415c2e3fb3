"""The restatements of tests/dtu_reference.py and the case table of tests/dtu_cases.py, proven without a GPU: what the DTU
kernels (csrc/gs_dng_dtu.hip) are held to in tests/test_gpu_dtu_kernels.py."""
import os
import re

import pytest
import torch

import dtu_cases as dc
import dtu_reference as dr


@pytest.mark.parametrize("H,W", dc.MASK_SIZES)
@pytest.mark.parametrize("run", (1, 50))
def test_the_run_length_statement_is_the_literal_loop(H, W, run):
    for kind in ("runs", "dark", "bright"):
        gt = dc.mask_image(H, W, 30 / 255, kind)
        want, zeroed = dr.background_mask(gt.clone(), 30 / 255, run)
        got = dr.background_mask_runs(gt, 30 / 255, run)
        assert want.shape == got.shape == (1, H, W)
        assert torch.equal(want, got), (kind, int((want != got).sum()))
        assert torch.equal(zeroed, torch.where(want, torch.zeros_like(gt), gt))
        if kind == "dark":
            assert bool(want.all())
        if kind == "bright":
            assert not bool(want.any())


def test_the_case_table_reaches_both_sides_of_every_run_edge():
    """a run of 48 or 49 rows masks nothing below row 48 unless it starts at row 0; runs of 50 and 51 mask their last 1 and 2
    rows; a run that starts at row 0 masks all of itself"""
    H, W = 130, 130
    specs = dc.run_specs(H)
    assert {L for _, L in specs} == {48, 49, 50, 51} and {s for s, _ in specs} >= {0, H // 3, H - 51}
    gt = dc.mask_image(H, W, 30 / 255)
    mask = dr.background_mask_runs(gt, 30 / 255, 50)[0]
    for x, (s, L) in enumerate(specs):
        col = mask[:, x]
        want = L if s == 0 else max(L - 49, 0)
        assert int(col.sum()) == want, (s, L, int(col.sum()))
    assert 0 < int(mask.sum()) < H * W


def test_the_mask_of_the_zeroed_image_is_the_same_mask():
    for H, W in ((51, 65), (130, 130)):
        gt = dc.mask_image(H, W, 30 / 255)
        mask, zeroed = dr.background_mask(gt.clone(), 30 / 255)
        again, twice = dr.background_mask(zeroed.clone(), 30 / 255)
        assert torch.equal(mask, again) and torch.equal(zeroed, twice)


@pytest.mark.parametrize("thr", dc.THRESHOLDS)
def test_the_threshold_is_float32_of_the_python_float(thr):
    """torch compares a float32 tensor against float32(thr): the neighbour below is under it, float32(thr) itself and the
    neighbour above are not - whatever side of float32(thr) the double lies on"""
    below, at, above = dc.around(thr)
    x = torch.tensor([below, at, above], dtype=torch.float32)
    assert (x < thr).tolist() == [True, False, False]
    assert (x > thr).tolist() == [False, False, True]
    assert (x < dc.f32(thr)).tolist() == [True, False, False]
    gt = torch.stack([x, x * 0.5, x * 0.25]).reshape(3, 1, 3)
    assert dr.background_mask(gt.clone(), thr, 1)[0].reshape(-1).tolist() == [True, False, False]


def test_the_mask_image_carries_the_threshold_rows():
    H, W, thr = 51, 65, 30 / 255
    gt = dc.mask_image(H, W, thr)
    mx = gt.max(0).values[:, W - 1]
    below, at, above = dc.around(thr)
    assert [float(mx[(H // 4) * k]) for k in (1, 2, 3)] == [at, below, above]
    dark = mx < thr
    assert dark.tolist().count(False) == 2


def test_an_empty_mask_gives_a_nan_penalty_a_zero_cotangent_and_a_step_that_moves():
    torch.manual_seed(0)
    raw = torch.randn((40, 1), requires_grad=True)
    opt = torch.optim.Adam([raw], lr=0.05, eps=1e-15)
    (torch.sigmoid(raw) ** 2).mean().backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    before = raw.detach().clone()
    alpha = torch.sigmoid(raw).reshape(1, 5, 8)
    loss = dr.alpha_penalty(alpha, torch.zeros((1, 5, 8), dtype=torch.bool))
    assert bool(loss.isnan())
    loss.backward()
    assert raw.grad is not None and float(raw.grad.abs().max()) == 0.0   # zeros, not None: Adam steps this tensor
    opt.step()
    assert int(opt.state[raw]["step"]) == 2
    assert float((raw.detach() - before).abs().min()) > 0                # the first step's moments move every row


@pytest.mark.parametrize("H,W", dc.FILL_SIZES)
@pytest.mark.parametrize("kind", dc.MASK_KINDS)
def test_fill_and_penalty_in_fp32_lie_within_the_summation_bound_of_float64(H, W, kind):
    """the table the kernels are held to: the float32 restatement against its float64 twin, each within (n - 1) u sum|x| of
    it (any summation order in fp32) plus one rounding; the kernels' own bar, one ulp, is tests/test_gpu_dtu_kernels.py's"""
    mask = dc.fill_mask(H, W, kind)
    n, u = H * W, 2.0 ** -24
    x, a = dc.fill_image(H, W), dc.alpha_image(H, W)
    assert float(x.min()) >= 0 and float(a.min()) >= 0
    n_un, n_m = int((~mask).sum()), int(mask.sum())
    f32, f64 = dr.masked_mean_fill(x, mask), dr.masked_mean_fill(x.double(), mask)
    assert torch.equal(f32[~mask], x[~mask])
    if n_un == 0:
        assert bool(f32.isnan().all()) and bool(f64.isnan().all())
    elif n_m:
        m32, m64 = float(f32[mask][0]), float(f64[mask][0])
        print("fill %dx%d %-11s mean %.9g, fp32 - float64 = %.3e (ulp %.3e)" % (H, W, kind, m64, m32 - m64, dr.ulp(m64)))
        assert abs(m32 - m64) <= (n_un * u + u) * m64 + dr.ulp(m64)
    p32, p64 = dr.alpha_penalty(a, mask), dr.alpha_penalty(a.double(), mask)
    if n_m == 0:
        assert bool(p32.isnan()) and bool(p64.isnan())
    else:
        print("penalty %dx%d %-11s loss %.9g, fp32 - float64 = %.3e (ulp %.3e)" % (H, W, kind, float(p64), float(p32) - float(p64),
                                                                                  dr.ulp(p64)))
        assert abs(float(p32) - float(p64)) <= ((n_m + 1) * u + u) * float(p64) + dr.ulp(p64)
    assert n <= 2 ** 21   # the kernels' bound: float64 accumulation of n <= 2^21 fp32 terms errs by at most n 2^-53


def test_the_fill_backward_drops_the_masked_cotangent_and_nothing_flows_through_the_mean():
    H, W = 7, 5
    mask = dc.fill_mask(H, W, "half")
    x = dc.fill_image(H, W).requires_grad_(True)
    g = torch.randn((1, H, W))
    dr.masked_mean_fill(x, mask).backward(g)
    assert torch.equal(x.grad[~mask], g[~mask]) and float(x.grad[mask].abs().max()) == 0.0


@pytest.mark.parametrize("P", dc.RULE_P)
def test_the_rule_rows_sit_on_both_thresholds(P):
    colour, stat, opacity = dc.rule_rows(P)
    for black, white in dc.RULE_FORMS:
        s, o = stat.clone(), opacity.clone()
        nb, nw = dr.colour_rules(colour, s, o, black, white, dr.reset_value())
        assert (black is not None or nb == 0) and (white is not None or nw == 0)
        changed = (s != stat).reshape(-1)
        fired = torch.zeros((P,), dtype=torch.bool)
        if black is not None:
            fired |= colour.max(-1).values < black[0]
        if white is not None:
            fired |= colour.min(-1).values > white[0]
        assert torch.equal(changed, fired & (stat.reshape(-1) != 0))
    if P >= 64:
        mx, mn = colour.max(-1).values, colour.min(-1).values
        for thr, v in ((20 / 255, mx), (240 / 255, mn)):
            for e in dc.around(thr):
                assert bool((v == e).any()), (thr, e)
        nb, nw = dr.colour_rules(colour, stat.clone(), opacity.clone(), *dc.RULE_FORMS[0], dr.reset_value())
        assert nb > 0 and nw > 0 and nb + nw < P


def test_the_reset_value_is_torchs_fp32_inverse_sigmoid():
    v = dr.reset_value(0.1)
    assert v == float(torch.log(torch.tensor(0.1) / (1 - torch.tensor(0.1))))
    assert abs(v - (-2.1972245773362196)) < 1e-6


def test_the_entry_points_are_declared_everywhere():
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gsplat.h")).read(), flags=re.S)
    for name in ("dtu_mask", "masked_tmp_bytes", "masked_fill_fwd", "masked_fill_bwd", "alpha_penalty_fwd", "alpha_penalty_bwd",
                 "dng_colour_rule"):
        assert name in PROTOTYPES and name in DEVICE_ONLY, name
        decl = re.search(r"\bgs_%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl and len(decl.group(1).split(",")) == len(PROTOTYPES[name][1]), name
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)   # additive: the ABI number stays
    makefile = open(os.path.join(root, "sparse-view-3dgs-pack_amd", "csrc", "Makefile")).read()
    assert re.search(r"gs_dng_dtu\.o: gs_dng_dtu\.hip \$\(HDRS\)\n\t\$\(HIPCC\) \$\(STRICT\)", makefile)


def test_the_public_names_and_their_argument_checks():
    import dng_loss
    import dng_reg
    from gsplat_amd import dng_dtu
    assert dng_loss.dtu_background_mask is dng_dtu.dtu_background_mask and dng_loss.masked_mean_fill is dng_dtu.masked_mean_fill
    assert dng_loss.alpha_penalty is dng_dtu.alpha_penalty and dng_reg.colour_rule is dng_dtu.colour_rule
    assert dng_dtu.reset_value(0.1) == dr.reset_value(0.1)
    with pytest.raises(ValueError, match=r"\[3,H,W\]"):
        dng_dtu.dtu_background_mask(torch.zeros((1, 4, 4)), 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_dtu.dtu_background_mask(torch.zeros((3, 4, 4)), 0.1)
    with pytest.raises(ValueError, match="elements"):
        dng_dtu.masked_mean_fill(torch.zeros((1, 4, 4)), torch.zeros((1, 4, 3), dtype=torch.bool))
    with pytest.raises(ValueError, match="bool"):
        dng_dtu.alpha_penalty(torch.zeros((1, 4, 4)), torch.zeros((1, 4, 4)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_dtu.alpha_penalty(torch.zeros((1, 4, 4)), torch.zeros((1, 4, 4), dtype=torch.bool))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        dng_dtu.colour_rule(torch.zeros((4, 2)), torch.zeros((4, 1)), torch.zeros((4, 1)))
    with pytest.raises(ValueError, match="divisor"):
        dng_dtu.colour_rule(torch.zeros((4, 3)), torch.zeros((4, 1)), torch.zeros((4, 1)), black=(0.1, 0, True))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_dtu.colour_rule(torch.zeros((4, 3)), torch.zeros((4, 1)), torch.zeros((4, 1)), black=(0.1, 10, True))
