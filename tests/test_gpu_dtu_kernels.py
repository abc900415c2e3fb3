"""The DTU kernels (csrc/gs_dng_dtu.hip through gsplat_amd/dng_dtu.py) on the GPU against tests/dtu_reference.py's torch
restatements on the CPU, over the case table of tests/dtu_cases.py (proven in tests/test_dtu_cpu.py): the mask, its count and
the zeroed image EXACT; the fill's mean and the penalty within one fp32 ulp of the float64 restatement (a float64 accumulation
of n <= 2^21 fp32 terms errs by at most n 2^-53 relative, then there is one rounding), the fill's unmasked pixels and its
backward bit for bit, the penalty's backward within 2 ulp per element (two fp32 roundings); the colour rules EXACT."""
import pytest
import torch

import dtu_cases as dc
import dtu_reference as dr
from gsplat_amd import dng_dtu, synthetic
from gsplat_amd.trainer import GaussianModelLite

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def spacing(t):
    """float32 ulp at |t|, per element (float64 tensor in, float64 out)"""
    a = t.abs().float()
    up = torch.nextafter(a, torch.full_like(a, float("inf")))
    return (up.double() - a.double())


# ---------------------------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("H,W", dc.MASK_SIZES)
@pytest.mark.parametrize("run", (1, 50))
def test_mask_count_and_zeroed_image_are_the_restatements(hip, H, W, run):
    for thr, kind in ((30 / 255, "runs"), (15 / 255, "runs"), (30 / 255, "dark"), (30 / 255, "bright")):
        gt = dc.mask_image(H, W, thr, kind)
        want_mask, want_gt = dr.background_mask(gt.clone(), thr, run)
        g = gt.to(DEV)
        mask, zeroed, count = dng_dtu.dtu_background_mask(g, thr, run, return_count=True)
        assert mask.dtype == torch.bool and mask.shape == (1, H, W) and zeroed.shape == (3, H, W)
        assert same_bits(g, gt)                                   # the separate output leaves the input alone
        assert torch.equal(mask.cpu(), want_mask), (thr, kind, int((mask.cpu() != want_mask).sum()))
        assert int(count[0]) == int(want_mask.sum()), (thr, kind)
        assert same_bits(zeroed, want_gt), (thr, kind)
        if kind == "dark":
            assert int(count[0]) == H * W
        if kind == "bright":
            assert int(count[0]) == 0
        # in place: the same bytes
        mask2, zeroed2, count2 = dng_dtu.dtu_background_mask(g, thr, run, out=g, return_count=True)
        assert zeroed2.data_ptr() == g.data_ptr()
        assert torch.equal(mask2, mask) and int(count2[0]) == int(count[0]) and same_bits(zeroed2, zeroed)
        # and the mask of the zeroed image is the same mask
        mask3, zeroed3 = dng_dtu.dtu_background_mask(zeroed, thr, run)
        assert torch.equal(mask3, mask) and same_bits(zeroed3, zeroed)


def test_mask_threshold_rows(hip):
    """the channel maximum at float32(thr) and at both neighbours, every pixel on its own (run = 1)"""
    for thr in dc.THRESHOLDS:
        x = torch.tensor(dc.around(thr), dtype=torch.float32)
        for c in range(3):
            gt = torch.stack([x * 0.5, x * 0.25, x * 0.125])
            gt[c] = x
            gt = gt.reshape(3, 1, 3).contiguous()
            mask, _ = dng_dtu.dtu_background_mask(gt.to(DEV), thr, 1)
            assert mask.reshape(-1).tolist() == [True, False, False] == dr.background_mask(gt.clone(), thr, 1)[0].reshape(-1).tolist()


# ---------------------------------------------------------------------------------------------------------------- fill
@pytest.mark.parametrize("H,W", dc.FILL_SIZES)
@pytest.mark.parametrize("kind", dc.MASK_KINDS)
def test_fill_forward_and_backward(hip, H, W, kind):
    mask, x = dc.fill_mask(H, W, kind), dc.fill_image(H, W)
    n_un = int((~mask).sum())
    xd = x.to(DEV).requires_grad_(True)
    out, mean = dng_dtu.masked_mean_fill(xd, mask.to(DEV), return_mean=True)
    assert out.shape == x.shape
    o = out.detach().cpu()
    assert same_bits(o[~mask], x[~mask])                          # unmasked pixels: bit for bit
    if n_un == 0:
        assert bool(o.isnan().all()) and bool(mean.isnan().all())
        assert bool(dr.masked_mean_fill(x.double(), mask).isnan().all())
    else:
        want = float(x.double()[~mask].mean())
        at = float(x.double()[~mask].abs().sum()) / n_un
        got = float(mean[0])
        print("fill %dx%d %-11s mean %.9g  kernel - float64 = %.3e  (ulp %.3e)" % (H, W, kind, want, got - want, dr.ulp(at)))
        assert abs(got - want) <= dr.ulp(at)
        if n_un < H * W:
            assert bool((bits(o[mask]) == bits(mean)[0]).all())   # every masked pixel holds that one value
    g = torch.randn((1, H, W), generator=torch.Generator().manual_seed(3))
    out.backward(g.to(DEV))
    gx = xd.grad.cpu()
    assert same_bits(gx[~mask], g[~mask])
    assert bool((bits(gx[mask]) == 0).all())                      # +0.0 by sign bit
    if kind == "half":                                            # the restatement's own backward says the same
        xr = x.clone().requires_grad_(True)
        dr.masked_mean_fill(xr, mask).backward(g)
        assert same_bits(gx, xr.grad)


# ---------------------------------------------------------------------------------------------------------------- penalty
@pytest.mark.parametrize("H,W", dc.FILL_SIZES)
@pytest.mark.parametrize("kind", dc.MASK_KINDS)
def test_penalty_forward_and_backward(hip, H, W, kind):
    mask, a = dc.fill_mask(H, W, kind), dc.alpha_image(H, W)
    n_m = int(mask.sum())
    ad = a.to(DEV).requires_grad_(True)
    loss = dng_dtu.alpha_penalty(ad, mask.to(DEV))
    assert loss.shape == ()
    gscale = 0.75
    (loss * gscale).backward()
    ga = ad.grad.cpu()
    if n_m == 0:
        assert bool(loss.isnan()) and bool(dr.alpha_penalty(a.double(), mask).isnan())
        assert bool((bits(ga) == 0).all())                        # exactly zero, every element
        return
    want = float(dr.alpha_penalty(a.double(), mask))
    got = float(loss.detach())
    print("penalty %dx%d %-11s loss %.9g  kernel - float64 = %.3e  (ulp %.3e)" % (H, W, kind, want, got - want, dr.ulp(want)))
    assert abs(got - want) <= dr.ulp(want)
    ref = torch.where(mask, (gscale / n_m) * (2.0 * a.double()), torch.zeros_like(a, dtype=torch.float64))
    err = (ga.double() - ref).abs()
    assert bool((err <= 2.0 * spacing(ref)).all()), float((err / spacing(ref)).max())
    assert bool((bits(ga[~mask]) == 0).all())
    # for the record, not asserted: is the backward torch's fp32 on the CPU, bit for bit?
    ar = a.clone().requires_grad_(True)
    (dr.alpha_penalty(ar, mask) * gscale).backward()
    print("penalty %dx%d %-11s backward bit-equal to torch's fp32 on the CPU: %s (%d of %d elements differ)"
          % (H, W, kind, same_bits(ga, ar.grad), int((bits(ga) != bits(ar.grad)).sum()), ga.numel()))


# ---------------------------------------------------------------------------------------------------------------- colour rule
@pytest.mark.parametrize("P", dc.RULE_P)
def test_colour_rule_rows_opacity_and_counts_are_the_restatements(hip, P):
    colour, stat, opacity = dc.rule_rows(P)
    value = dr.reset_value(0.1)
    assert value == dng_dtu.reset_value(0.1)
    for black, white in dc.RULE_FORMS:
        ws, wo = stat.clone(), opacity.clone()
        nb, nw = dr.colour_rules(colour, ws, wo, black, white, value)
        c, s, o = colour.to(DEV), stat.to(DEV), opacity.to(DEV)
        counts = dng_dtu.colour_rule(c, s, o, black=black, white=white, value=value)
        assert counts.dtype == torch.int32 and counts.tolist() == [nb, nw], (black, white, counts.tolist(), nb, nw)
        assert same_bits(s, ws), (black, white)
        assert same_bits(o, wo), (black, white)
        assert same_bits(c, colour)
    # the rows on the thresholds decide as torch does: [P] views of the same memory too
    s, o = stat.reshape(-1).to(DEV), opacity.reshape(-1).to(DEV)
    ws, wo = stat.clone(), opacity.clone()
    dr.colour_rules(colour, ws, wo, *dc.RULE_FORMS[0], value)
    dng_dtu.colour_rule(colour.to(DEV), s, o, *dc.RULE_FORMS[0])
    assert same_bits(s, ws.reshape(-1)) and same_bits(o, wo.reshape(-1))


def test_colour_rule_leaves_the_moments_of_a_flat_adam_alone(hip):
    P = 257
    sc = synthetic.trained_like(P, seed=4)
    m = GaussianModelLite(sc, DEV, api=hip.api)
    o = m.optimizer
    g = torch.Generator().manual_seed(8)
    o.exp_avg.copy_(torch.randn(o.exp_avg.shape, generator=g))
    o.exp_avg_sq.copy_(torch.rand(o.exp_avg_sq.shape, generator=g))
    m.xyz_gradient_accum.copy_(torch.rand((P, 1), generator=g))
    colour, _, _ = dc.rule_rows(P)
    before = dict(m=o.exp_avg.clone(), v=o.exp_avg_sq.clone(), flat=m.flat.detach().clone(), accum=m.xyz_gradient_accum.clone())
    raw = m.params["opacity"].detach()
    assert raw.data_ptr() == m.params["opacity"].data_ptr()
    counts = dng_dtu.colour_rule(colour.to(DEV), m.xyz_gradient_accum, raw, *dc.RULE_FORMS[0])
    assert min(counts.tolist()) > 0
    assert same_bits(o.exp_avg, before["m"]) and same_bits(o.exp_avg_sq, before["v"])
    ws, wo = before["accum"].cpu(), before["flat"].cpu()[51 * P:52 * P].reshape(P, 1).clone()
    dr.colour_rules(colour, ws, wo, *dc.RULE_FORMS[0], dr.reset_value(0.1))
    assert same_bits(m.xyz_gradient_accum, ws)
    want_flat = before["flat"].cpu().clone()
    want_flat[51 * P:52 * P] = wo.reshape(-1)
    assert same_bits(m.flat, want_flat)                           # the opacity rows alone moved
    assert int((bits(m.flat) != bits(before["flat"])).sum()) > 0
