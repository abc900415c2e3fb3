"""Every input form the per-Gaussian kernels accept (tests/form_cases.py), HIP against the CPU checker - which
tests/test_form_cases_cpu.py holds to the float64 model in each of these forms first.

Per form and list mode (GsView.tile_cull = 0, 1, 2; region mode in its cooperative form): the per-Gaussian state bit for
bit, the binning state bit for bit on the reference's lists, image / final_T / inverse depth and the gradients by
tests/test_gpu_raster_parity.py's procedure and bars (compare_forward, flip_mask, helpers.check_grads at helpers.TOL with the
cotangent zeroed on flipped pixels).  The split call (dc= / shs=) against the concatenated HIP call bit for bit AND against
the checker's concatenated gradients; the FSGS generation by tests/test_gpu_fsgs.py's procedure; the depth pass under a scale
modifier by tests/test_gpu_depth_pass.py's yardstick.  What is pinned here and nowhere else on the HIP side: generic row
counts M (1, 4, 9, 25) against an independent reference, a scale modifier != 1 on own scales and rotations (forward,
chain_from_row, the depth pass's copy of the chain, dL_dscales without the factor), SH colour with a given covariance,
precomputed colour with own scales, and non-zero inactive rows at low degrees."""
import pytest
import torch

import dc_cases
import depth_pass_reference as dpr
import dgr_fsgs
import diff_gaussian_rasterization as dgr
import form_cases
from helpers import TOL, check_grads, run_scene
from test_gpu_depth_pass import _bit_identical, run_pass
from test_gpu_rasterizer_dc import _poison
from test_gpu_raster_parity import compare_forward, flip_mask, forward_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CPU = torch.device("cpu")
BG = form_cases.BG
MODES = {0: (False, "lsd"), 1: (True, "lsd"), 2: (True, "region")}   # GsView.tile_cull -> RasterBackend (tile_cull, binning)


@pytest.fixture(autouse=True)
def backend_state(hip):
    names = ("tile_cull", "binning", "depth_limit_on", "_capacity_hint", "_capacity_hint_limited")
    old = {k: getattr(hip, k) for k in names}
    coop = hip.region_coop
    hip.depth_limit_on = False
    hip.region_coop = True
    hip._cam_cache.clear()
    hip._region_off.clear()
    yield
    for k, v in old.items():
        setattr(hip, k, v)
    hip.region_coop = coop
    hip._cam_cache.clear()
    hip._region_off.clear()


_ORACLE_STATE, _ORACLE_RUN = {}, {}


def oracle_state(oracle, form):
    if form["id"] not in _ORACLE_STATE:
        sc, cam = form_cases.build(form)
        _ORACLE_STATE[form["id"]] = forward_state(oracle.backend, sc, cam, CPU, BG, form["aa"])
    return _ORACLE_STATE[form["id"]]


def oracle_run(oracle, form, keep):
    """the checker's gradients under the form's cotangents x keep (cached for the usual case: no pixel flipped)"""
    key = form["id"] if bool(keep.all()) else None
    if key is None or key not in _ORACLE_RUN:
        sc, cam = form_cases.build(form)
        dc, di = masked(form, keep)
        r = run_scene(oracle.Rasterizer, oracle.Settings, sc, cam, CPU, bg=BG, antialiasing=form["aa"], dL_dcolor=dc, dL_dinvdepth=di)
        if key is None:
            return r
        _ORACLE_RUN[key] = r
    return _ORACLE_RUN[key]


def masked(form, keep):
    dc, di = form_cases.cotangents(form)
    k = keep.float()
    return dc * k, (None if di is None else di * k)


def hip_run(form, sc, cam, keep):
    dc, di = masked(form, keep)
    return run_scene(dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, sc, cam, DEV, bg=BG, antialiasing=form["aa"],
                     dL_dcolor=dc, dL_dinvdepth=di)


def check_sh_rows(g, radii, form, what):
    """dL_dsh [P,M,3]: every row written, zero for a culled Gaussian, zero above the active degree"""
    g, radii = g.cpu(), radii.cpu()
    assert tuple(g.shape) == (form["P"], form["M"], 3), what
    assert bool(torch.isfinite(g).all()), "%s: dL_dsh has rows the kernel did not write" % what
    assert not g[radii == 0].any(), "%s: dL_dsh of a culled Gaussian is not zero" % what
    assert not g[:, (form["D"] + 1) ** 2:, :].any(), "%s: rows above the active degree take a gradient" % what
    if int((radii > 0).sum()) >= 25:
        assert float(g[:, :(form["D"] + 1) ** 2, :].abs().amax(dim=(0, 2)).min()) > 0, "%s: an active row takes no gradient" % what


@pytest.mark.parametrize("cull", [0, 1, 2], ids=["lists_reference", "lists_culled_lsd", "lists_culled_region"])
@pytest.mark.parametrize("form", form_cases.UNSPLIT, ids=lambda f: f["id"])
def test_form_matches_oracle(hip, oracle, form, cull):
    sc, cam = form_cases.build(form)
    hip.tile_cull, hip.binning = MODES[cull]
    name = "form_%s_cull%d" % (form["id"], cull)
    h = forward_state(hip, sc, cam, DEV, BG, form["aa"])
    assert int(hip._last.view.tile_cull) == cull, "the forward took another list mode"
    o = oracle_state(oracle, form)
    info = compare_forward(h, o, name, form_cases.skipped_state(form), culled=cull > 0)
    visible = int((o["radii"] > 0).sum())
    print(name, "visible %d of %d, R=%d" % (visible, form["P"], h["num_rendered"]), info)
    keep = ~flip_mask(h, o)
    if not form["colors"]:
        _poison(DEV, form["P"], form["M"] - 1)
    ho = hip_run(form, sc, cam, keep)
    oo = oracle_run(oracle, form, keep)
    assert torch.equal(ho["radii"].cpu(), oo["radii"])
    hg = {k: v.cpu() for k, v in ho["grads"].items()}
    assert set(hg) == set(oo["grads"])
    check_grads(hg, oo["grads"], name)
    assert float(hg["means2D"][:, 2].abs().max()) == 0.0
    if not form["colors"]:
        check_sh_rows(hg["shs"], ho["radii"], form, name)
    if form["twin"]:   # both inputs precomputed: the modifier reaches nothing, the modifier-1 run has the same bits
        tw = form["twin"]
        tsc, tcam = form_cases.build(tw)
        t = forward_state(hip, tsc, tcam, DEV, BG, tw["aa"])
        for k in ("color", "invdepth", "final_T", "radii", "n_contrib", "depths", "means2D", "conic_opacity", "point_list"):
            assert dc_cases.same_bits(h[k], t[k]), "%s: %s moves with the modifier" % (name, k)
        to = hip_run(tw, tsc, tcam, keep)
        for k in hg:
            assert dc_cases.same_bits(hg[k], to["grads"][k].cpu()), "%s: dL_d%s moves with the modifier" % (name, k)


@pytest.mark.parametrize("cull", [0, 2], ids=["lists_reference", "lists_culled_region"])
@pytest.mark.parametrize("form", form_cases.SPLIT, ids=lambda f: f["id"])
def test_split_form_is_the_concatenated_call_and_matches_oracle(hip, oracle, form, cull):
    from gsplat_amd import accel
    sc, cam = form_cases.build(form)
    hip.tile_cull, hip.binning = MODES[cull]
    name = "form_%s_cull%d" % (form["id"], cull)
    h = forward_state(hip, sc, cam, DEV, BG, form["aa"])
    o = oracle_state(oracle, form)
    compare_forward(h, o, name, culled=cull > 0)
    keep = ~flip_mask(h, o)
    dc, di = masked(form, keep)
    cat = hip_run(form, sc, cam, keep)
    _poison(DEV, form["P"], form["M"] - 1)
    split = form_cases.run_split(accel.GaussianRasterizer, accel.GaussianRasterizationSettings, sc, cam, DEV, BG, form["aa"], dc, di)
    assert tuple(split["grads"]["dc"].shape) == (form["P"], 1, 3) and tuple(split["grads"]["rest"].shape) == (form["P"], form["M"] - 1, 3)
    dc_cases.assert_same(form_cases.as_pair(split), form_cases.as_pair(cat), name)
    check_sh_rows(split["grads"]["shs"], split["radii"], form, name + " split")
    check_sh_rows(cat["grads"]["shs"], cat["radii"], form, name + " concatenated")
    oo = oracle_run(oracle, form, keep)
    hg = {k: v.cpu() for k, v in split["grads"].items() if k not in ("dc", "rest")}
    assert set(hg) == set(oo["grads"])
    check_grads(hg, oo["grads"], name)


# ---- the FSGS rasterizer generation ----------------------------------------------------------------------------------
@pytest.fixture(params=[True, False], ids=["productT", "readbackT"])
def exact_T(oracle, request):
    """tests/test_gpu_fsgs.py's fixture: the checker in both forms of T_final"""
    oracle.lib.gso_set_fsgs_exact_T(1 if request.param else 0)
    yield request.param
    oracle.lib.gso_set_fsgs_exact_T(0)


def fsgs_run(Rast, Settings, sc, cam, device, dL, conf):
    """tests/test_fsgs_cpu.py's fsgs_run for any input form: the scene's own leaves and scale modifier"""
    leaves = [k for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations") if sc.get(k) is not None]
    p = {k: sc[k].detach().clone().to(device).requires_grad_(True) for k in leaves}
    rs = Settings(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                  bg=BG.to(device), scale_modifier=sc["scale_modifier"], viewmatrix=cam.world_view_transform.to(device),
                  projmatrix=cam.full_proj_transform.to(device), sh_degree=sc["sh_degree"], campos=cam.camera_center.to(device),
                  prefiltered=False, debug=False, confidence=conf.to(device))
    m2 = torch.zeros_like(p["means3D"], requires_grad=True)
    color, radii, depth, alpha = Rast(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], shs=p.get("shs"),
                                          colors_precomp=p.get("colors_precomp"), scales=p["scales"], rotations=p["rotations"])
    ((color * dL[0].to(device)).sum() + (depth * dL[1].to(device)).sum() + (alpha * dL[2].to(device)).sum()).backward()
    g = {k: v.grad.detach().cpu() for k, v in p.items()}
    g["means2D"] = m2.grad.detach().cpu()
    return dict(color=color.detach().cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.cpu(), grads=g)


@pytest.mark.parametrize("cull", [False, True], ids=["lists_reference", "lists_culled"])
@pytest.mark.parametrize("form", form_cases.FSGS_FORMS, ids=lambda f: f["id"])
def test_fsgs_generation_form_matches_oracle(hip, oracle, exact_T, form, cull):
    hip.tile_cull = cull
    sc, cam = form_cases.build(form)
    P, W, H = form["P"], form["W"], form["H"]
    g = torch.Generator().manual_seed(3000 + form["seed"])
    dL = [torch.randn((3, H, W), generator=g), torch.randn((1, H, W), generator=g) * 0.3, torch.randn((1, H, W), generator=g)]
    conf = torch.rand((P, 1), generator=g)

    def both(dL):
        if not form["colors"]:
            _poison(DEV, P, form["M"] - 1)
        return (fsgs_run(dgr_fsgs.GaussianRasterizer, dgr_fsgs.GaussianRasterizationSettings, sc, cam, DEV, dL, conf),
                fsgs_run(oracle.FsgsRasterizer, oracle.FsgsSettings, sc, cam, CPU, dL, conf))
    h, o = both(dL)
    assert torch.equal(h["radii"], o["radii"])
    assert int((o["radii"] > 0).sum()) >= 25 and int((o["radii"] == 0).sum()) >= 25
    bad = torch.zeros((H, W), dtype=torch.bool)
    flip = torch.zeros((H, W), dtype=torch.bool)
    for k in ("color", "depth", "alpha"):
        e = (h[k] - o[k]).abs().amax(dim=0)
        bad |= e > TOL * max(1.0, float(o[k].abs().max()))
        flip |= e > 0.2 * TOL * max(1.0, float(o[k].abs().max()))
    print(form["id"], "pixels out of tolerance %d, flipped %d" % (int(bad.sum()), int(flip.sum())))
    assert int(bad.sum()) <= max(2, W * H // 20000)
    if bool(flip.any()):  # a threshold pixel took the other branch: compare gradients without it
        keep = (~flip).float()
        h, o = both([d * keep for d in dL])
    assert set(h["grads"]) == set(o["grads"])
    check_grads(h["grads"], o["grads"], "form_%s_cull%d_exactT%d" % (form["id"], int(cull), int(exact_T)),
                **({} if exact_T else dict(tol=5e-3, chain_tol=5e-3)))
    if not form["colors"]:
        check_sh_rows(h["grads"]["shs"], h["radii"], form, form["id"])


# ---- the depth pass under a scale modifier ---------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [False, True], ids=["lists_reference", "lists_culled"])
@pytest.mark.parametrize("mod", form_cases.DEPTH_MODIFIERS)
@pytest.mark.parametrize("name", form_cases.DEPTH_CASES)
def test_depth_pass_under_a_scale_modifier(hip, oracle, name, mod, cull):
    """tests/test_gpu_depth_pass.py's test 1 and test 2 on a constructed scene under a modifier (gs_depth_pass.hip's own copy of
    the covariance chain): depth and alpha within TOL of float64 on every pixel, the checker's radii, each gradient within
    max(TOL, 3 d_ref), and the bits of the general path."""
    hip.tile_cull = cull
    r = dpr.oracle_case(oracle, name, modifier=mod)
    case, sc, (dd, da), dn, dg = r["case"], r["scene"], r["cot"], r["dense"], r["dense_grads"]
    assert sc["scale_modifier"] == mod
    for grad in ("means", "opacity", "both"):
        h = run_pass(sc, case.cam, case.bg, dd, da, grad)
        assert torch.equal(h["radii"], r["oracle"]["radii"]), "radii differ"
        for k in ("depth", "alpha"):
            e = float((h[k].double() - dn[k]).abs().max()) / max(1.0, float(dn[k].abs().max()))
            print("form_depth", name, mod, grad, k, "%.2e" % e)
            assert e <= TOL, "%s mod %s %s: %s is %.3e from float64 on some pixel" % (name, mod, grad, k, e)
        assert set(h["grads"]) == set(dpr.FAMILY[grad])
        for k, g in h["grads"].items():
            d = dpr.distance(g, dg[k], k)
            bound = max(TOL, 3.0 * r["d_ref"][k])
            print("form_depth", name, mod, grad, k, "err %.2e  d_ref %.2e  bound %.2e" % (d, r["d_ref"][k], bound))
            assert d <= bound, "%s mod %s %s: dL_d%s is %.3e from float64, bound %.3e" % (name, mod, grad, k, d, bound)
    _bit_identical(sc, case.cam, case.bg, "%s mod %s" % (name, mod))
