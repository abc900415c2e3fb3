"""The blend kernels on the constructed scenes of tests/blend_cases.py, against the dense float64 model.

Every case clears the margin condition (blend_cases.margins, asserted by tests/test_blend_cases_cpu.py): no skip, stop or
clamp decision lies within 1e-3 of its threshold, so an fp32 implementation has no decision to flip and NOTHING is exempt
here: every inside pixel's last contributor equals the reference's, final_T / colour / inverse depth lie within
helpers.TOL of the float64 values on every pixel, and every gradient tensor goes through helpers.check_grads against the
float64 gradients with random, unmasked cotangents.  Each case runs on every list mode the product has (the reference's
lists with the per-entry CULL test, culled lists from the LSD path and from region binning), the stop cases also on a
camera's second, depth-limited visit, and all of them through the 4-channel (HAS_EXTRA) and FSGS instantiations in the
same three list modes.  Every output the forward writes is planted with a NaN pattern first (RasterBackend.output_fill for
colour / inverse depth / radii / extra, RasterBackend.scratch_fill for final_T and n_contrib): a pixel of a partial tile
that nobody wrote shows instead of inheriting the previous render's value.  The stop and quadrant cases also take one
fused train step (gs_backward_step) against the plain backward + gs_adam_step, bit for bit.
"""
import ctypes as C

import pytest
import torch

import blend_cases
import dense_reference
import diff_gaussian_rasterization as dgr
from helpers import TOL, canonical_lists, check_grads, run_scene
from test_gpu_raster_parity import BINNING_STATE, forward_state, last_contributor_id

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CPU = torch.device("cpu")
MODES = {"reference": (False, "lsd"), "culled_lsd": (True, "lsd"), "culled_region": (True, "region")}
STOP_CASES = [n for n in blend_cases.NAMES if n.startswith("stop_") or n.endswith("_stop128") or n.endswith("_inside_stop")]


NAN_BITS = 0x7FC0BEEF   # a quiet NaN with a payload (as an int32: a last contributor / radius no scene here can have)


def plant(kind, t):
    t.view(torch.int32).fill_(NAN_BITS)


def plant_image_state(kind, t):
    """RasterBackend.scratch_fill: final_T and n_contrib, the first two blocks of the image scratch (csrc/gs_common.h,
    img_view: N floats and N words, each rounded up to 256 bytes).  Everything behind them (ranges, tile order, region
    counters) and the other scratch buffers hold indices and are left as the allocator gave them.  Armed around forwards
    only: a backward reads n_contrib as a loop bound."""
    if kind == "img":
        t[: 2 * ((4 * plant_image_state.pixels + 255) // 256 * 256)].view(torch.int32).fill_(NAN_BITS)


def planted_forward_state(hip, case, **kw):
    """forward_state with final_T / n_contrib planted; asserts that every element of every output was written"""
    plant_image_state.pixels = case.W * case.H
    hip.scratch_fill = plant_image_state
    try:
        st = forward_state(hip, case.scene, case.cam, DEV, case.bg, False, **kw)
    finally:
        hip.scratch_fill = None
    for k in ("color", "invdepth", "final_T", "n_contrib", "radii"):
        assert not bool((st[k].contiguous().view(torch.int32) == NAN_BITS).any()), "%s: %s has elements nobody wrote" % (case.name, k)
    return st


def written(t, what):
    assert not bool((t.detach().contiguous().view(torch.int32) == NAN_BITS).any()), "%s has elements nobody wrote" % what
    return t


@pytest.fixture(autouse=True)
def backend_state(hip):
    names = ("tile_cull", "binning", "depth_limit_on", "_capacity_hint", "_capacity_hint_limited", "scratch_fill", "output_fill")
    old = {k: getattr(hip, k) for k in names}
    hip.depth_limit_on = False
    hip.output_fill = plant
    hip._cam_cache.clear()
    hip._region_off.clear()
    yield
    for k, v in old.items():
        setattr(hip, k, v)
    hip._cam_cache.clear()
    hip._region_off.clear()


@pytest.fixture(scope="module")
def reference():
    """name, which -> the float64 outputs and gradients (evaluated once per case: the host side dominates this file)"""
    return lambda name, which="scene": blend_cases.dense(blend_cases.build(name), which)


def check_forward(h, dn, case, tag):
    W, H = case.W, case.H
    got, want = last_contributor_id(h, W, H), dn["last_id"]
    assert torch.equal(got, want), "%s: last contributor differs on %d pixels, first at %s" % (
        tag, int((got != want).sum()), (got != want).nonzero()[0].tolist())
    errs = dict(final_T=float((h["final_T"].reshape(H, W).double() - dn["final_T"]).abs().max()),
                color=float((h["color"].double() - dn["color"]).abs().max()) / max(1.0, float(dn["color"].abs().max())),
                invdepth=float((h["invdepth"].double() - dn["invdepth"]).abs().max()) / max(1.0, float(dn["invdepth"].abs().max())))
    print("forward %s: %s" % (tag, {k: "%.1e" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v <= TOL, "%s: %s off by %.3e on some pixel (bar %.0e, no pixel exempt)" % (tag, k, v, TOL)


def reference_grads(hg, dg):
    og = {k: dg[k] for k in hg if k in dg}
    og["means2D"] = torch.cat([dg["ndc_probe"], torch.zeros_like(dg["ndc_probe"][:, :1])], dim=1)
    return og


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", blend_cases.NAMES)
def test_forward_and_gradients(hip, oracle, reference, name, mode):
    case = blend_cases.build(name)
    hip.tile_cull, hip.binning = MODES[mode]
    tag = "%s/%s" % (name, mode)
    dn, dg = reference(name)
    h = planted_forward_state(hip, case)
    if mode == "reference":   # the binning state, bit for bit against the oracle (as compare_forward does)
        o = forward_state(oracle.backend, case.scene, case.cam, CPU, case.bg, False)
        assert h["num_rendered"] == o["num_rendered"] == int(case.tile_len.sum())
        for k in ("radii",) + BINNING_STATE:
            assert torch.equal(h[k], o[k]), "%s: %s not bit-exact" % (tag, k)
        for k in ("depths", "means2D", "conic_opacity"):
            assert torch.equal(h[k].view(torch.int32), o[k].view(torch.int32)), "%s: %s not bit-exact" % (tag, k)
    else:
        assert h["num_rendered"] <= int(case.tile_len.sum())
        canonical_lists(h)
    check_forward(h, dn, case, tag)
    dc, di = blend_cases.cotangents(case)
    for which in ("scene", "scene_sr"):
        sc = getattr(case, which)
        if sc is None:    # (alpha_diagonal_corner: no scales + identity rotation describe its footprint)
            continue
        dg = reference(name, which)[1]
        r = run_scene(dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, sc, case.cam, DEV, bg=case.bg, dL_dcolor=dc,
                      dL_dinvdepth=di)
        written(r["color"], "color")
        written(r["invdepth"], "invdepth")
        assert float((r["color"].cpu().double() - dn["color"]).abs().max()) <= TOL * max(1.0, float(dn["color"].abs().max()))
        hg = {k: v.cpu() for k, v in r["grads"].items()}
        assert float(hg["means2D"][:, 2].abs().max()) == 0.0
        check_grads(hg, reference_grads(hg, dg), "blend_%s_%s" % (tag, which), scene=sc if which == "scene_sr" else None)


def tile_stop_depths(hip, P, W, H, R, bufs):
    s = hip._scratch(bufs["geom"], bufs["img"], bufs["binning"], hip._capacity_for(bufs["binning"], P, W, H, R))
    out = torch.empty((int(hip.api.raw("tile_depth_limit_floats")(W, H)),), dtype=torch.float32, device=DEV)
    hip.api.call("export_tile_stop_depth", C.byref(s), W, H, out.data_ptr(), hip._stream(DEV))
    torch.cuda.synchronize()
    return out.cpu()[: ((W + 15) // 16) * ((H + 15) // 16)]


@pytest.mark.parametrize("binning", ["lsd", "region"])
@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_cases_on_depth_limited_lists(hip, reference, name, binning):
    """A camera's second visit: the lists are cut behind the depth at which each tile stopped.  The exported stop depth of
    a saturated tile is the view depth of entry k (every tile of these cases stops at the same k, so the export's 3 x 3
    maximum is that number too), the cut lists still hold entries 1 .. k in order, and the image is the float64 image."""
    case = blend_cases.build(name)
    W, H, P = case.W, case.H, case.scene["means3D"].shape[0]
    hip.tile_cull, hip.binning, hip.depth_limit_on = True, binning, True
    hip._cam_cache.clear()
    dn, _ = reference(name)
    k = set(case.meta["stop"].values())
    assert len(k) == 1
    k = k.pop()
    used0 = hip.depth_limit_stats["used"]
    bufs = {}
    full = planted_forward_state(hip, case, buffers=bufs)
    assert hip.depth_limit_stats["used"] == used0
    stop = tile_stop_depths(hip, P, W, H, full["num_rendered"], bufs)
    want = full["depths"][k - 1]
    assert torch.equal(stop.view(torch.int32), want.view(torch.int32).expand_as(stop)), (stop.tolist(), float(want))
    check_forward(full, dn, case, "%s/%s/first_visit" % (name, binning))
    cut = planted_forward_state(hip, case)
    assert hip.depth_limit_stats["used"] == used0 + 1 and hip.last_status()[2] == 0
    assert cut["num_rendered"] < full["num_rendered"]
    check_forward(cut, dn, case, "%s/%s/second_visit" % (name, binning))
    for key in ("color", "invdepth", "final_T"):
        assert torch.equal(cut[key], full[key]), key
    cf, kf = canonical_lists(full)
    cc, kc = canonical_lists(cut)
    first_f, first_c = cf.cumsum() - cf, cc.cumsum() - cc
    for t in range(len(cf)):
        lf, lc = (kf[first_f[t]:first_f[t] + cf[t]] & 0xFFFFFFFF).tolist(), (kc[first_c[t]:first_c[t] + cc[t]] & 0xFFFFFFFF).tolist()
        upto = lf.index(k - 1) + 1
        assert lc[:upto] == lf[:upto] and len(lc) < len(lf), "tile %d: the cut list lost or reordered an entry up to the stop" % t
    dc, di = blend_cases.cotangents(case)
    r = run_scene(dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, case.scene, case.cam, DEV, bg=case.bg, dL_dcolor=dc,
                  dL_dinvdepth=di)
    assert hip.depth_limit_stats["used"] == used0 + 2
    hg = {k_: v.cpu() for k_, v in r["grads"].items()}
    check_grads(hg, reference_grads(hg, reference(name)[1]), "blend_%s_%s_limited" % (name, binning))


_EXTRA = {}


def extra_reference(case):
    """float64: colour, the 4th channel (the extra value blended with the same weights, over bg[0]) and the gradients of
    sum(colour dc) + sum(extra_img dn)"""
    if case.name not in _EXTRA:
        P = case.scene["means3D"].shape[0]
        g = torch.Generator().manual_seed(77)
        extra = torch.rand((P,), generator=g)
        dc, _ = blend_cases.cotangents(case)
        dn = torch.randn((1, case.H, case.W), generator=g)
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
        leaves["extra"] = extra.double().clone().requires_grad_(True)
        leaves["ndc_probe"] = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
        d = dict(case.scene, **{k: v for k, v in leaves.items() if k != "extra"})
        a = dense_reference.render(d, case.cam, case.bg, False)
        b = dense_reference.render(dict(d, colors_precomp=leaves["extra"][:, None].repeat(1, 3)), case.cam, case.bg, False)
        ((a["color"] * dc.double()).sum() + (b["color"][0:1] * dn.double()).sum()).backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
        _EXTRA[case.name] = (extra, dn, a["color"].detach(), b["color"][0:1].detach(), grads)
    return _EXTRA[case.name]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", blend_cases.NAMES)
def test_four_channel_pass(hip, name, mode):
    """HAS_EXTRA forward and backward (gsplat_amd.nir.GaussianRasterizerX, as tests/test_gpu_nir.py drives it): the extra
    channel against the same float64 weights"""
    from gsplat_amd.nir import GaussianRasterizerX
    from helpers import settings_for
    case = blend_cases.build(name)
    hip.tile_cull, hip.binning = MODES[mode]
    extra, dn, want_rgb, want_x, dg = extra_reference(case)
    dc, _ = blend_cases.cotangents(case)
    p = {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
    xp = extra.clone().to(DEV).requires_grad_(True)
    m2 = torch.zeros_like(p["means3D"], requires_grad=True)
    rs = settings_for(dgr.GaussianRasterizationSettings, case.cam, case.bg, 0, DEV)
    rgb, radii, invd, ximg = GaussianRasterizerX(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], extra=xp,
                                                      colors_precomp=p["colors_precomp"], cov3D_precomp=p["cov3D_precomp"])
    for t, what in ((rgb, "color"), (invd, "invdepth"), (ximg, "extra"), (radii, "radii")):
        written(t, what)
    ((rgb * dc.to(DEV)).sum() + (ximg * dn.to(DEV)).sum()).backward()
    assert float((rgb.detach().cpu().double() - want_rgb).abs().max()) <= TOL * max(1.0, float(want_rgb.abs().max()))
    assert float((ximg.detach().cpu().double() - want_x).abs().max()) <= TOL, "extra channel"
    hg = {k: (v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()) for k, v in p.items()}
    hg["extra"] = xp.grad.cpu()
    hg["means2D"] = m2.grad.cpu()
    check_grads(hg, reference_grads(hg, dg), "blend_%s_%s_extra" % (name, mode))


_FSGS = {}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", blend_cases.NAMES)
def test_fsgs_generation(hip, name, mode):
    """dgr_fsgs (the FSGS instantiation of the blend kernels): colour, depth = sum depth alpha T and alpha = sum alpha T
    against dense_reference's `depth` / `alpha`, and the gradients of all three"""
    import dgr_fsgs
    case = blend_cases.build(name)
    hip.tile_cull, hip.binning = MODES[mode]
    W, H, P = case.W, case.H, case.scene["means3D"].shape[0]
    dc, dd = blend_cases.cotangents(case)
    da = torch.randn((1, H, W), generator=torch.Generator().manual_seed(78))
    if name not in _FSGS:
        leaves = {k: v.double().clone().requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
        leaves["ndc_probe"] = torch.zeros((P, 2), dtype=torch.float64, requires_grad=True)
        out = dense_reference.render(dict(case.scene, **leaves), case.cam, case.bg, False)
        ((out["color"] * dc.double()).sum() + (out["depth"] * dd.double()).sum() + (out["alpha"] * da.double()).sum()).backward()
        _FSGS[name] = ({k: out[k].detach() for k in ("color", "depth", "alpha")},
                       {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
    want, dg = _FSGS[name]
    cam = case.cam
    p = {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in case.scene.items() if torch.is_tensor(v)}
    m2 = torch.zeros_like(p["means3D"], requires_grad=True)
    rs = dgr_fsgs.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=case.bg.to(DEV), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV), sh_degree=0,
        campos=cam.camera_center.to(DEV), prefiltered=False, debug=False, confidence=torch.ones((P, 1), device=DEV))
    color, radii, depth, alpha = dgr_fsgs.GaussianRasterizer(rs)(
        means3D=p["means3D"], means2D=m2, opacities=p["opacities"], colors_precomp=p["colors_precomp"],
        cov3D_precomp=p["cov3D_precomp"])
    for t, what in ((color, "color"), (depth, "depth"), (alpha, "alpha"), (radii, "radii")):
        written(t, what)
    ((color * dc.to(DEV)).sum() + (depth * dd.to(DEV)).sum() + (alpha * da.to(DEV)).sum()).backward()
    for k, v in (("color", color), ("depth", depth), ("alpha", alpha)):
        e = float((v.detach().cpu().double().reshape(want[k].shape) - want[k]).abs().max()) / max(1.0, float(want[k].abs().max()))
        assert e <= TOL, "%s/%s: %s off by %.3e" % (name, mode, k, e)
    hg = {k: (v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()) for k, v in p.items()}
    hg["means2D"] = m2.grad.cpu()
    check_grads(hg, reference_grads(hg, dg), "blend_%s_%s_fsgs" % (name, mode))


FUSED_CASES = STOP_CASES + [n for n in blend_cases.NAMES if n.startswith("quad_")]


def fused_trainer(hip, case, fused):
    """tests/test_gpu_fused_step.py's harness on a constructed scene: the scales + identity rotation form, the colours as
    degree-0 SH rows, one camera, a random target.  The criterion is L1 + SSIM only: the DWT / patch terms have nothing to
    do with the rasterizer's backward and their kernels were never meant for 16x16 images."""
    import lgdwt_loss
    from gsplat_amd.trainer import GaussianModelLite, Trainer, camera_to
    sc = {k: v for k, v in case.scene_sr.items() if k != "colors_precomp"}
    P = sc["means3D"].shape[0]
    shs = torch.zeros((P, 16, 3))
    shs[:, 0] = (case.scene_sr["colors_precomp"] - 0.5) / dense_reference.SH_C0
    sc["shs"], sc["sh_degree"] = shs, 0
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, case.H, case.W), generator=g).to(DEV)]
    model = GaussianModelLite(sc, DEV, api=hip.api, spatial_order=False)
    crit = lgdwt_loss.criterion(dwt_enable=False, patch_dwt_enable=False)
    tr = Trainer(model, [camera_to(case.cam, DEV)], gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings,
                 case.bg.to(DEV), optimizer_step=True)
    tr.FUSED_STEP = fused
    return tr


def trainer_state(tr):
    m, o = tr.model, tr.model.optimizer
    return dict(flat=m.flat.detach().clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
                accum=m.xyz_gradient_accum.clone(), denom=m.denom.clone(), max_radii=m.max_radii2D.clone())


@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_train_step(hip, name):
    """One gs_backward_step against the plain gradients + gs_adam_step on the same inputs, bit for bit, in the two forms of
    tests/test_gpu_fused_step.py: handed the plain backward's blend sums (the fused tail alone), and on its own blend sums.
    The second form is bit-exact too where one tile holds the image (one wave adds a Gaussian's sums in a fixed order); with
    several tiles their float64 atomics arrive in any order, which moves a sum by an ulp of float64 and its float32 image by
    at most one ulp (2^-23), carried through the few fp32 operations of the activation backward and the moment updates:
    2^-21 of the tensor's largest entry is the bar there, on the moments and statistics.  The parameters themselves are
    left out in that case only: Adam's first step is lr g / (|g| + 1e-15), which turns the SIGN of a sum that is zero up to
    rounding into a full step (the reason tests/test_gpu_fused_step.py compares whole runs by rms)."""
    case = blend_cases.build(name)
    hip.binning = "region"    # (pinned as in test_gpu_fused_step.py: the two runs of a comparison must share a path)
    hip.output_fill = None    # (the trainer's images are its own)
    a, b, c = fused_trainer(hip, case, False), fused_trainer(hip, case, True), fused_trainer(hip, case, True)
    assert torch.equal(a.model.flat, b.model.flat)
    start = a.model.flat.detach().clone()
    hip.keep_workspace = True
    try:
        a._step_camera(0, True, ())
        torch.cuda.synchronize()
        rows = hip.last_workspace[: a.model.P * 128].view(torch.float64).clone()
    finally:
        hip.keep_workspace, hip.last_workspace = False, None
    b.rows_override = rows
    b._step_camera(0, True, ())
    c._step_camera(0, True, ())
    torch.cuda.synchronize()
    sa, sb, sc_ = trainer_state(a), trainer_state(b), trainer_state(c)
    assert float((sa["flat"] - start).abs().max()) > 0 and float(sa["denom"].max()) == 1.0
    one_tile = case.W <= 16 and case.H <= 16
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (name, k, float((sa[k] - sb[k]).abs().max()))
        if one_tile:
            assert torch.equal(sa[k], sc_[k]), (name, k, "own blend sums", float((sa[k] - sc_[k]).abs().max()))
        elif k != "flat":
            assert float((sa[k] - sc_[k]).abs().max()) <= 2.0 ** -21 * float(sa[k].abs().max()), (name, k, "own blend sums")
    assert a.model.optimizer.t == b.model.optimizer.t == c.model.optimizer.t == 1
