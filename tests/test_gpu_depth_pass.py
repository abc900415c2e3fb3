"""The depth-only pass on the GPU (gsplat_amd.depth_pass over gs_depth_forward / gs_depth_backward, csrc/gs_depth_pass.hip):
against float64 on the constructed blend scenes, bit for bit against the general path it replaces, against the CPU checker
on random scenes, and its interface (float opacity, no interference with the general path's state, edge cases, status
codes, the two drop-in functions of dgr_dng).

Yardsticks: tests/depth_pass_reference.py - the reference's two compositions over a rasterizer class, the float64 model, and
d_ref, the CPU checker's own distance to float64 per case and tensor (never taken from the code under test)."""
import ctypes as C
import json
import os

import pytest
import torch

import blend_cases
import depth_pass_reference as dpr
import dgr_dng
from gsplat_amd import synthetic
from gsplat_amd.depth_pass import depth_pass
from helpers import TOL, check_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_CASES = [n for n in blend_cases.NAMES if n not in blend_cases.NO_SCALES_ROTATIONS]
MEASURED = {}


def _record(key, value):
    """every measured distance is printed where it is asserted; with GS_MEASURED_DIR set they are also kept as
    depth_pass_cases.json in that directory"""
    MEASURED[key] = value
    out = os.environ.get("GS_MEASURED_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump(MEASURED, open(os.path.join(out, "depth_pass_cases.json"), "w"), indent=1)
    except OSError:
        pass


@pytest.fixture(params=[False, True], ids=["lists_reference", "lists_culled"])
def cull(hip, request):
    old = hip.tile_cull
    hip.tile_cull = request.param
    yield request.param
    hip.tile_cull = old


def _settings(cam, bg, scale_modifier=1.0):
    return dgr_dng.GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg.to(DEV),
        scale_modifier=scale_modifier, viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV),
        sh_degree=0, campos=cam.camera_center.to(DEV), prefiltered=False, debug=False)


def run_pass(sc, cam, bg, dd, da, grad, opacity=None):
    """depth_pass on the GPU in the shape of dpr.reference_pass's result (CPU tensors)"""
    want = dpr.FAMILY[grad]
    means = sc["means3D"].detach().clone().to(DEV).requires_grad_(True)
    op = opacity if opacity is not None else sc["opacities"].detach().clone().to(DEV).requires_grad_(True)
    m2 = torch.zeros_like(means, requires_grad=True)
    shape = {k: sc[k].to(DEV) for k in ("scales", "rotations", "cov3D_precomp") if sc.get(k) is not None}
    depth, alpha, radii = depth_pass(_settings(cam, bg, sc.get("scale_modifier", 1.0)), means, op, grad=grad, means2D=m2, **shape)
    assert depth.shape == alpha.shape == (1, cam.image_height, cam.image_width) and radii.dtype == torch.int32
    out = dict(depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.cpu(), grads={})
    terms = [(img * d.to(DEV)).sum() for img, d in ((depth, dd), (alpha, da)) if d is not None]
    if want and terms:
        sum(terms).backward()
        leaves = dict(means3D=means, means2D=m2, opacities=op)
        for k in ("means3D", "means2D", "opacities"):
            leaf = leaves[k]
            if not torch.is_tensor(leaf):
                continue
            if k in want:
                assert leaf.grad is not None, k
                out["grads"][k] = leaf.grad.detach().cpu()
            else:   # the backward returns gradients only for what `grad` names
                assert leaf.grad is None, k
    else:
        assert not depth.requires_grad or not want
    return out


def general_pass(sc, cam, bg, dd, da, grad, opacity=None):
    """the parent's path: the reference composition through dgr_dng.GaussianRasterizer"""
    return dpr.reference_pass(dgr_dng.GaussianRasterizer, dgr_dng.GaussianRasterizationSettings, sc, cam, bg, DEV, dd, da, grad,
                              opacity=opacity)


# ---- 1. constructed scenes against float64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR_CASES)
def test_constructed_scenes_match_float64(hip, oracle, cull, name):
    """Every pixel of depth and alpha within helpers.TOL of float64, radii the checker's, every gradient tensor within
    max(helpers.TOL, 3 d_ref): d_ref is the CPU checker's distance to float64 on the same case and tensor (another fp32
    realisation of the cancellation that colour 1 puts into dL_dalpha), 3 the allowance for a second, independent one."""
    r = dpr.oracle_case(oracle, name)
    case, (dd, da), dn, dg = r["case"], r["cot"], r["dense"], r["dense_grads"]
    rec = {}
    for grad in ("means", "opacity", "both"):
        h = run_pass(case.scene_sr, case.cam, case.bg, dd, da, grad)
        assert torch.equal(h["radii"], r["oracle"]["radii"]), "radii differ"
        for k in ("depth", "alpha"):
            e = float((h[k].double() - dn[k]).abs().max()) / max(1.0, float(dn[k].abs().max()))
            rec["%s/%s" % (grad, k)] = e
            print(name, grad, k, "%.2e" % e)
            assert e <= TOL, "%s %s: %s is %.3e from float64 on some pixel" % (name, grad, k, e)
        assert set(h["grads"]) == set(dpr.FAMILY[grad])
        for k, g in h["grads"].items():
            d = dpr.distance(g, dg[k], k)
            bound = max(TOL, 3.0 * r["d_ref"][k])
            rec["%s/d%s" % (grad, k)] = dict(err=d, d_ref=r["d_ref"][k], bound=bound)
            print(name, grad, k, "err %.2e  d_ref %.2e  bound %.2e" % (d, r["d_ref"][k], bound))
            assert d <= bound, "%s %s: dL_d%s is %.3e from float64, bound %.3e" % (name, grad, k, d, bound)
    _record("%s/cull%d" % (name, int(cull)), rec)


# ---- 2. bit identity with the general path ---------------------------------------------------------------------------
RANDOM = {"trained_8000": ("trained", 8000, 320, 240), "init_10000": ("init", 10000, 400, 400),
          "trained_30000": ("trained", 30000, 640, 360)}
_SCENES = {}


def random_scene(key):
    if key not in _SCENES:
        kind, P, W, H = RANDOM[key]
        sc = (synthetic.init_like if kind == "init" else synthetic.trained_like)(P, seed=6, sh_degree=0)
        sc = {k: sc[k] for k in ("means3D", "opacities", "scales", "rotations")}
        _SCENES[key] = (sc, synthetic.orbit_cameras(W, H)[5], torch.tensor([0.3, 0.6, 0.1]))
    return _SCENES[key]


def _bit_identical(sc, cam, bg, what):
    for opacity in (0.95, None):
        h = run_pass(sc, cam, bg, None, None, None, opacity=opacity)
        g = general_pass(sc, cam, bg, None, None, None, opacity=opacity)
        for k in ("depth", "alpha", "radii"):
            assert torch.equal(h[k], g[k]), "%s, opacity %s: %s differs from the general path in %d elements (max %.3e)" % (
                what, opacity, k, int((h[k] != g[k]).sum()), float((h[k].double() - g[k].double()).abs().max()))


@pytest.mark.parametrize("name", SR_CASES)
def test_bit_identical_to_general_path_constructed(hip, cull, name):
    case = blend_cases.build(name)
    _bit_identical(case.scene_sr, case.cam, case.bg, name)


@pytest.mark.parametrize("key", list(RANDOM))
def test_bit_identical_to_general_path_random(hip, cull, key):
    _bit_identical(*random_scene(key), key)


# ---- 3. random scenes against the CPU checker ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["hard", "soft"])
@pytest.mark.parametrize("key", list(RANDOM))
def test_random_scenes_match_oracle(hip, oracle, key, mode):
    """tests/test_gpu_fsgs.py's protocol: its TOL, its cap on out-of-tolerance pixels, its re-run without threshold-flip
    pixels, check_grads on the family the pass produces.  Control: the general path stays within the cap on the same
    inputs (if it does not, the inputs are at fault, not the pass)."""
    sc, cam, bg = random_scene(key)
    W, H = cam.image_width, cam.image_height
    opacity, grad = (0.95, "means") if mode == "hard" else (None, "opacity")
    dd, da = dpr.cotangents(H, W, 2)

    def three(dd, da):
        h = run_pass(sc, cam, bg, dd, da, grad, opacity=opacity)
        c = general_pass(sc, cam, bg, dd, da, grad, opacity=opacity)
        with dpr.exact_T(oracle):
            o = dpr.reference_pass(oracle.FsgsRasterizer, oracle.FsgsSettings, sc, cam, bg, CPU, dd, da, grad, opacity=opacity)
        return h, c, o
    h, c, o = three(dd, da)
    assert torch.equal(h["radii"], o["radii"])
    cap = max(2, W * H // 20000)
    flip = torch.zeros((H, W), dtype=torch.bool)
    for who, r in (("control", c), ("depth_pass", h)):
        bad = torch.zeros((H, W), dtype=torch.bool)
        for k in ("depth", "alpha"):
            e = (r[k] - o[k]).abs().amax(dim=0)
            bad |= e > TOL * max(1.0, float(o[k].abs().max()))
            flip |= e > 0.2 * TOL * max(1.0, float(o[k].abs().max()))
        print(key, mode, who, "pixels out of tolerance:", int(bad.sum()), "cap", cap)
        assert int(bad.sum()) <= cap, "%s: %d pixels out of tolerance" % (who, int(bad.sum()))
    if bool(flip.any()):   # a threshold pixel took the other branch: compare gradients without it
        keep = (~flip).float()
        h, c, o = three(dd * keep, da * keep)
    check_grads(h["grads"], o["grads"], "depth_pass_%s_%s" % (key, mode))


# ---- 4. float opacity ---------------------------------------------------------------------------------------------------
def test_float_opacity_is_the_filled_tensor(hip):
    sc, cam, bg = random_scene("trained_8000")
    dd, da = dpr.cotangents(cam.image_height, cam.image_width, 4)
    a = run_pass(sc, cam, bg, dd, da, "means", opacity=0.95)
    filled = dict(sc, opacities=torch.full((sc["means3D"].shape[0], 1), 0.95))
    b = run_pass(filled, cam, bg, dd, da, "means")
    for k in ("depth", "alpha", "radii"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["grads"]["means3D"], b["grads"]["means3D"])
    from gsplat_amd import depth_pass as mod
    n = len(mod._filled)
    run_pass(sc, cam, bg, None, None, None, opacity=0.95)
    assert len(mod._filled) == n    # the constant's tensor is kept per (device, P, value)


# ---- 5. no interference with the general path's state -----------------------------------------------------------------
def test_interleaved_pass_leaves_the_general_path_alone(hip):
    sc = synthetic.trained_like(4000, seed=9, sh_degree=2)
    cam = synthetic.orbit_cameras(256, 192)[4]
    H, W = 192, 256
    g = torch.Generator().manual_seed(0)
    dL = [torch.randn((3, H, W), generator=g).to(DEV), torch.randn((1, H, W), generator=g).to(DEV), torch.randn((1, H, W), generator=g).to(DEV)]
    leaves_of = ("means3D", "opacities", "shs", "scales", "rotations")
    sm = {k: sc[k] for k in ("means3D", "opacities", "scales", "rotations")}

    def general(interleave):
        p = {k: sc[k].detach().clone().to(DEV).requires_grad_(True) for k in leaves_of}
        m2 = torch.zeros_like(p["means3D"], requires_grad=True)
        rs = _settings(cam, torch.zeros(3))._replace(sh_degree=2)
        color, radii, depth, alpha = dgr_dng.GaussianRasterizer(rs)(means3D=p["means3D"], means2D=m2, opacities=p["opacities"],
                                                                    shs=p["shs"], scales=p["scales"], rotations=p["rotations"])
        if interleave:
            last, arena, step = hip._last, hip.grad_arena, hip.fused_step
            cams = {k: (id(v), v["order_ok"], v["limit_ok"]) for k, v in hip._cam_cache.items()}
            dd, da = dpr.cotangents(H, W, 8)
            run_pass(sm, cam, torch.zeros(3), dd, da, "both")
            run_pass(sm, cam, torch.zeros(3), dd, da, "means", opacity=0.95)
            assert hip._last is last and hip.grad_arena is arena and hip.fused_step is step
            assert cams == {k: (id(v), v["order_ok"], v["limit_ok"]) for k, v in hip._cam_cache.items()}
        ((color * dL[0]).sum() + (depth * dL[1]).sum() + (alpha * dL[2]).sum()).backward()
        out = {k: v.grad.detach().cpu() for k, v in p.items()}
        out["means2D"] = m2.grad.detach().cpu()
        return (color.detach().cpu(), depth.detach().cpu(), alpha.detach().cpu()), out
    img_a, a = general(False)
    img_b, b = general(True)
    for x, y in zip(img_a, img_b):
        assert torch.equal(x, y)
    for k in a:   # same kernels, different atomic order between the two runs (tests/test_gpu_fsgs.py's bound for two runs)
        assert float((a[k] - b[k]).abs().max()) <= 2e-4 * max(1e-12, float(a[k].abs().max())), k


# ---- 6. edge cases ---------------------------------------------------------------------------------------------------
def test_empty_model(hip):
    cam = synthetic.orbit_cameras(40, 24)[0]
    means = torch.zeros((0, 3), device=DEV, requires_grad=True)
    op = torch.zeros((0, 1), device=DEV, requires_grad=True)
    depth, alpha, radii = depth_pass(_settings(cam, torch.zeros(3)), means, op, torch.zeros((0, 3), device=DEV),
                                     torch.zeros((0, 4), device=DEV), grad="both")
    assert depth.shape == (1, 24, 40) and float(depth.abs().max()) == 0 and float(alpha.abs().max()) == 0 and radii.numel() == 0
    (depth.sum() + alpha.sum()).backward()
    assert means.grad is None or means.grad.numel() == 0


def test_scene_behind_the_camera(hip, cull):
    sc, cam, bg = random_scene("trained_8000")
    sc = {k: v[:3000] for k, v in sc.items()}
    # the camera looks at the origin from `camera_center`: mirror the scene to the far side of the camera
    behind = dict(sc, means3D=sc["means3D"] * 0.2 + 2.0 * cam.camera_center[None])
    dd, da = dpr.cotangents(cam.image_height, cam.image_width, 5)
    h = run_pass(behind, cam, bg, dd, da, "both")
    torch.cuda.synchronize()
    assert int(h["radii"].abs().max()) == 0
    assert float(h["depth"].abs().max()) == 0 and float(h["alpha"].abs().max()) == 0
    for k, g in h["grads"].items():
        assert float(g.abs().max()) == 0, k


@pytest.mark.parametrize("name", ["alpha_diagonal_corner", "len_65", "quad_early_sat", "partial_9x33_stop128"])
def test_precomputed_covariance(hip, oracle, cull, name):
    """cov3D_precomp input (tests/blend_cases.py's `scene`, among them the one footprint scales + identity rotation cannot
    describe), gradient to the opacities, the bounds of test 1"""
    r = dpr.oracle_case(oracle, name, "scene")
    case, (dd, da), dn, dg = r["case"], r["cot"], r["dense"], r["dense_grads"]
    h = run_pass(case.scene, case.cam, case.bg, dd, da, "opacity")
    assert torch.equal(h["radii"], r["oracle"]["radii"])
    for k in ("depth", "alpha"):
        assert float((h[k].double() - dn[k]).abs().max()) / max(1.0, float(dn[k].abs().max())) <= TOL, k
    d = dpr.distance(h["grads"]["opacities"], dg["opacities"], "opacities")
    print(name, "opacities err %.2e d_ref %.2e" % (d, r["d_ref"]["opacities"]))
    assert d <= max(TOL, 3.0 * r["d_ref"]["opacities"])
    g = general_pass(case.scene, case.cam, case.bg, None, None, None)
    assert torch.equal(h["depth"], g["depth"]) and torch.equal(h["alpha"], g["alpha"])


def test_null_alpha_cotangent_is_zero(hip):
    """A missing cotangent is a zero image: the kernel's per-tile sums are the same fp32 numbers either way (kd = z dL_ddepth
    + 0), so the two results differ at most by the order in which the float64 rows received them - below one fp32 rounding
    of an element, 2^-24 = 6e-8 of it; 1e-6 of the tensor's largest entry."""
    sc, cam, bg = random_scene("trained_8000")
    dd, da = dpr.cotangents(cam.image_height, cam.image_width, 6)
    a = run_pass(sc, cam, bg, dd, None, "both")
    b = run_pass(sc, cam, bg, dd, torch.zeros_like(da), "both")
    for k in a["grads"]:
        assert float(a["grads"][k].abs().max()) > 0
        assert float((a["grads"][k] - b["grads"][k]).abs().max()) <= 1e-6 * float(b["grads"][k].abs().max()), k


def test_status_codes(hip):
    """the C ABI's argument rules, straight through the entry points: status codes, no launch"""
    E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -5
    case = blend_cases.build("len_65")
    sc, cam = case.scene_sr, case.cam
    W, H, P = case.W, case.H, sc["means3D"].shape[0]
    keep = []
    means = sc["means3D"].to(DEV)

    def structs(antialiasing=False, **gkw):
        view = hip._view(keep, DEV, case.bg, cam.world_view_transform, cam.full_proj_transform, cam.camera_center, cam.tanfovx,
                         cam.tanfovy, H, W, 1.0, 0, False, antialiasing, False, tile_cull=0)
        g = hip._gauss(keep, DEV, means, None, means, sc["opacities"], sc["scales"], sc["rotations"], None)
        for k, v in gkw.items():
            setattr(g, k, v)
        return view, g
    gb, ib, _, _ = hip.scratch_bytes(P, W, H, 0)
    geom = torch.zeros((gb,), dtype=torch.uint8, device=DEV)
    img = torch.zeros((ib,), dtype=torch.uint8, device=DEV)
    s = hip._scratch(geom, img, None, 0)
    f = lambda n: torch.zeros((n,), device=DEV)   # noqa: E731
    depth, alpha, radii = f(W * H), f(W * H), torch.zeros((P,), dtype=torch.int32, device=DEV)
    dm3, dm2, dop, ws = f(3 * P), f(3 * P), f(P), torch.zeros((P * 128 + 256,), dtype=torch.uint8, device=DEV)
    fwd, bwd = hip.api.raw("depth_forward"), hip.api.raw("depth_backward")
    stream = hip._stream(DEV)

    def forward(view, g, d=depth, a=alpha):
        return fwd(C.byref(view), C.byref(g), C.byref(s), d.data_ptr() if d is not None else None,
                   a.data_ptr() if a is not None else None, stream)

    def backward(view, g, flags, m3=dm3, m2=dm2, op=dop):
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        return bwd(C.byref(view), C.byref(g), radii.data_ptr(), C.byref(s), 0, depth.data_ptr(), alpha.data_ptr(), flags,
                   p(m3), p(m2), p(op), ws.data_ptr(), ws.numel(), stream)
    v, g = structs()
    va, _ = structs(antialiasing=True)
    assert forward(va, g) == E_UNSUPPORTED and backward(va, g, 3) == E_UNSUPPORTED
    assert forward(v, g, d=None) == E_NULL and forward(v, g, a=None) == E_NULL
    assert backward(v, g, 1, m3=None) == E_NULL and backward(v, g, 3, m2=None) == E_NULL and backward(v, g, 2, op=None) == E_NULL
    assert backward(v, g, 2, m3=None, m2=None) == 0 and backward(v, g, 1, op=None) == 0   # only what was asked for is needed
    for flags in (0, 4, -1):
        assert backward(v, g, flags) == E_SHAPE
    x = f(P)
    for gkw in (dict(raw_activations=1), dict(shs_rest=x.data_ptr()), dict(extra_channel=x.data_ptr())):
        _, gx = structs(**gkw)
        assert forward(v, gx) == E_UNSUPPORTED and backward(v, gx, 3) == E_UNSUPPORTED, gkw
    # P == 0: the outputs are zeroed, GS_OK
    depth.fill_(7.0)
    alpha.fill_(7.0)
    _, g0 = structs(P=0)
    assert forward(v, g0) == 0 and backward(v, g0, 3) == 0
    torch.cuda.synchronize()
    assert float(depth.abs().max()) == 0 and float(alpha.abs().max()) == 0


# ---- 7. the drop-in functions -----------------------------------------------------------------------------------------
class _Model:
    """what DNGaussian's render_for_depth / render_for_opa read of a GaussianModel"""
    active_sh_degree = 0

    def __init__(self, sc):
        self.get_xyz = sc["means3D"].detach().clone().to(DEV).requires_grad_(True)
        self.get_opacity = sc["opacities"].detach().clone().to(DEV).requires_grad_(True)
        self.get_scaling = sc["scales"].detach().clone().to(DEV).requires_grad_(True)
        self.get_rotation = sc["rotations"].detach().clone().to(DEV).requires_grad_(True)

        self.cov_cpu = covariance(sc)
        self._cov = self.cov_cpu.to(DEV).requires_grad_(True)

    def get_covariance(self, scaling_modifier=1.0):
        assert scaling_modifier == 1.0
        return self._cov * 1.0    # (attached, as the model's: the pass must detach it)


def covariance(sc):
    import dense_reference
    R = dense_reference.quat_to_rot(sc["rotations"].double())
    S = torch.diag_embed(sc["scales"].double())
    Sig = (R @ S @ S @ R.transpose(1, 2)).float()
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], dim=1).contiguous()


class _Pipe:
    debug = False

    def __init__(self, compute_cov3D_python):
        self.compute_cov3D_python = compute_cov3D_python


@pytest.mark.parametrize("cov_python", [False, True], ids=["scales_rotations", "cov3D_python"])
def test_render_for_depth_and_render_for_opa(hip, cov_python):
    sc, cam, bg = random_scene("trained_8000")
    sc = {k: v[:4000] for k, v in sc.items()}
    vc = synthetic.Camera(cam.image_height, cam.image_width, cam.FoVx, cam.FoVy, cam.world_view_transform.to(DEV),
                          cam.full_proj_transform.to(DEV), cam.camera_center.to(DEV))
    dd, da = dpr.cotangents(cam.image_height, cam.image_width, 7)
    pipe = _Pipe(cov_python)
    ref_sc = sc
    if cov_python:
        ref_sc = dict(means3D=sc["means3D"], opacities=sc["opacities"], cov3D_precomp=covariance(sc))

    def bound(a, b, k):
        assert float((a.cpu() - b).abs().max()) <= 2e-4 * max(1e-12, float(b.abs().max())), k
    # hard depth
    pc = _Model(sc)
    pkg = dgr_dng.render_for_depth(vc, pc, pipe, bg.to(DEV), 1.0, 0.95)
    assert set(pkg) == {"depth", "alpha", "viewspace_points", "visibility_filter", "radii"}   # no "render"
    ((pkg["depth"] * dd.to(DEV)).sum() + (pkg["alpha"] * da.to(DEV)).sum()).backward()
    ref = general_pass(ref_sc, cam, bg, dd, da, "means", opacity=0.95)
    for k in ("depth", "alpha", "radii"):
        assert torch.equal(pkg[k].detach().cpu(), ref[k]), k
    assert torch.equal(pkg["visibility_filter"].cpu(), ref["radii"] > 0)
    bound(pc.get_xyz.grad, ref["grads"]["means3D"], "means3D")
    bound(pkg["viewspace_points"].grad, ref["grads"]["means2D"], "means2D")
    assert pc.get_opacity.grad is None and pc.get_scaling.grad is None and pc.get_rotation.grad is None
    # soft depth
    pc = _Model(sc)
    pkg = dgr_dng.render_for_opa(vc, pc, pipe, bg.to(DEV))
    assert set(pkg) == {"depth", "alpha", "viewspace_points", "visibility_filter", "radii", "opacity"}
    assert pkg["opacity"] is pc.get_opacity
    ((pkg["depth"] * dd.to(DEV)).sum() + (pkg["alpha"] * da.to(DEV)).sum()).backward()
    ref = general_pass(ref_sc, cam, bg, dd, da, "opacity")
    for k in ("depth", "alpha", "radii"):
        assert torch.equal(pkg[k].detach().cpu(), ref[k]), k
    bound(pc.get_opacity.grad, ref["grads"]["opacities"], "opacities")
    assert pc.get_xyz.grad is None and pc.get_scaling.grad is None and pc.get_rotation.grad is None
