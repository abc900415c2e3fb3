"""The input forms the per-Gaussian kernels accept (preprocess_fwd_kernel, chain_kernel, preprocess_bwd_kernel<SPLIT>, the
depth pass's point backward), one small scene each: SH rows of any count M, packed or split, at every active degree;
a scale modifier on own scales and rotations; precomputed colours and / or covariances.  Shared by
tests/test_form_cases_cpu.py (the CPU checker against the float64 model in every form) and tests/test_gpu_input_forms.py (HIP
against the CPU checker).

The scene of every form is dc_cases.scene_rows under dc_cases.inside_camera: the camera sits inside the cloud, so every
wave holds culled and visible Gaussians; every SH row, inactive ones included, is non-zero."""
import torch

import dc_cases

SIZES = ((64, 48), (37, 53))     # whole tiles / partial tiles on both edges
BG = torch.tensor([0.1, 0.2, 0.3])
P_FULL = 257                     # one full 256-lane workgroup + one real lane beside 255 shadowing lanes
# The depth pass under a modifier: two constructed scenes of tests/blend_cases.py (scales + rotations form) whose footprints
# are narrow enough for the modifier to move every pixel (narrow blobs; a 70-run of mixed widths) and which keep the margin
# condition under both modifiers (tests/test_form_cases_cpu.py asserts it).  The wide-footprint cases are left out: a
# footprint many times the tile barely notices the modifier (final_T moves by 1e-6).
DEPTH_CASES = ("quad_four_batches", "ties_70")
DEPTH_MODIFIERS = (0.6, 1.8)


def _form(fid, n, **kw):
    f = dict(id=fid, P=P_FULL, M=16, D=3, split=False, mod=1.0, aa=False, depth=False, colors=False, cov=False, twin=None)
    f.update(kw)
    f["W"], f["H"] = SIZES[n % 2]
    f["seed"] = 40 + n
    return f


def _table():
    t = []
    n = 0
    # unsplit rows: every M at every active degree that fits
    for M in (1, 4, 9, 16, 25):
        for D in range(4):
            if (D + 1) ** 2 <= min(M, 16):
                t.append(_form("M%d_D%d" % (M, D), n, M=M, D=D, aa=bool(n & 1), depth=bool(n & 2)))
                n += 1
    # the three generic row counts at their highest degree, at the workgroup's edges
    for M, D in ((1, 0), (4, 1), (9, 2)):
        for P in (1, 255, 256):
            t.append(_form("M%d_D%d_P%d" % (M, D, P), n, M=M, D=D, P=P, aa=bool(n & 1), depth=bool(n & 2)))
            if P == 1:   # a seed whose one Gaussian is on screen and opaque enough to blend (opacity 0.47 ... 0.72)
                t[-1]["seed"] = 67 + M // 4
            n += 1
    # split rows (dc= / shs=)
    for M, top in ((4, 1), (9, 2), (16, 3)):
        for D in (0, top):
            t.append(_form("split_M%d_D%d" % (M, D), n, M=M, D=D, split=True, aa=bool(n & 1), depth=bool(n & 2)))
            n += 1
    # a scale modifier on own scales and rotations
    for mod in (0.6, 1.8):
        for aa in (False, True):
            for depth in (False, True):
                t.append(_form("mod%.1f_aa%d_depth%d" % (mod, aa, depth), n, mod=mod, aa=aa, depth=depth))
                n += 1
    # precomputed colours with own scales and rotations (the modifier-1 form is the same input form)
    for mod in (0.6, 1.8):
        t.append(_form("colors_mod%.1f" % mod, n, colors=True, mod=mod, aa=mod > 1, depth=True))
        n += 1
    # SH colour with a precomputed covariance
    for M, D in ((16, 3), (9, 2)):
        t.append(_form("cov_M%d_D%d" % (M, D), n, M=M, D=D, cov=True, aa=M == 9, depth=True))
        n += 1
    # both precomputed: the modifier must change nothing (`twin`: the same form at modifier 1, compared bit for bit)
    for mod in (0.6, 1.8):
        f = _form("colors_cov_mod%.1f" % mod, n, colors=True, cov=True, mod=mod, aa=mod > 1, depth=True)
        f["twin"] = dict(f, id=f["id"] + "_twin", mod=1.0)
        t.append(f)
        n += 1
    return t


FORMS = _table()
# the FSGS rasterizer generation (dgr_fsgs: no anti-aliasing, depth and alpha images instead of the inverse depth)
FSGS_FORMS = [_form("fsgs_M4_D1_mod1.8", 60, M=4, D=1, mod=1.8), _form("fsgs_M9_D2", 61, M=9, D=2),
              _form("fsgs_colors_mod0.6", 62, colors=True, mod=0.6)]
UNSPLIT = [f for f in FORMS if not f["split"]]
SPLIT = [f for f in FORMS if f["split"]]
BY_ID = {f["id"]: f for f in FORMS}
assert len(BY_ID) == len(FORMS)
_BUILT = {}


def build(form):
    """-> (scene dict as helpers.run_scene / forward_state take it, camera).  A split form's scene holds the concatenated
    rows: the callers split them."""
    key = form["id"]
    if key not in _BUILT:
        M, P = form["M"], form["P"]
        K = min(M, 16) - 1
        sc = dc_cases.scene_rows(P, K, seed=form["seed"], max_degree=form["D"])
        g = torch.Generator().manual_seed(1000 + form["seed"])
        if M > 16:   # rows no degree reaches
            sc["shs"] = torch.cat([sc["shs"], 0.15 * torch.randn((P, M - 16, 3), generator=g)], dim=1).contiguous()
        assert tuple(sc["shs"].shape) == (P, M, 3) and bool((sc["shs"] != 0).all())
        scene = dict(means3D=sc["means3D"], opacities=sc["opacities"], sh_degree=form["D"], scale_modifier=form["mod"])
        if form["colors"]:
            scene["colors_precomp"] = torch.rand((P, 3), generator=g)
        else:
            scene["shs"] = sc["shs"]
        if form["cov"]:
            scene["cov3D_precomp"] = dc_cases.covariances(sc)
        else:
            scene["scales"], scene["rotations"] = sc["scales"], sc["rotations"]
        _BUILT[key] = (scene, dc_cases.inside_camera(form["W"], form["H"]))
    return _BUILT[key]


def cotangents(form):
    """-> (dL_dcolor [3,H,W], dL_dinvdepth [1,H,W] or None)"""
    g = torch.Generator().manual_seed(2000 + form["seed"])
    dc = torch.randn((3, form["H"], form["W"]), generator=g)
    di = torch.randn((1, form["H"], form["W"]), generator=g) * 0.3
    return dc, (di if form["depth"] else None)


def analytic(grads, scene):
    """The gradients as the float64 model has them: the rasterizer returns dL_dscales w.r.t. modifier x scale without the
    factor `modifier` (the reference's backward.cu:372-375, csrc/gs_backward_math.h: cov3d_backward), so that tensor is
    multiplied by the modifier.  Used only where the arbiter is the float64 model."""
    out = dict(grads)
    if out.get("scales") is not None:
        out["scales"] = out["scales"] * scene.get("scale_modifier", 1.0)
    return out


def skipped_state(form):
    """per-Gaussian state a precomputed input never materialises (test_gpu_raster_parity.compare_forward's `skip`)"""
    return (("rgb", "clamped") if form["colors"] else ()) + (("cov3D",) if form["cov"] else ())


def run_split(Rasterizer, Settings, scene, cam, device, bg, antialiasing, dL_dcolor, dL_dinvdepth):
    """helpers.run_scene for the split call rasterizer(dc=shs[:, :1], shs=shs[:, 1:], ...) of gsplat_amd.accel: the same
    result dict, the SH gradient as grads["dc"], grads["rest"] and, concatenated, grads["shs"]."""
    from helpers import settings_for
    p = {k: scene[k].detach().clone().to(device).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    dc = scene["shs"][:, :1, :].detach().clone().contiguous().to(device).requires_grad_(True)
    rest = scene["shs"][:, 1:, :].detach().clone().contiguous().to(device).requires_grad_(True)
    means2D = torch.zeros_like(p["means3D"], requires_grad=True)
    rs = settings_for(Settings, cam, bg, scene["sh_degree"], device, antialiasing, scene.get("scale_modifier", 1.0))
    color, radii, invdepth = Rasterizer(raster_settings=rs)(
        means3D=p["means3D"], means2D=means2D, opacities=p["opacities"], dc=dc, shs=rest, colors_precomp=None,
        scales=p["scales"], rotations=p["rotations"], cov3D_precomp=None)
    loss = (color * dL_dcolor.to(device)).sum()
    if dL_dinvdepth is not None:
        loss = loss + (invdepth * dL_dinvdepth.to(device)).sum()
    loss.backward()
    grads = {k: v.grad.detach() for k, v in p.items()}
    grads.update(dc=dc.grad.detach(), rest=rest.grad.detach(), means2D=means2D.grad.detach())
    grads["shs"] = torch.cat((grads["dc"], grads["rest"]), dim=1)
    return dict(color=color.detach(), radii=radii.detach(), invdepth=invdepth.detach(), grads=grads)


def as_pair(out):
    """a helpers.run_scene / run_split result in the shape dc_cases.assert_same compares (host tensors, dc / rest rows)"""
    g = {k: v.cpu() for k, v in out["grads"].items()}
    if "dc" not in g:
        g["dc"], g["rest"] = g["shs"][:, :1, :], g["shs"][:, 1:, :]
    g.setdefault("cov3D_precomp", None)
    return dict(color=out["color"].cpu(), radii=out["radii"].cpu(), invdepth=out["invdepth"].cpu(), grads=g)
