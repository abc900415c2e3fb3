"""DNGaussian's two depth passes restated over any rasterizer class of the FSGS generation, and their float64 model.

`reference_pass` is the composition of DNGaussian/gaussian_renderer/__init__.py:128-269 (`render_for_depth`,
`render_for_opa`): colours = ones, scales / rotations / covariance detached, the means detached in the soft pass, the
opacity a constant in the hard one - through `Rast(settings)(...)`, so that the parent's general path (dgr_dng), the CPU
checker (oracle.FsgsRasterizer) and nothing of the depth-only kernels is involved.  Unlike the reference it takes arbitrary
cotangents of the depth and alpha images and returns the gradients of the family asked for.

`dense_pass` is the same pass in tests/dense_reference.py's float64 autograd model (colors_precomp = 1), and `oracle_case`
holds the checker's own distance to it per gradient tensor - the yardstick d_ref of tests/test_gpu_depth_pass.py."""
import contextlib

import torch

import dense_reference

FAMILY = {"means": ("means3D", "means2D"), "opacity": ("opacities",), "both": ("means3D", "means2D", "opacities"), None: ()}


def _settings(Settings, cam, bg, device, P, scale_modifier=1.0):
    kw = dict(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
              bg=bg.to(device), scale_modifier=scale_modifier, viewmatrix=cam.world_view_transform.to(device),
              projmatrix=cam.full_proj_transform.to(device), sh_degree=0, campos=cam.camera_center.to(device),
              prefiltered=False, debug=False)
    if "confidence" in Settings._fields:
        kw["confidence"] = torch.ones((P, 1), device=device)
    return Settings(**kw)


def reference_pass(Rast, Settings, sc, cam, bg, device, dL_ddepth, dL_dalpha, grad, opacity=None):
    """-> dict(depth, alpha, radii, grads{means3D, means2D, opacities as `grad` names them}), all on the CPU.
    opacity: None = the scene's own [P,1] opacities (the soft pass), a float = that constant everywhere (the hard pass)."""
    P = sc["means3D"].shape[0]
    want = FAMILY[grad]
    means = sc["means3D"].detach().clone().to(device).requires_grad_("means3D" in want)
    if opacity is None:
        op = sc["opacities"].detach().clone().to(device).requires_grad_("opacities" in want)
    else:
        assert "opacities" not in want
        op = torch.ones((P, 1), device=device) * opacity
    m2 = torch.zeros_like(means, requires_grad=True)
    shape = {k: (sc[k].detach().to(device) if sc.get(k) is not None else None) for k in ("scales", "rotations", "cov3D_precomp")}
    colors = torch.ones((P, 3), device=device)
    color, radii, depth, alpha = Rast(_settings(Settings, cam, bg, device, P, sc.get("scale_modifier", 1.0)))(
        means3D=means, means2D=m2, opacities=op, shs=None, colors_precomp=colors, **shape)
    out = dict(depth=depth.detach().cpu(), alpha=alpha.detach().cpu(), radii=radii.detach().cpu(), grads={})
    terms = [(img * d.to(device)).sum() for img, d in ((depth, dL_ddepth), (alpha, dL_dalpha)) if d is not None]
    if want and terms and (means.requires_grad or op.requires_grad):
        sum(terms).backward()
        leaves = dict(means3D=means, means2D=m2, opacities=op)
        for k in want:
            g = leaves[k].grad
            out["grads"][k] = (g if g is not None else torch.zeros_like(leaves[k])).detach().cpu()
    return out


def dense_pass(sc, cam, bg, dL_ddepth, dL_dalpha, opacity=None):
    """The pass in float64 (tests/dense_reference.py, colors_precomp = 1) -> (outputs, grads{means3D, means2D [P,2],
    opacities}); the gradients of both families at once (neither depends on which leaves the other has)."""
    P = sc["means3D"].shape[0]
    f64 = torch.float64
    d = dict(sh_degree=0, scale_modifier=sc.get("scale_modifier", 1.0), colors_precomp=torch.ones((P, 3), dtype=f64))
    d["means3D"] = sc["means3D"].double().clone().requires_grad_(True)
    op = sc["opacities"].double().clone() if opacity is None else torch.full((P, 1), float(torch.tensor(opacity, dtype=torch.float32)), dtype=f64)
    d["opacities"] = op.requires_grad_(True)
    for k in ("scales", "rotations", "cov3D_precomp"):
        if sc.get(k) is not None:
            d[k] = sc[k].double()
    d["ndc_probe"] = torch.zeros((P, 2), dtype=f64, requires_grad=True)
    out = dense_reference.render(d, cam, bg, False)
    terms = [(out[k] * t.double()).sum() for k, t in (("depth", dL_ddepth), ("alpha", dL_dalpha)) if t is not None]
    grads = {}
    if terms:
        sum(terms).backward()
        for k, leaf in (("means3D", "means3D"), ("means2D", "ndc_probe"), ("opacities", "opacities")):
            g = d[leaf].grad
            grads[k] = g if g is not None else torch.zeros_like(d[leaf])
    return {k: out[k].detach() for k in ("depth", "alpha", "radii")}, grads


def distance(a, ref, key):
    """max |a - ref| over max |ref| (floor 1e-12); means2D: the two image-plane columns (the third of the carrier is 0)."""
    a = a.double().cpu()
    if key == "means2D":
        a = a[:, :2]
    return float((a - ref).abs().max()) / max(1e-12, float(ref.abs().max()))


def cotangents(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((1, H, W), generator=g) * 0.3, torch.randn((1, H, W), generator=g)


@contextlib.contextmanager
def exact_T(oracle):
    """The checker keeps the transmittance product as T_final (what the HIP kernels keep) instead of the reference's
    `1 - alpha` read-back, whose fp32 cancellation on saturated pixels puts up to 6.5e-2 on these passes' gradients (colour 1
    makes the backward's `1 - accum_alpha_rec` a second cancellation); as tests/test_gpu_fsgs.py's fixture, off again after."""
    oracle.lib.gso_set_fsgs_exact_T(1)
    try:
        yield
    finally:
        oracle.lib.gso_set_fsgs_exact_T(0)


_ORACLE = {}


def oracle_case(oracle, name, which="scene_sr", modifier=None):
    """One constructed scene (tests/blend_cases.py; its scales + rotations form, or `scene`: its covariances; its own opacities) through the checker's
    FSGS generation in the exact-transmittance form and through the float64 model, both gradient families at once.
    modifier: the scene under that scale modifier (None: as built).
    -> dict(dense outputs, dense grads, oracle result, d_ref{tensor: the checker's distance to float64}); cached."""
    key = (name, which) if modifier is None else (name, which, float(modifier))
    if key not in _ORACLE:
        import blend_cases
        case = blend_cases.build(name)
        sc = getattr(case, which)
        if modifier is not None:
            sc = dict(sc, scale_modifier=float(modifier))
        dd, da = cotangents(case.H, case.W, 4000 + blend_cases.NAMES.index(name))
        dn, dg = dense_pass(sc, case.cam, case.bg, dd, da)
        with exact_T(oracle):
            o = reference_pass(oracle.FsgsRasterizer, oracle.FsgsSettings, sc, case.cam, case.bg, torch.device("cpu"), dd, da, "both")
        d_ref = {k: distance(o["grads"][k], dg[k], k) for k in FAMILY["both"]}
        _ORACLE[key] = dict(case=case, scene=sc, cot=(dd, da), dense=dn, dense_grads=dg, oracle=o, d_ref=d_ref)
    return _ORACLE[key]
