"""The depth-only pass (gsplat_amd.depth_pass, csrc/gs_depth_pass.hip) on the host: the yardstick the GPU tests hold it to -
the reference's two depth compositions (tests/depth_pass_reference.py) over the CPU checker against the float64 model - and
the parts of the interface that need no device."""
import os
import re

import pytest
import torch

import blend_cases
import depth_pass_reference as dpr
from gsplat_amd import synthetic
from helpers import TOL
from test_oracle_dense import small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
SR_CASES = [n for n in blend_cases.NAMES if n not in blend_cases.NO_SCALES_ROTATIONS]

# Gradient bar of the checker against float64 on these passes.  With colour 1 the backward's dL_dalpha carries
# (1 - accum_alpha_rec), which cancels on saturated pixels down to the final transmittance, 1e-4 at the stopping rule: an fp32
# rounding of 2^-24 = 6e-8 on either operand becomes 6e-8 / 1e-4 = 6e-4 of the term.  1e-3 leaves a factor 1.7 for the sums around
# it.  (The checker in its exact-transmittance form; with the reference's `1 - alpha` read-back T_final itself cancels the same
# way and the distance reaches 6.5e-2.)  Every other tensor of these tests is held to helpers.TOL.
GRAD_BAR = 1e-3


def _check_outputs(got, dn, what):
    assert torch.equal(got["radii"].long(), dn["radii"].long()), what
    for k in ("depth", "alpha"):
        e = float((got[k].double() - dn[k]).abs().max()) / max(1.0, float(dn[k].abs().max()))
        print(what, k, "%.2e" % e)
        assert e <= TOL, "%s: %s is %.3e from float64 on some pixel" % (what, k, e)   # no pixel is exempt


@pytest.mark.parametrize("name", SR_CASES)
def test_reference_composition_on_constructed_scenes(oracle, name):
    """depth, alpha: every pixel within helpers.TOL of float64 (the margin condition of tests/blend_cases.py is on alpha and
    T alone, so it carries over to colour 1 and to any opacity-independent cotangent).  Gradients: the checker's distance
    d_ref per tensor, recorded for tests/test_gpu_depth_pass.py, below the bar derived above."""
    r = dpr.oracle_case(oracle, name)
    _check_outputs(r["oracle"], r["dense"], name)
    print(name, "d_ref", {k: "%.2e" % v for k, v in r["d_ref"].items()})
    for k, v in r["d_ref"].items():
        assert v <= GRAD_BAR, "%s: dL_d%s of the checker is %.3e from float64" % (name, k, v)


@pytest.mark.parametrize("seed,eye,big,opacity,grad", [(1, (3.2, 1.0, 1.5), False, None, "opacity"),
                                                        (3, (0.6, -1.4, 0.4), True, 0.95, "means"),
                                                        (5, (2.0, 2.0, 2.0), False, None, "both")])
def test_reference_composition_on_small_scenes(oracle, seed, eye, big, opacity, grad):
    """the hard pass (constant opacity, gradient to the means), the soft pass and both families at once on random scenes"""
    sc = small_scene(110, seed, False, False, 3, big)
    W, H = 44, 36
    cam = synthetic.look_at_camera(eye, W, H, FoVx=0.9)
    bg = torch.tensor([0.2, 0.9, 0.1])
    dd, da = dpr.cotangents(H, W, seed)
    with dpr.exact_T(oracle):
        o = dpr.reference_pass(oracle.FsgsRasterizer, oracle.FsgsSettings, sc, cam, bg, CPU, dd, da, grad, opacity=opacity)
    dn, dg = dpr.dense_pass(sc, cam, bg, dd, da, opacity=opacity)
    _check_outputs(o, dn, "small_%d" % seed)
    assert set(o["grads"]) == set(dpr.FAMILY[grad])
    for k in o["grads"]:
        d = dpr.distance(o["grads"][k], dg[k], k)
        print("small_%d" % seed, k, "%.2e" % d)
        assert d <= GRAD_BAR, (k, d)


def test_helper_is_the_reference_composition(oracle):
    """what the helper detaches gets no gradient, what it asks for is all it returns, and a null cotangent is a zero one"""
    sc = small_scene(60, 2, False, False, 3, False)
    cam = synthetic.look_at_camera((3.0, 0.5, 1.0), 40, 32, FoVx=0.9)
    dd, da = dpr.cotangents(32, 40, 0)
    bg = torch.zeros(3)
    run = lambda *a, **k: dpr.reference_pass(oracle.FsgsRasterizer, oracle.FsgsSettings, sc, cam, bg, CPU, *a, **k)  # noqa: E731
    hard, soft = run(dd, da, "means", opacity=0.95), run(dd, da, "opacity")
    assert set(hard["grads"]) == {"means3D", "means2D"} and set(soft["grads"]) == {"opacities"}
    assert run(dd, da, None)["grads"] == {}
    a, b = run(dd, None, "opacity"), run(dd, torch.zeros_like(da), "opacity")
    assert torch.equal(a["grads"]["opacities"], b["grads"]["opacities"]) and torch.equal(a["depth"], soft["depth"])
    assert not torch.equal(hard["alpha"], soft["alpha"])


# ---- the interface rules that need no library call -------------------------------------------------------------------
def _settings(confidence=False):
    import dgr_dng
    import dgr_fsgs
    cam = synthetic.look_at_camera((3.0, 0.0, 0.0), 32, 32)
    kw = dict(image_height=32, image_width=32, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3), scale_modifier=1.0,
              viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center,
              prefiltered=False, debug=False)
    if confidence:
        return dgr_fsgs.GaussianRasterizationSettings(confidence=torch.ones((4, 1)), **kw)
    return dgr_dng.GaussianRasterizationSettings(**kw)


def test_depth_pass_interface_rules():
    from gsplat_amd.depth_pass import depth_pass
    m, op, s, q, cov = torch.zeros((4, 3)), torch.full((4, 1), 0.5), torch.ones((4, 3)), torch.ones((4, 4)), torch.ones((4, 6))
    rs = _settings()
    with pytest.raises(RuntimeError, match="no fallback"):   # CPU tensors raise, as everywhere else
        depth_pass(rs, m, op, s, q)
    with pytest.raises(RuntimeError, match="no fallback"):
        depth_pass(rs, m, 0.95, cov3D_precomp=cov, grad=None)
    for bad in ("mean", "opacities", "all", 3, ""):
        with pytest.raises(ValueError, match="grad must be"):
            depth_pass(rs, m, op, s, q, grad=bad)
    for g in ("opacity", "both"):                            # a constant has no gradient
        with pytest.raises(ValueError, match="constant opacity"):
            depth_pass(rs, m, 0.95, s, q, grad=g)
    msg = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
    for kw in (dict(), dict(scales=s), dict(rotations=q), dict(scales=s, rotations=q, cov3D_precomp=cov),
               dict(scales=s, cov3D_precomp=cov)):
        with pytest.raises(Exception, match=re.escape(msg)):
            depth_pass(rs, m, op, **kw)
    with pytest.raises(ValueError, match="confidence"):      # the FSGS settings tuple: this pass does not rescale gradients
        depth_pass(_settings(confidence=True), m, op, s, q)


def test_drop_in_functions_carry_the_reference_signatures():
    import inspect
    import dgr_dng
    a = inspect.signature(dgr_dng.render_for_depth)
    b = inspect.signature(dgr_dng.render_for_opa)
    assert list(a.parameters) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "value"]
    assert list(b.parameters) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier"]
    assert a.parameters["scaling_modifier"].default == 1.0 and a.parameters["value"].default == 0.95
    assert b.parameters["scaling_modifier"].default == 1.0


# ---- ABI, prototype table, build ---------------------------------------------------------------------------------------
def test_abi_declares_the_pair_and_stays_at_7():
    from gsplat_amd import capi
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert re.search(r"#define GS_ABI_VERSION 7\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    fwd = re.search(r"int gs_depth_forward\(([^)]*)\)", code).group(1)
    bwd = re.search(r"int gs_depth_backward\(([^)]*)\)", code).group(1)
    assert len(fwd.split(",")) == 6 == len(capi.PROTOTYPES["depth_forward"][1])
    assert len(bwd.split(",")) == 14 == len(capi.PROTOTYPES["depth_backward"][1])
    assert "int grad_flags" in bwd and "workspace_bytes" in bwd
    for n in ("depth_forward", "depth_backward"):
        assert n in capi.DEVICE_ONLY, n      # HIP-only: the checker is not touched
    mk = open(os.path.join(ROOT, "sparse-view-3dgs-pack_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS = (.*)$", mk, flags=re.M).group(1).split()
    assert "gs_depth_pass.o" in objs
    rule = re.search(r"^gs_depth_pass\.o:.*\n\t(.*)$", mk, flags=re.M).group(1)
    assert "$(STRICT)" in rule                # built without fp contraction
    assert os.path.exists(os.path.join(ROOT, "sparse-view-3dgs-pack_amd", "csrc", "gs_depth_pass.hip"))
