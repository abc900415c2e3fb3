"""SparseGaussianAdam and the `dc=` rasterizer call, as far as they can be checked without a GPU: the two update rules'
restatement (tests/sparse_adam_reference.py) against a closed form and a plain-Python recurrence, the optimizer class's state
layout under the reference's optimizer surgery, the opt-in packages' import surface, and the `dc=` call's fall-back path on
the CPU checker."""
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch import nn

import dc_cases
import sparse_adam_reference as ref
import step_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-view-3dgs-pack_amd")
ACCEL = os.path.join(PKG, "accel")
B1, B2, EPS = step_reference.BETA1, step_reference.BETA2, step_reference.EPS


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_no_bias_first_step_is_the_closed_form():
    """From zero moments the first step moves a stepped element by lr (1-b1) g / (sqrt((1-b2) g^2) + eps) =
    lr * 0.1 / sqrt(0.001) * sign(g) = 3.1623 lr sign(g) for |g| >= 1e-3 at eps = 1e-15 (the "3.16 x lr" of ADVICE.md)."""
    rng = np.random.default_rng(0)
    n, lr = 300, 0.0025
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 2, n)).astype(np.float32)
    p = rng.normal(size=n).astype(np.float32)
    z = np.zeros(n, np.float32)
    p1, m1, v1 = ref.no_bias_ref(p, g, z, z, lr, np.ones(n, bool), np.float64)
    gd = g.astype(np.float64)
    closed = lr * (1 - B1) * gd / (np.sqrt((1 - B2) * gd * gd) + EPS)
    move = p.astype(np.float64) - p1
    assert np.all(np.abs(move - closed) <= 1e-12 * np.abs(closed))
    factor = (1 - B1) / math.sqrt(1 - B2)
    assert abs(factor - 3.1623) < 1e-4
    assert np.all(np.abs(move / (lr * np.sign(gd)) - factor) <= 1e-6 * factor)
    assert np.array_equal(m1, (1 - B1) * gd) and np.allclose(v1, (1 - B2) * gd * gd, rtol=1e-15)


def test_no_bias_six_steps_equal_the_recurrence_in_python_floats():
    rng = np.random.default_rng(1)
    n, lr = 17, 0.005
    p0 = rng.normal(size=n).astype(np.float32)
    gs = rng.normal(size=(6, n)).astype(np.float32)
    # the restatement takes float32 state (the model's numbers) and returns float64: carry the float64 state by hand
    want = []
    for i in range(n):
        p, m, v = float(p0[i]), 0.0, 0.0
        for s in range(6):
            g = float(gs[s, i])
            m = B1 * m + (1.0 - B1) * g
            v = B2 * v + ((1.0 - B2) * g) * g
            p = p - lr * (m / (math.sqrt(v) + EPS))
        want.append(p)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for s in range(6):
        g = gs[s].astype(np.float64)
        m = B1 * m + (1.0 - B1) * g
        v = B2 * v + ((1.0 - B2) * g) * g
        p = p - lr * (m / (np.sqrt(v) + EPS))
    assert np.array_equal(p, np.array(want))
    # ... and one restated step from rounded state is that recurrence's step
    m32, v32, p32 = m.astype(np.float32), v.astype(np.float32), p.astype(np.float32)
    g = rng.normal(size=n).astype(np.float32)
    got_p, got_m, got_v = ref.no_bias_ref(p32, g, m32, v32, lr, np.ones(n, bool), np.float64)
    for i in range(n):
        mi = B1 * float(m32[i]) + (1.0 - B1) * float(g[i])
        vi = B2 * float(v32[i]) + ((1.0 - B2) * float(g[i])) * float(g[i])
        assert got_m[i] == mi and got_v[i] == vi
        assert got_p[i] == float(p32[i]) - lr * (mi / (math.sqrt(vi) + EPS))


@pytest.mark.parametrize("bias_correction", [False, True])
def test_masked_rows_keep_their_bits_nan_included(bias_correction):
    rng = np.random.default_rng(2)
    P, w = 9, 5
    mask = np.array([1, 0, 0, 1, 0, 1, 1, 0, 1], bool)
    p, g, m = (rng.normal(size=P * w).astype(np.float32) for _ in range(3))
    v = np.abs(rng.normal(size=P * w)).astype(np.float32)
    off = ~np.repeat(mask, w)
    nan = np.array([0x7fc01234], np.uint32).view(np.float32)[0]   # (a payload: the bits must survive, not just NaN-ness)
    for x in (g, m, v):
        x[off] = nan
    for dtype in (np.float32, np.float64):
        p1, m1, v1 = ref.sparse_adam_ref(p, g, m, v, 0.01, 3, w, mask, bias_correction, dtype)
        for got, was in ((p1, p), (m1, m), (v1, v)):
            assert np.array_equal(got[off].astype(np.float32).view(np.uint32), was[off].view(np.uint32))
            assert np.all(np.isfinite(got[~off])) and not np.array_equal(got[~off].astype(np.float32), was[~off])


def test_bias_corrected_rule_is_step_reference_adam_ref():
    rng = np.random.default_rng(3)
    n = 40
    p, g, m = (rng.normal(size=n).astype(np.float32) for _ in range(3))
    v = np.abs(rng.normal(size=n)).astype(np.float32)
    mask = rng.random(n // 4) < 0.5
    for dtype in (np.float32, np.float64):
        a = ref.sparse_adam_ref(p, g, m, v, 0.02, 5, 4, mask, True, dtype)
        b = step_reference.adam_ref(p, g, m, v, np.full(n, 0.02), np.full(n, 5), np.repeat(mask, 4), dtype)
        for x, y in zip(a, b):
            assert x.dtype == dtype and np.array_equal(x, y)


def test_float32_form_lies_within_param_tolerance_of_the_float64_form():
    rng = np.random.default_rng(4)
    for w, lr, t in zip(ref.WIDTHS, ref.LRS, (1, 2, 3, 5, 8, 13)):
        n = 257 * w
        p, m = (rng.normal(size=n).astype(np.float32) for _ in range(2))
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-4, 1, n)).astype(np.float32)
        v = (rng.normal(size=n) ** 2 * 1e-3).astype(np.float32)
        for bc in (False, True):
            p32, m32, v32 = ref.sparse_adam_ref(p, g, m, v, lr, t, w, None, bc, np.float32)
            p64, m64, v64 = ref.sparse_adam_ref(p, g, m, v, lr, t, w, None, bc, np.float64)
            tol, own = step_reference.param_tolerance(p32, p64)
            assert own <= tol and np.abs(p32 - p64).max() <= tol
            # (the moments are not compared across the two forms: the float32 form holds 1 - b2 = 0.001 to 3e-5 only, as the
            #  kernels do; they are held to the float32 form bit for bit on the GPU)
            assert m32.dtype == v32.dtype == np.float32 and m64.dtype == v64.dtype == np.float64
            assert not np.array_equal(p32, p)


# ---------------------------------------------------------------------------------------------- the class, on CPU leaves
def _model(P=12):
    g = torch.Generator().manual_seed(5)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    return [{"params": [nn.Parameter(torch.randn(s, generator=g))], "lr": lr, "name": n}
            for (n, s), lr in zip(shapes.items(), ref.LRS)]


def _fill_state(opt, value=0.5):
    """What a first step leaves (created here by hand: no GPU)."""
    for group in opt.param_groups:
        p = group["params"][0]
        opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.full_like(p, value), "exp_avg_sq": torch.full_like(p, value)}


# the reference's optimizer surgery, restated (LGDWT-GS/scene/gaussian_model.py:316-386)
def replace_tensor_to_optimizer(opt, tensor, name):
    out = {}
    for group in opt.param_groups:
        if group["name"] == name:
            stored = opt.state.get(group["params"][0], None)
            stored["exp_avg"] = torch.zeros_like(tensor)
            stored["exp_avg_sq"] = torch.zeros_like(tensor)
            del opt.state[group["params"][0]]
            group["params"][0] = nn.Parameter(tensor.requires_grad_(True))
            opt.state[group["params"][0]] = stored
            out[group["name"]] = group["params"][0]
    return out


def prune_optimizer(opt, mask):
    out = {}
    for group in opt.param_groups:
        stored = opt.state.get(group["params"][0], None)
        if stored is not None:
            stored["exp_avg"] = stored["exp_avg"][mask]
            stored["exp_avg_sq"] = stored["exp_avg_sq"][mask]
            del opt.state[group["params"][0]]
            group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
            opt.state[group["params"][0]] = stored
        else:
            group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
        out[group["name"]] = group["params"][0]
    return out


def cat_tensors_to_optimizer(opt, tensors):
    out = {}
    for group in opt.param_groups:
        assert len(group["params"]) == 1
        ext = tensors[group["name"]]
        stored = opt.state.get(group["params"][0], None)
        if stored is not None:
            stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(ext)), dim=0)
            stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del opt.state[group["params"][0]]
            group["params"][0] = nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))
            opt.state[group["params"][0]] = stored
        else:
            group["params"][0] = nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))
        out[group["name"]] = group["params"][0]
    return out


def test_class_builds_without_the_library_and_survives_the_optimizer_surgery():
    from gsplat_amd.optim import SparseGaussianAdam
    assert issubclass(SparseGaussianAdam, torch.optim.Adam)
    code = ("import sys; from gsplat_amd.optim import SparseGaussianAdam; import torch;"
            "o = SparseGaussianAdam([{'params': [torch.nn.Parameter(torch.zeros(4, 3))], 'lr': 0.1, 'name': 'xyz'}], lr=0.0, eps=1e-15);"
            "assert 'gsplat_amd._lib' not in sys.modules, 'the constructor loaded the library'; print(o.defaults['eps'])")
    env = dict(os.environ, PYTHONPATH=PKG)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "1e-15"

    P = 12
    opt = SparseGaussianAdam(_model(P), lr=0.0, eps=1e-15)     # the reference's call (gaussian_model.py:194-196)
    assert opt.bias_correction is False and opt.defaults["betas"] == (0.9, 0.999)
    assert [g["name"] for g in opt.param_groups] == list(ref.NAMES) and [g["lr"] for g in opt.param_groups] == list(ref.LRS)
    _fill_state(opt)
    # densify: 5 rows appended with zero moments
    gen = torch.Generator().manual_seed(6)
    ext = {g["name"]: torch.randn((5,) + tuple(g["params"][0].shape[1:]), generator=gen) for g in opt.param_groups}
    new = cat_tensors_to_optimizer(opt, ext)
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state[p]
        assert p is new[group["name"]] and p.shape[0] == P + 5 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["exp_avg"].shape == p.shape and float(st["exp_avg"][:P].min()) == 0.5 and float(st["exp_avg"][P:].abs().max()) == 0.0
    # prune: every third row goes
    keep = torch.arange(P + 5) % 3 != 0
    prune_optimizer(opt, keep)
    for group in opt.param_groups:
        p = group["params"][0]
        assert p.shape[0] == int(keep.sum()) and opt.state[p]["exp_avg_sq"].shape == p.shape
    # reset_opacity: the tensor replaced, its moments zeroed
    old = opt.param_groups[3]["params"][0]
    got = replace_tensor_to_optimizer(opt, torch.full_like(old.detach(), -4.0), "opacity")
    p = opt.param_groups[3]["params"][0]
    assert got["opacity"] is p and old not in opt.state and float(opt.state[p]["exp_avg"].abs().max()) == 0.0
    assert len(opt.state) == 6
    # state_dict round trip
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and len(sd["param_groups"]) == 6
    other = SparseGaussianAdam([{"params": [nn.Parameter(torch.zeros_like(g["params"][0]))], "lr": 0.0, "name": g["name"]}
                                for g in opt.param_groups], lr=0.0, eps=1e-15)
    other.load_state_dict(sd)
    for ga, gb in zip(opt.param_groups, other.param_groups):
        assert ga["lr"] == gb["lr"] and ga["name"] == gb["name"] and gb["eps"] == 1e-15
        sa, sb = opt.state[ga["params"][0]], other.state[gb["params"][0]]
        assert float(sb["step"]) == float(sa["step"]) == 1.0
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


def test_class_refuses_what_it_cannot_step():
    from gsplat_amd.optim import SparseGaussianAdam
    P = 12
    opt = SparseGaussianAdam(_model(P), lr=0.0, eps=1e-15)
    for group in opt.param_groups:
        group["params"][0].grad = torch.ones_like(group["params"][0])
    vis = torch.ones(P, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no fallback"):
        opt.step(vis, P)                      # CPU tensors
    with pytest.raises(RuntimeError, match="no fallback"):
        opt.step()
    assert len(opt.state) == 0                # (a refused step leaves no state behind)
    with pytest.raises(ValueError, match="rows"):
        opt.step(torch.ones(7, dtype=torch.bool), 7)      # 12 * 3 elements do not divide into 7 rows
    with pytest.raises(ValueError, match="entries"):
        opt.step(torch.ones(5, dtype=torch.bool), P)
    with pytest.raises(ValueError):
        opt.step(vis)
    two = SparseGaussianAdam([{"params": [nn.Parameter(torch.zeros(4, 3)), nn.Parameter(torch.zeros(4, 1))], "lr": 0.1, "name": "two"}],
                             lr=0.0, eps=1e-15)
    with pytest.raises(ValueError, match="'two'.*ONE tensor per group"):
        two.step()


# ---------------------------------------------------------------------------------------------- the import surface
def _python(code, path):
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.pathsep.join(path)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_opt_in_path_entry_serves_the_probes_of_train_py():
    code = """
import inspect
try:                                                    # LGDWT-GS/train.py:42-46
    from diff_gaussian_rasterization import SparseGaussianAdam
    SPARSE_ADAM_AVAILABLE = True
except:
    SPARSE_ADAM_AVAILABLE = False
assert SPARSE_ADAM_AVAILABLE
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer   # gaussian_renderer/__init__.py
import diff_gaussian_rasterization as d, dgr_3dgs, gsplat_amd.accel as accel, gsplat_amd.optim as optim
import diff_gaussian_rasterization._C
assert d.SparseGaussianAdam is optim.SparseGaussianAdam is dgr_3dgs.SparseGaussianAdam
assert d.GaussianRasterizer is accel.GaussianRasterizer is dgr_3dgs.GaussianRasterizer
assert d._RasterizeGaussians is accel._RasterizeGaussians and d.rasterize_gaussians is accel.rasterize_gaussians
assert list(inspect.signature(GaussianRasterizer.forward).parameters) == ['self', 'means3D', 'means2D', 'opacities', 'shs',
    'colors_precomp', 'scales', 'rotations', 'cov3D_precomp', 'dc']
assert GaussianRasterizationSettings._fields == ('image_height', 'image_width', 'tanfovx', 'tanfovy', 'bg', 'scale_modifier',
    'viewmatrix', 'projmatrix', 'sh_degree', 'campos', 'prefiltered', 'debug', 'antialiasing')
for name in ('GaussianRasterizationSettings', 'GaussianRasterizer', '_RasterizeGaussians', 'rasterize_gaussians', '_C'):
    assert hasattr(d, name) and hasattr(dgr_3dgs, name), name
for name in ('backend', 'rasterize_gaussians', 'rasterize_gaussians_backward', 'mark_visible'):
    assert hasattr(d._C, name), name
import sys
assert 'gsplat_amd._lib' not in sys.modules     # nothing is loaded by the imports
print('ok')
"""
    out = _python(code, [ACCEL, PKG])
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_default_path_still_has_no_sparse_gaussian_adam():
    code = """
try:
    from diff_gaussian_rasterization import SparseGaussianAdam
    print('imported')
except ImportError:
    print('ImportError')
import inspect, diff_gaussian_rasterization as d
assert 'dc' not in inspect.signature(d.GaussianRasterizer.forward).parameters
"""
    out = _python(code, [PKG])
    assert out.returncode == 0 and out.stdout.strip() == "ImportError", out.stderr


# ---------------------------------------------------------------------------------------------- dc= on the CPU checker
@pytest.fixture(scope="module")
def oracle_dc_rasterizer(oracle):
    """gsplat_amd.accel's classes bound to the CPU checker, as tests/oracle_lib.py binds the default package's."""
    from gsplat_amd import accel

    class _Impl:
        backend = oracle.backend
        rasterize_gaussians = staticmethod(oracle.backend.rasterize_gaussians)
        rasterize_gaussians_backward = staticmethod(oracle.backend.rasterize_gaussians_backward)
        mark_visible = staticmethod(oracle.backend.mark_visible)

    class _Fn(accel._RasterizeGaussians):
        _impl = _Impl

    class Rasterizer(accel.GaussianRasterizer):
        _fn = _Fn

    assert _Fn.split_backend() is None      # the checker has no gs_backward_split: the call must take the fall-back
    return Rasterizer


@pytest.mark.parametrize("max_degree", [0, 3])
def test_dc_call_falls_back_and_matches_the_concatenated_call(oracle, oracle_dc_rasterizer, max_degree):
    K = (max_degree + 1) ** 2 - 1
    sc = dc_cases.scene_rows(40, K, seed=7, max_degree=max_degree)
    cam = dc_cases.inside_camera(48, 32)
    cpu = torch.device("cpu")
    for degree in range(max_degree + 1):
        cat = dc_cases.run(oracle.Rasterizer, oracle.Settings, sc, cam, cpu, degree, split=False, use_depth=True)
        split = dc_cases.run(oracle_dc_rasterizer, oracle.Settings, sc, cam, cpu, degree, split=True, use_depth=True)
        assert int((cat["radii"] > 0).sum()) > 0 and float(cat["grads"]["dc"].abs().max()) > 0
        dc_cases.assert_same(split, cat, "degree %d of %d" % (degree, max_degree))
    # positional callers of the default API see no change; markVisible works as on the base class
    rs = dc_cases.settings_for(oracle.Settings, cam, torch.zeros(3), max_degree, cpu)
    rast = oracle_dc_rasterizer(rs)
    m2 = torch.zeros_like(sc["means3D"])
    a = rast(sc["means3D"], m2, sc["opacities"], sc["shs"], None, sc["scales"], sc["rotations"], None)
    b = oracle.Rasterizer(rs)(sc["means3D"], m2, sc["opacities"], sc["shs"], None, sc["scales"], sc["rotations"], None)
    assert all(dc_cases.same_bits(x, y) for x, y in zip(a, b))
    assert torch.equal(rast.markVisible(sc["means3D"]), oracle.Rasterizer(rs).markVisible(sc["means3D"]))


def test_dc_argument_rules_raise_the_reference_texts():
    from gsplat_amd import accel
    rs = accel.GaussianRasterizationSettings(*([None] * 13))
    rast = accel.GaussianRasterizer(rs)
    m = torch.zeros((4, 3))
    geo = dict(means3D=m, means2D=m, opacities=torch.ones((4, 1)), scales=torch.ones((4, 3)), rotations=torch.ones((4, 4)))
    text = "Please provide excatly one of either SHs or precomputed colors!"
    with pytest.raises(Exception, match=text):
        rast(dc=torch.zeros((4, 1, 3)), **geo)                                         # dc without shs
    with pytest.raises(Exception, match=text):
        rast(dc=torch.zeros((4, 1, 3)), colors_precomp=torch.zeros((4, 3)), **geo)     # dc with colours instead of shs
    with pytest.raises(Exception, match=text):
        rast(dc=torch.zeros((4, 1, 3)), shs=torch.zeros((4, 15, 3)), colors_precomp=torch.zeros((4, 3)), **geo)   # both sources
    with pytest.raises(Exception, match=text):
        rast(**geo)
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        rast(dc=torch.zeros((4, 1, 3)), shs=torch.zeros((4, 15, 3)), cov3D_precomp=torch.zeros((4, 6)), **geo)
    assert list(inspect.signature(accel.rasterize_gaussians).parameters)[:4] == ["means3D", "means2D", "dc", "sh"]
