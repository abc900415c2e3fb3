"""DNGaussian's per-Gaussian regulariser, view directions and near-camera mask without a GPU: the closed forms of
tests/dng_reg_reference.py (what the kernels of csrc/gs_dng_reg.hip evaluate) against torch CPU autograd of the composition
in float64 - values, gradients, tie rows, o == 0.2, an empty set, the raw form through exp and sigmoid, a gradcheck of the
directions; torch's own fp32 rules the formulas rest on; the dng_reg package surface, the header's constants, the ABI
additions and the argument checks of the Python layer and of the library, none of which needs a device."""
import inspect
import os
import re

import pytest
import torch

import dng_reg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("dng_reg_tmp_bytes", "dng_reg_fwd", "dng_reg_bwd", "view_dirs_fwd", "view_dirs_bwd", "near_mask")
F64 = torch.float64


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)


def _define(name):
    return int(re.search(r"#define\s+%s\s+(-?\d+)\b" % name, _header()).group(1))


def _close(got, want, scale, tol=1e-12):
    return bool(((got - want).abs() <= tol * scale + 1e-300).all())


def _autograd(s, o, g_terms, g_total, raw):
    ss, os_ = s.clone().requires_grad_(True), o.clone().requires_grad_(True)
    t = ref.terms_raw(ss, os_) if raw else ref.terms(ss, os_)
    loss = 0.0
    if g_terms is not None:
        loss = loss + (t * torch.tensor(g_terms, dtype=F64)).sum()
    if g_total is not None:
        loss = loss + g_total * ref.total(t)
    loss.backward()
    return t.detach(), ss.grad, os_.grad


# ---- the restatement against torch CPU autograd ----
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("g_terms,g_total", [(None, 1.0), ((1.0, 0.0, 0.0), None), ((0.0, 1.0, 0.0), None),
                                             ((0.0, 0.0, 1.0), None), ((0.3, -2.0, 0.7), 1.5)])
@pytest.mark.parametrize("P", [2, 8, 65, 1031])
def test_closed_form_equals_autograd(P, g_terms, g_total, raw):
    s, o = ref.scene(P, "mixed", seed=1, raw=raw)
    t, gs, go = _autograd(s, o, g_terms, g_total, raw)
    w = ref.regulariser_closed(s, o, ref.coefficients(g_terms, g_total), raw=raw)
    assert bool(torch.isfinite(t).all()) and _close(w["terms"], t, t.abs())
    assert _close(w["g_scaling"], gs, w["g_scaling_scale"]) and _close(w["g_opacity"], go, w["g_opacity_scale"])
    # a structurally zero element (scale 0) is zero in autograd's gradient too
    assert not gs[w["g_scaling_scale"] == 0].any() and not go[w["g_opacity_scale"] == 0].any()
    assert bool((w["g_scaling_scale"] >= w["g_scaling"].abs() * (1 - 1e-12)).all())


def test_tie_rows_send_the_gradient_to_the_lowest_column():
    s = torch.tensor([[1.0, 1.0, 1.0], [2.0, 3.0, 3.0], [2.0, 2.0, 3.0], [0.5, 0.25, 0.25]], dtype=F64)
    o = torch.tensor([0.9, 0.1, 0.5, 0.05], dtype=F64)
    for g_terms in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
        _, gs, _ = _autograd(s, o, g_terms, None, False)
        w = ref.regulariser_closed(s, o, g_terms)
        assert _close(w["g_scaling"], gs, w["g_scaling_scale"])
        assert bool(((gs != 0) <= (w["g_scaling_scale"] != 0)).all())
    w = ref.regulariser_closed(s, o, (1.0, 1.0, 0.0))
    nz = w["g_scaling_scale"] != 0
    assert nz.tolist() == [[True, False, False], [True, True, False], [True, False, True], [True, True, False]]
    # the all-tied row, the state training starts in: max and min are both column 0, the shape term's two parts cancel there
    assert abs(float(ref.regulariser_closed(s, o, (1.0, 0.0, 0.0))["g_scaling"][0, 0])) <= 1e-16
    # torch's fp32 max / min follow the same rule
    s32 = s.float().requires_grad_(True)
    (s32.max(dim=1).values / s32.min(dim=1).values).sum().backward()
    assert bool(((s32.grad != 0) <= nz).all())


def test_the_threshold_is_the_fp32_one_and_belongs_to_neither_set():
    o32 = torch.tensor([0.2, 0.9, 0.1], dtype=torch.float32)
    assert (o32 > 0.2).tolist() == [False, True, False] and (o32 < 0.2).tolist() == [False, False, True]
    assert float(o32[0]) == ref.THRESHOLD != 0.2
    s = torch.ones((3, 3), dtype=F64)
    o = o32.to(F64)
    _, _, go = _autograd(s, o, None, 1.0, False)
    w = ref.regulariser_closed(s, o, ref.coefficients(None, 1.0))
    assert float(go[0]) == 0.0 and float(w["g_opacity"][0]) == 0.0 and float(w["g_opacity_scale"][0]) == 0.0
    assert _close(w["g_opacity"], go, w["g_opacity_scale"]) and float(go[1]) != 0.0 and float(go[2]) != 0.0


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("kind", ["H_empty", "L_empty"])
@pytest.mark.parametrize("P", [1, 65])
def test_an_empty_set_is_nan_with_finite_gradients(P, kind, raw):
    s, o = ref.scene(P, kind, seed=2, raw=raw)
    t, gs, go = _autograd(s, o, None, 1.0, raw)
    w = ref.regulariser_closed(s, o, ref.coefficients(None, 1.0), raw=raw)
    assert torch.isnan(t).tolist() == [False, False, True] == torch.isnan(w["terms"]).tolist()
    assert bool(torch.isnan(ref.total(t)))
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(go).all()) and bool((go != 0).all())
    assert _close(w["terms"][:2], t[:2], t[:2].abs())
    assert _close(w["g_scaling"], gs, w["g_scaling_scale"]) and _close(w["g_opacity"], go, w["g_opacity_scale"])


def test_raw_scenes_keep_their_ties_and_their_distance_to_the_threshold():
    for P in (8, 65, 1031):
        rs, ro = ref.scene(P, "mixed", seed=3, raw=True)
        assert bool((rs[0::8] == rs[0::8, :1]).all())                      # all tied
        assert bool((rs[1::8, 1] == rs[1::8, 2]).all()) and bool((rs[1::8, 0] > rs[1::8, 1]).all())
        assert bool((rs[4::8, 1] == rs[4::8, 2]).all()) and bool((rs[4::8, 0] < rs[4::8, 1]).all())
        assert float((torch.sigmoid(ro) - ref.THRESHOLD).abs().min()) >= 1.5e-3
        o = torch.sigmoid(ro)
        assert bool((o > ref.THRESHOLD).any()) and bool((o < ref.THRESHOLD).any())
        assert bool((rs == rs.float().to(F64)).all()) and bool((ro == ro.float().to(F64)).all())


def test_view_dirs_gradcheck_and_closed_form():
    xyz, _, campos = ref.points(9, 3, seed=4)
    xs = xyz.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: ref.view_dirs(a, campos), (xs,))
    g = torch.randn((9, 3), generator=torch.Generator().manual_seed(5), dtype=F64)
    out = ref.view_dirs(xs, campos)
    out.backward(g)
    w = ref.view_dirs_closed(xyz, campos, g)
    assert _close(w["out"], out.detach(), torch.ones(())) and _close(w["g_xyz"], xs.grad, w["g_xyz_scale"])
    assert _close(w["out"].norm(dim=1), torch.ones(9, dtype=F64), torch.ones(()))
    # at the camera centre: a NaN row, that row only, as torch gives
    x32 = xyz.float()
    x32[4] = campos.float()
    d = x32 - campos.float()
    torch_rows = torch.isnan(d / d.norm(dim=1, keepdim=True)).all(dim=1)
    ours = torch.isnan(ref.view_dirs_closed(x32.to(F64), campos, g)["out"]).all(dim=1)
    assert torch_rows.tolist() == ours.tolist() == [i == 4 for i in range(9)]


@pytest.mark.parametrize("K", [1, 2, 120])
def test_near_mask_restatement_equals_the_camera_loop(K):
    near = 0.5
    xyz, centers, _ = ref.points(300, K, near=near, seed=6)
    want, gap = ref.near_mask(xyz, centers, near)
    assert gap >= 1e-5
    x32 = xyz.float()
    loop = None
    for k in range(K):   # the loop over cameras, in fp32
        m = (x32 - centers[k].float().repeat(x32.shape[0], 1)).norm(dim=1, keepdim=True) < near
        loop = loop + m if loop is not None else m
    assert torch.equal(loop.squeeze(1), want)
    assert bool(want[-1]) and not bool(want[0]) and 0 < int(want.sum()) < 300
    if K > 1:   # the last row is the last camera's alone
        assert not bool(ref.near_mask(xyz[-1:], centers[:-1], near)[0][0])


# ---- package surface, header, ABI ----
def test_package_names_and_signatures():
    import dng_reg
    assert dng_reg.__all__ == ["gaussian_regulariser", "gaussian_regulariser_raw", "view_dirs", "near_camera_mask"]
    for fn in (dng_reg.gaussian_regulariser, dng_reg.gaussian_regulariser_raw):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["scaling", "opacity", "shape_pena", "scale_pena", "opa_pena", "return_terms"]
        assert [sig.parameters[k].default for k in ("shape_pena", "scale_pena", "opa_pena", "return_terms")] == \
            [0.001, 0.001, 0.01, False]
    assert list(inspect.signature(dng_reg.view_dirs).parameters) == ["xyz", "campos"]
    assert list(inspect.signature(dng_reg.near_camera_mask).parameters) == ["xyz", "centers", "near"]
    assert ref.WEIGHTS == (0.001, 0.001, 0.01)


def test_python_constants_are_the_headers():
    from gsplat_amd import dng_reg as k
    assert k.RAW == _define("GS_DNG_REG_RAW")
    assert k.BLOCK_ROWS == _define("GS_DNG_REG_BLOCK_ROWS") and k.MAX_BLOCKS == _define("GS_DNG_REG_MAX_BLOCKS")


def test_abi_additions_are_declared_bound_exported_and_device_only():
    from gsplat_amd import capi
    from gsplat_amd._lib import LIB_PATH
    from test_abi import exported
    src = _header()
    have = exported(LIB_PATH, "gs_")
    for n in ABI:
        assert re.search(r"\bgs_%s\s*\(" % n, src), n
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
        assert "gs_" + n in have, n
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", src)


# ---- argument checks, none of which reaches a device ----
class _OnDevice:
    """Stands for a tensor on the device where there is none: shape, device and dtype are all the checks look at."""

    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

    def dim(self):
        return len(self.shape)


def test_wrong_shapes_raise_value_error():
    import dng_reg
    z = torch.zeros
    for fn in (dng_reg.gaussian_regulariser, dng_reg.gaussian_regulariser_raw):
        with pytest.raises(ValueError, match=r"\[P,3\]"):
            fn(z((8, 4)), z((8, 1)))
        with pytest.raises(ValueError, match=r"\[P,3\]"):
            fn(z((24,)), z((8,)))
        with pytest.raises(ValueError, match=r"\[P\] or \[P,1\]"):
            fn(z((8, 3)), z((8, 2)))
        with pytest.raises(ValueError, match="rows"):
            fn(z((8, 3)), z((9, 1)))
        with pytest.raises(ValueError, match="P = 0"):
            fn(z((0, 3)), z((0, 1)))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        dng_reg.view_dirs(z((8, 2)), z((3,)))
    with pytest.raises(ValueError, match=r"\[3\]"):
        dng_reg.view_dirs(z((8, 3)), z((1, 3)))
    with pytest.raises(ValueError, match="P = 0"):
        dng_reg.view_dirs(z((0, 3)), z((3,)))
    with pytest.raises(ValueError, match=r"\[K,3\]"):
        dng_reg.near_camera_mask(z((8, 3)), z((3,)), 0.5)
    with pytest.raises(ValueError, match="K = 0"):
        dng_reg.near_camera_mask(z((8, 3)), z((0, 3)), 0.5)
    with pytest.raises(ValueError, match="P = 0"):
        dng_reg.near_camera_mask(z((0, 3)), z((2, 3)), 0.5)


def test_cpu_tensors_raise():
    import dng_reg
    z = torch.zeros
    for call in (lambda: dng_reg.gaussian_regulariser(z((8, 3)), z((8, 1))),
                 lambda: dng_reg.gaussian_regulariser_raw(z((8, 3)), z((8,))),
                 lambda: dng_reg.view_dirs(z((8, 3)), z((3,))),
                 lambda: dng_reg.near_camera_mask(z((8, 3)), z((2, 3)), 0.5),
                 # a CPU tensor in either place, and before its dtype is looked at
                 lambda: dng_reg.view_dirs(_OnDevice((8, 3)), z((3,), dtype=F64)),
                 lambda: dng_reg.gaussian_regulariser(z((8, 3), dtype=F64), _OnDevice((8, 1)))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


def test_fp64_tensors_raise():
    from gsplat_amd import dng_reg as k
    for check, args in ((k.check_regulariser, (_OnDevice((8, 3), F64), _OnDevice((8, 1)))),
                        (k.check_regulariser, (_OnDevice((8, 3)), _OnDevice((8,), F64))),
                        (k.check_view_dirs, (_OnDevice((8, 3)), _OnDevice((3,), torch.float16))),
                        (k.check_near_mask, (_OnDevice((8, 3), F64), _OnDevice((2, 3), F64)))):
        with pytest.raises(RuntimeError, match="fp32 only"):
            check("f", *args)
    # shapes are looked at first
    with pytest.raises(ValueError):
        k.check_regulariser("f", _OnDevice((8, 2), F64), _OnDevice((8, 1), F64))
    assert k.check_regulariser("f", _OnDevice((8, 3)), _OnDevice((8, 1))) == 8
    assert k.check_near_mask("f", _OnDevice((8, 3)), _OnDevice((2, 3))) == (8, 2)


def test_library_argument_checks():
    from gsplat_amd import dng_reg as k
    from gsplat_amd._lib import hip_api
    api = hip_api()
    size = api.raw("dng_reg_tmp_bytes")
    assert size(0) == 0 and size(-1) == 0 and size((1 << 40) + 1) == 0 and size(1) > 0
    # one partial per workgroup and no more workgroups than the cap: the scratch stops growing where the grid does
    B, G = k.BLOCK_ROWS, k.MAX_BLOCKS
    assert size(B) == size(1) and size(64 * B) > size(B)
    assert size(G * B) == size(G * B + 1) == size(100 * G * B) > size((G - 16) * B)
    fwd, bwd = api.raw("dng_reg_fwd"), api.raw("dng_reg_bwd")
    one = 16  # any non-null address: the checks below return before anything is launched
    assert fwd(None, None, 8, 1.0, 1.0, 1.0, 0, 0, None, None, None) == -1          # GS_E_NULL
    assert fwd(one, one, 8, 1.0, 1.0, 1.0, 0, 0, one, None, None) == -1
    assert fwd(one, one, 0, 1.0, 1.0, 1.0, 0, 0, one, one, None) == -2              # GS_E_SHAPE: P < 1
    assert fwd(one, one, 8, 1.0, 1.0, 1.0, 2, 0, one, one, None) == -2              # an unknown flag
    assert fwd(one, one, 8, 1.0, 1.0, 1.0, 0, -1, one, one, None) == -2             # max_blocks < 0
    assert bwd(one, one, 0, 0, one, one, one, one, one, None) == -2
    assert bwd(one, one, 8, 4, one, one, one, one, one, None) == -2
    assert bwd(one, one, 8, 0, None, one, one, one, one, None) == -1
    assert bwd(one, one, 8, 0, one, None, None, one, one, None) == -1               # no incoming gradient
    assert bwd(one, one, 8, 0, one, one, one, None, None, None) == -1               # no gradient asked for
    vf, vb, nm = api.raw("view_dirs_fwd"), api.raw("view_dirs_bwd"), api.raw("near_mask")
    assert vf(one, one, 0, one, None) == -2 and vf(one, None, 8, one, None) == -1 and vf(one, one, 8, None, None) == -1
    assert vb(one, one, 0, one, one, None) == -2 and vb(one, one, 8, None, one, None) == -1
    assert nm(one, 0, one, 1, 0.5, one, None) == -2 and nm(one, 8, one, 0, 0.5, one, None) == -2   # P = 0, K = 0
    assert nm(one, 8, None, 1, 0.5, one, None) == -1 and nm(one, 8, one, 1, 0.5, None, None) == -1
