"""DNGaussian's depth-normalisation losses without a GPU: the float64 restatement (tests/dng_depth_reference.py) against
fixtures recorded by executing the reference's own functions (tests/golden/dng_depth.npz), its imposed-mask form, its
gradcheck, the closed form the backward kernel evaluates, the dng_loss package surface and the ABI additions."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import dng_depth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dng_depth.npz")
NAMES = ("patch_norm_mse_loss", "patch_norm_mse_loss_global", "patch_norm_l1_loss", "patch_norm_l1_loss_global")
ABI = ("depth_norm_tmp_bytes", "depth_norm_fwd", "depth_norm_bwd", "depth_smooth_fwd", "depth_smooth_bwd",
       "dng_depth_reg_fwd", "dng_depth_reg_bwd")


def golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))


def _inputs(z):
    return torch.from_numpy(z["depth"]).double(), torch.from_numpy(z["mono"]).double()


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _cases():
    return [pytest.param(c, id="%s-p%d-m%g" % (c["loss"], c["p"], c["margin"])) for c in golden()[1] if c["key"] != "empty"]


def test_fixture_covers_what_it_should():
    _, cases = golden()
    real = [c for c in cases if c["key"] != "empty"]
    assert {c["p"] for c in real} == {5, 8, 17} and {c["loss"] for c in real} == set(ref.FORMS)
    for p in (5, 8, 17):
        assert {c["margin"] for c in real if c["p"] == p} == {0.00025, 0.01, 0.2}
    for name in ref.FORMS:
        assert {c["margin"] for c in real if c["loss"] == name} == {0.00025, 0.01, 0.2}
    assert os.path.getsize(GOLDEN) < (1 << 20)


@pytest.mark.parametrize("case", _cases())
def test_restatement_equals_the_recorded_reference(case):
    z, _ = golden()
    depth, mono = _inputs(z)
    glob, l1 = ref.FORMS[case["loss"]]
    x = depth.clone().requires_grad_(True)
    loss, mask, d = ref.patch_norm_loss(x, mono, case["p"], case["margin"], glob, l1, return_all=True)
    loss.backward()
    k = case["key"]
    want_mask = torch.from_numpy(z[k + "_mask"])
    assert mask.shape == want_mask.shape == ((64 // case["p"]) * (80 // case["p"]), case["p"] ** 2)
    assert torch.equal(mask, want_mask)
    assert abs(float(loss.detach()) - float(z[k + "_loss"])) <= 1e-10 * abs(float(z[k + "_loss"]))
    assert _rel(x.grad, torch.from_numpy(z[k + "_grad"])) <= 1e-10
    dk = "d_p%d_%s" % (case["p"], "global" if glob else "local")
    if dk in z.files:
        assert _rel(d.detach(), torch.from_numpy(z[dk])) <= 1e-10
    # the imposed-mask form with its own mask is the free form
    x2 = depth.clone().requires_grad_(True)
    loss2 = ref.patch_norm_loss(x2, mono, case["p"], case["margin"], glob, l1, mask=mask)
    loss2.backward()
    assert float(loss2.detach()) == float(loss.detach()) and torch.equal(x2.grad, x.grad)


def test_named_forms_are_the_flag_forms():
    z, _ = golden()
    depth, mono = _inputs(z)
    for name, (glob, l1) in ref.FORMS.items():
        fn = getattr(ref, "patch_norm_%s" % name.replace("mse", "mse_loss").replace("l1", "l1_loss"))
        a, m = fn(depth, mono, 8, 0.01, return_mask=True)
        b, mb, _ = ref.patch_norm_loss(depth, mono, 8, 0.01, glob, l1, return_all=True)
        assert float(a) == float(b) and torch.equal(m, mb)


def test_empty_mask_is_nan_with_a_zero_gradient():
    z, _ = golden()
    depth, mono = _inputs(z)
    assert np.isnan(float(z["empty_loss"])) and not z["empty_mask"].any() and float(np.abs(z["empty_grad"]).max()) == 0.0
    x = depth.clone().requires_grad_(True)
    loss, mask = ref.patch_norm_mse_loss(x, mono, 8, 1e9, return_mask=True)
    loss.backward()
    assert bool(torch.isnan(loss)) and not bool(mask.any())
    assert x.grad.shape == depth.shape and float(x.grad.abs().max()) == 0.0


def test_imposed_mask_replaces_the_threshold():
    z, _ = golden()
    depth, mono = _inputs(z)
    _, free, d = ref.patch_norm_loss(depth, mono, 8, 0.2, return_all=True)
    other = ~free
    loss = ref.patch_norm_loss(depth, mono, 8, 0.2, mask=other)
    assert abs(float(loss) - float((d[other] ** 2).mean())) < 1e-15
    assert float(d[other].abs().max()) <= 0.2  # elements the threshold would never have taken


@pytest.mark.parametrize("tag,img", [("smooth_mono", "mono"), ("smooth_rgb", "rgb")])
def test_smoothness_equals_the_recorded_reference(tag, img):
    z, _ = golden()
    depth, _ = _inputs(z)
    x = depth.clone().requires_grad_(True)
    loss = ref.loss_depth_smoothness(x, torch.from_numpy(z[img]).double())
    loss.backward()
    assert abs(float(loss) - float(z[tag + "_loss"])) <= 1e-10 * abs(float(z[tag + "_loss"]))
    assert _rel(x.grad, torch.from_numpy(z[tag + "_grad"])) <= 1e-10


@pytest.mark.parametrize("name", sorted(ref.FORMS))
def test_restatement_gradcheck(name):
    glob, l1 = ref.FORMS[name]
    depth, mono = ref.scene(7, 9, seed=2)
    x = depth.clone().requires_grad_(True)
    mask = ref.patch_norm_loss(depth, mono, 3, 0.1, glob, l1, return_all=True)[1]
    assert 0 < int(mask.sum()) < mask.numel()
    # (the mask is held fixed: the loss is differentiable in the input only between threshold crossings; so is the global
    #  form's whole-image std, which the reference detaches)
    std = depth.std() if glob else None
    assert torch.autograd.gradcheck(lambda a: ref.patch_norm_loss(a, mono, 3, 0.1, glob, l1, mask=mask, input_std=std), (x,))


def test_smoothness_gradcheck():
    depth, mono = ref.scene(6, 7, seed=3)
    x = depth.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: ref.loss_depth_smoothness(a, mono), (x,))


def closed_form_grad(x, t, p, margin, glob, l1):
    """What the backward kernel evaluates: from the per-patch sums G = sum g, Q = sum g (x - m) and the two
    scalars T = sum_l Q_l / D_l^2 and the cropped mean M,
        dL/dx_j = [ (g_j - G_l / n) / D_l  -  (local) Q_l / D_l^2 c_j / ((n - 1) s_l)  -  0.01 (x_j - M) / ((N - 1) std_all) T ] / count
    with g = f'(d) on the mask."""
    X, Tt = ref.patches(x, p), ref.patches(t, p)
    n, N = X.shape[1], X.numel()
    d = ref.normalised_difference(x, t, p, glob)
    mask = d.abs() > margin
    g = torch.where(mask, torch.sign(d) if l1 else 2 * d, torch.zeros_like(d))
    m = X.mean(1, keepdim=True)
    c = X - m
    s = (c ** 2).sum(1, keepdim=True).div(n - 1).sqrt()
    M = X.mean()
    sig = ((X - M) ** 2).sum().div(N - 1).sqrt()
    D = (x.std() if glob else s) + 1e-2 * sig
    D = D.expand_as(s)
    G, Q = g.sum(1, keepdim=True), (g * c).sum(1, keepdim=True)
    T = (Q / D ** 2).sum()
    out = (g - G / n) / D - 1e-2 * (X - M) / ((N - 1) * sig) * T
    if not glob:
        out = out - Q / D ** 2 * c / ((n - 1) * s)
    out = out / mask.sum()
    H, W = x.shape[2], x.shape[3]
    ny, nx = H // p, W // p
    full = torch.zeros((H, W), dtype=x.dtype)
    full[:ny * p, :nx * p] = out.reshape(ny, nx, p, p).permute(0, 2, 1, 3).reshape(ny * p, nx * p)
    return full[None, None]


@pytest.mark.parametrize("name", sorted(ref.FORMS))
@pytest.mark.parametrize("p", [5, 17])
def test_backward_closed_form_is_the_autograd_gradient(name, p):
    glob, l1 = ref.FORMS[name]
    depth, mono = ref.scene(40, 53, seed=4)
    x = depth.clone().requires_grad_(True)
    ref.patch_norm_loss(x, mono, p, 0.05, glob, l1).backward()
    assert _rel(closed_form_grad(depth, mono, p, 0.05, glob, l1), x.grad) < 1e-12


def test_scene_is_of_the_stated_kind():
    depth, mono = ref.scene(378, 504, seed=0)
    assert 2.0 < float(depth.mean()) < 4.5 and 0.5 < float(depth.std()) < 2.0
    assert 90.0 < float(mono.mean()) < 160.0 and 20.0 < float(mono.std()) < 80.0


# ---- package surface ----
def test_package_names_and_signatures():
    import dng_loss
    for n in NAMES:
        assert list(inspect.signature(getattr(dng_loss, n)).parameters) == ["input", "target", "patch_size", "margin",
                                                                             "return_mask"]
        assert inspect.signature(getattr(dng_loss, n)).parameters["return_mask"].default is False
    assert list(inspect.signature(dng_loss.loss_depth_smoothness).parameters) == ["depth", "img"]
    sig = inspect.signature(dng_loss.depth_regulariser)
    assert list(sig.parameters)[:8] == ["depth", "depth_mono", "p_local", "p_global", "margin", "w_local", "w_global",
                                        "w_smooth"]
    assert (sig.parameters["w_local"].default, sig.parameters["w_global"].default, sig.parameters["w_smooth"].default) == (
        0.1, 1.0, 0.0)
    assert set(dng_loss.__all__) == set(NAMES) | {"loss_depth_smoothness", "depth_regulariser"}


def test_shapes_outside_the_contract_raise_value_error():
    import dng_loss
    two = torch.zeros((2, 1, 16, 16))
    one = torch.zeros((1, 1, 16, 16))
    for n in NAMES:
        with pytest.raises(ValueError, match="batch 1 only"):
            getattr(dng_loss, n)(two, two, 4, 0.01)
        with pytest.raises(ValueError, match="one channel only"):
            getattr(dng_loss, n)(torch.zeros((1, 3, 16, 16)), torch.zeros((1, 3, 16, 16)), 4, 0.01)
        with pytest.raises(ValueError, match="patch size"):
            getattr(dng_loss, n)(one, one, 17, 0.01)
    with pytest.raises(ValueError, match="batch 1 only"):
        dng_loss.depth_regulariser(two, two, 4, 5, 0.01)
    with pytest.raises(ValueError, match="batch 1 only"):
        dng_loss.loss_depth_smoothness(two, two)


def test_cpu_tensors_raise():
    import dng_loss
    one = torch.zeros((1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_loss.patch_norm_mse_loss(one, one, 4, 0.01)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_loss.loss_depth_smoothness(one, one)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dng_loss.depth_regulariser(one, one, 4, 5, 0.01)


# ---- ABI additions ----
def test_abi_additions_are_declared_bound_and_device_only():
    from gsplat_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)
    for n in ABI:
        assert re.search(r"\bgs_%s\s*\(" % n, src), n
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", src)


def test_host_side_argument_checks():
    from gsplat_amd._lib import hip_api
    api = hip_api()
    size = api.raw("depth_norm_tmp_bytes")
    assert size(378, 504, 5, 17) > size(378, 504, 5, 0) > size(378, 504, 0, 0) > 0
    assert size(378, 504, 1, 0) == 0 and size(378, 504, 379, 0) == 0 and size(0, 504, 5, 0) == 0
    assert size(378, 504, 378, 378) > 0
    assert api.raw("depth_norm_fwd")(None, None, 32, 32, 4, 0.1, 0, None, None, None, None) == -1   # GS_E_NULL
    assert api.raw("depth_norm_fwd")(None, None, 32, 32, 33, 0.1, 0, None, None, None, None) == -2  # GS_E_SHAPE
    assert api.raw("depth_norm_fwd")(None, None, 32, 32, 4, 0.1, 4, None, None, None, None) == -2
    assert api.raw("depth_smooth_fwd")(None, None, 0, 32, 32, None, None, None) == -2
    assert api.raw("dng_depth_reg_bwd")(None, None, 32, 32, 4, 0, 0.1, 0.1, 1.0, 0.1, None, None, None, None) == -2
    assert api.raw("dng_depth_reg_fwd")(None, None, 32, 32, 4, 5, 0.1, 0.1, 1.0, 0.1, None, None, None, None, None) == -1
