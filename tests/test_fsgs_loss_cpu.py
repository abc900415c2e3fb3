"""FSGS's depth-correlation term and proximity unpooling without a GPU: the float64 restatement
(tests/fsgs_loss_reference.py) against torch.corrcoef, its gradcheck, the closed form the backward kernel evaluates, the
gap between the two forms on every scene the GPU file holds the branch on, the fsgs_loss package surface, the ABI additions,
and GaussianModelLite.proximity on the CPU (the oracle's kNN) against the literal restatement, bit for bit."""
import inspect
import os
import re

import pytest
import torch

import fsgs_loss_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("A", "B", "offset", "exact+", "exact-", "constant")
ABI = ("pearson_tmp_bytes", "pearson_fwd", "pearson_bwd")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)


def _define(name):
    return int(re.search(r"#define\s+%s\s+(-?\d+)\b" % name, _header()).group(1))


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---- the restatement ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 65), (7, 9), (378, 504)])
def test_restatement_equals_torch_corrcoef(kind, shape):
    x, m = ref.scene(*shape, kind, seed=1)
    for name in ref.FORMS:
        y = ref.form(m, name)
        got = ref.pearson(x, y)
        want = torch.corrcoef(torch.stack((x.reshape(-1), y.reshape(-1))))[0, 1]
        if kind == "constant":
            assert bool(torch.isnan(got)) and bool(torch.isnan(want))
        else:
            assert abs(float(got) - float(want)) <= 1e-12, (name, float(got), float(want))
            assert -1.0 <= float(got) <= 1.0


def test_exact_scenes_are_exact_and_two_elements_are_degenerate():
    for shape in [(1, 2), (1, 65), (378, 504)]:
        x, m = ref.scene(*shape, "exact+", seed=2)
        assert abs(float(ref.pseudo_depth_pearson_loss(x, m))) <= 1e-12
        x, m = ref.scene(*shape, "exact-", seed=2)
        assert abs(float(ref.pseudo_depth_pearson_loss(x, m)) - 2.0) <= 1e-12
    x, m = ref.scene(1, 2, "A", seed=2)
    assert abs(abs(float(ref.pearson(x, m))) - 1.0) <= 1e-12


def test_min_rule_is_pythons():
    def t(v):
        return torch.tensor(float(v))
    for a, b, branch in ((t(1), t(2), 0), (t(2), t(1), 1), (t(1), t(1), 0), (t("nan"), t(1), 0), (t(1), t("nan"), 0)):
        value, got = ref.py_min(a, b)
        assert value is min(a, b) and got == branch and (value is b) == bool(branch)


@pytest.mark.parametrize("kind", ["A", "B", "offset"])
def test_restatement_gradcheck(kind):
    x, m = ref.scene(3, 5, kind, seed=3)
    xs = x.clone().requires_grad_(True)
    ms = m.clone().requires_grad_(True)
    for name in ref.FORMS:
        assert torch.autograd.gradcheck(lambda a, b: ref.pearson(a, ref.form(b, name)), (xs, ms))
    assert torch.autograd.gradcheck(lambda a: ref.depth_pearson_loss(a, m), (xs,))
    assert torch.autograd.gradcheck(ref.pseudo_depth_pearson_loss, (xs, ms))


@pytest.mark.parametrize("kind", ["A", "B", "offset"])
def test_backward_closed_form_is_the_autograd_gradient(kind):
    x, m = ref.scene(40, 53, kind, seed=4)
    for name in ref.FORMS:
        xs = x.clone().requires_grad_(True)
        ys = ref.form(m, name).clone().requires_grad_(True)
        ref.pearson(xs, ys).backward()
        gx, gy = ref.pearson_grad(x, ref.form(m, name))
        assert _rel(gx, xs.grad) < 1e-12 and _rel(gy, ys.grad) < 1e-12


def test_clamp_does_not_gate_the_gradient():
    """On an exact scene r sits on the clamp's edge (rounding puts it on either side): the gradient is the unclamped one."""
    for kind in ("exact+", "exact-"):
        x, m = ref.scene(1, 65, kind, seed=5)
        grads = []
        for clamp in (True, False):
            xs = x.clone().requires_grad_(True)
            ref.pearson(xs, -m, clamp=clamp).backward()
            grads.append(xs.grad)
        assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0.0
        assert abs(float(ref.pearson(x, -m))) == 1.0 or abs(float(ref.pearson(x, -m, clamp=False))) < 1.0


def test_shifted_float64_sums_survive_an_offset_where_raw_fp32_moments_do_not():
    """Why the kernel adds float64 sums of the values shifted by the first element: x = 1000 + 0.01 noise."""
    x, m = ref.scene(378, 504, "offset", seed=6)
    want = float(ref.pearson(x, -m))
    x32, y32 = x.float().reshape(-1), (-m).float().reshape(-1)
    n = x32.numel()
    raw = (n * (x32 * y32).sum() - x32.sum() * y32.sum()) / torch.sqrt(
        (n * (x32 * x32).sum() - x32.sum() ** 2) * (n * (y32 * y32).sum() - y32.sum() ** 2))
    assert not abs(float(raw) - want) <= 1e-3  # NaN or far off
    dx, dy = x.reshape(-1) - x.reshape(-1)[0], (-m).reshape(-1) - (-m).reshape(-1)[0]
    sxx = (dx * dx).sum() - dx.sum() ** 2 / n
    syy = (dy * dy).sum() - dy.sum() ** 2 / n
    sxy = (dx * dy).sum() - dx.sum() * dy.sum() / n
    assert abs(float(sxy / torch.sqrt(sxx * syy)) - want) <= 1e-12


def test_gpu_scenes_have_a_form_gap():
    """A branch disagreement on these scenes would move the loss by >= 0.01, a thousand loss bars: it cannot hide."""
    import test_gpu_fsgs_loss as gpu
    assert len(gpu.AB_SIZES) >= 11
    for size in gpu.AB_SIZES:
        for kind, winner in (("A", 0), ("B", 1)):
            x, m = gpu.inputs(size, kind)
            a = float(1 - ref.pearson(-m, x))
            b = float(1 - ref.pearson(1 / (m + 200.), x))
            assert abs(a - b) >= 0.01, (size, kind, a, b)
            assert ref.depth_pearson_loss(x, m, return_branch=True)[1] == winner, (size, kind)


# ---- package surface ----
def test_package_names_and_signatures():
    import fsgs_loss
    assert set(fsgs_loss.__all__) == {"pearson_corrcoef", "depth_pearson_loss", "pseudo_depth_pearson_loss"}
    assert list(inspect.signature(fsgs_loss.pearson_corrcoef).parameters) == ["preds", "target"]
    sig = inspect.signature(fsgs_loss.depth_pearson_loss)
    assert list(sig.parameters) == ["rendered_depth", "midas_depth", "return_branch"]
    assert sig.parameters["return_branch"].default is False
    assert list(inspect.signature(fsgs_loss.pseudo_depth_pearson_loss).parameters) == ["rendered_depth", "midas_depth"]


def test_shapes_outside_the_contract_raise_value_error():
    import fsgs_loss
    with pytest.raises(ValueError, match=r"\[N\] or \[N,1\]"):
        fsgs_loss.pearson_corrcoef(torch.zeros((8, 2)), torch.zeros((8, 2)))
    with pytest.raises(ValueError, match=r"\[N\] or \[N,1\]"):
        fsgs_loss.pearson_corrcoef(torch.zeros((8,)), torch.zeros((4, 2)))
    for fn in (fsgs_loss.pearson_corrcoef, fsgs_loss.depth_pearson_loss, fsgs_loss.pseudo_depth_pearson_loss):
        with pytest.raises(ValueError, match="elements"):
            fn(torch.zeros((8,)), torch.zeros((9,)))
        with pytest.raises(ValueError, match="at least 2"):
            fn(torch.zeros((1,)), torch.zeros((1,)))
    with pytest.raises(ValueError, match="elements"):
        fsgs_loss.depth_pearson_loss(torch.zeros((4, 6)), torch.zeros((4, 5)))


def test_cpu_tensors_raise():
    import fsgs_loss
    for fn in (fsgs_loss.pearson_corrcoef, fsgs_loss.pseudo_depth_pearson_loss):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros((8, 1)), torch.zeros((8, 1)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fsgs_loss.depth_pearson_loss(torch.zeros((4, 6)), torch.zeros((4, 6)))   # [H,W] is accepted: the device is what fails


def test_midas_depth_requiring_grad_raises():
    import fsgs_loss
    with pytest.raises(RuntimeError, match="no gradient to midas_depth"):
        fsgs_loss.depth_pearson_loss(torch.zeros((8,)), torch.zeros((8,), requires_grad=True))


# ---- ABI additions ----
def test_abi_additions_are_declared_bound_and_device_only():
    from gsplat_amd import capi
    src = _header()
    for n in ABI:
        assert re.search(r"\bgs_%s\s*\(" % n, src), n
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", src)


def test_python_constants_are_the_headers():
    from gsplat_amd import pearson
    assert (pearson.ID, pearson.NEG, pearson.RECIP200) == (_define("GS_PEARSON_ID"), _define("GS_PEARSON_NEG"),
                                                           _define("GS_PEARSON_RECIP200"))
    assert pearson.WRT_R == _define("GS_PEARSON_WRT_R")
    assert pearson.BLOCK_ELEMS == _define("GS_PEARSON_BLOCK_ELEMS") and pearson.MAX_BLOCKS == _define("GS_PEARSON_MAX_BLOCKS")


def test_host_side_argument_checks():
    from gsplat_amd import pearson
    from gsplat_amd._lib import hip_api
    api = hip_api()
    size = api.raw("pearson_tmp_bytes")
    assert size(0) == 0 and size(1) == 0 and size(2) > 0
    # one partial per workgroup, and no more workgroups than the cap: the scratch stops growing where the grid does
    B, G = pearson.BLOCK_ELEMS, pearson.MAX_BLOCKS
    assert size(B) == size(2) and size(4 * B + 1) > size(4 * B)
    assert size(G * B) == size(G * B + 1) == size(100 * G * B) > size((G - 4) * B)
    fwd, bwd = api.raw("pearson_fwd"), api.raw("pearson_bwd")
    assert fwd(None, None, 8, 0, -1, None, None, None, None) == -1       # GS_E_NULL
    assert fwd(None, None, 1, 0, -1, None, None, None, None) == -2       # GS_E_SHAPE: n < 2
    assert fwd(None, None, 8, 3, -1, None, None, None, None) == -2       # an unknown form
    assert fwd(None, None, 8, 0, -2, None, None, None, None) == -2
    assert bwd(None, None, 8, 0, -1, 0, None, None, None, None, None) == -1
    assert bwd(None, None, 1, 0, -1, 0, None, None, None, None, None) == -2
    assert bwd(None, None, 8, 0, -1, 2, None, None, None, None, None) == -2   # an unknown flag
    one = 16  # any non-null address: the checks below return before anything is launched
    assert bwd(one, one, 8, 1, 2, 0, one, one, one, one, None) == -5      # GS_E_UNSUPPORTED: grad_t through RECIP200
    assert bwd(one, one, 8, 2, -1, 0, one, one, None, one, None) == -5
    assert bwd(one, one, 8, 1, -1, 0, one, one, None, None, None) == -1   # no gradient asked for


# ---- proximity unpooling ----
def _model(oracle, P=400, seed=3, duplicates=0, **kw):
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import GaussianModelLite
    sc = synthetic.trained_like(P, seed=seed, scale_mult=1.5)
    m = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api, **kw)
    g = torch.Generator().manual_seed(seed)
    for _ in range(3):  # non-trivial Adam moments
        m.flat_grad.copy_(torch.randn(m.flat.numel(), generator=g) * 1e-2)
        m.optimizer.step()
    if duplicates:  # the same centre twice: zero distances, ties in the neighbour lists
        with torch.no_grad():
            m.params["xyz"][P - duplicates:] = m.params["xyz"][:duplicates]
    m.xyz_gradient_accum = torch.rand((P, 1), generator=g)
    m.denom = torch.ones((P, 1))
    m.max_radii2D = torch.rand((P,), generator=g) * 50
    return m


def _state(m):
    from gsplat_amd.trainer import FIELDS
    opt = m.optimizer
    m1, m2 = opt.field_views(opt.exp_avg), opt.field_views(opt.exp_avg_sq)
    return ({k: m.params[k].detach().reshape(m.P, n).clone() for k, n in FIELDS}, {k: m1[k].clone() for k, _ in FIELDS},
            {k: m2[k].clone() for k, _ in FIELDS})


@pytest.mark.parametrize("extent,duplicates", [(0.02, 0), (0.05, 0), (0.1, 0), (0.01, 40)])
def test_proximity_equals_the_literal_restatement(oracle, extent, duplicates):
    from gsplat_amd.knn import dist2_with_indices
    from gsplat_amd.trainer import FIELDS
    m = _model(oracle, duplicates=duplicates, spatial_order=False)
    P0 = m.P
    p0, a0, b0 = _state(m)
    dist, nearest = dist2_with_indices(oracle.api, p0["xyz"])
    want, sel = ref.proximity(p0["xyz"], p0["scaling"], p0["opacity"], p0["rotation"], p0["features"].reshape(P0, 16, 3),
                              dist, nearest, extent)
    S = int(sel.sum())
    if extent == 0.1:
        assert S == 0
    else:
        assert 1 < S < P0, "the extent must select some rows and not all"
    if duplicates:
        twins = (p0["xyz"][nearest[:, 0].long()] == p0["xyz"]).all(dim=1)
        assert int(twins.sum()) == 2 * duplicates and int((twins & sel).sum()) > 0
    generation = m.generation
    n_new = m.proximity(extent)
    assert n_new == 3 * S and m.P == P0 + 3 * S and m.generation > generation
    p1, a1, b1 = _state(m)
    for k, n in FIELDS:
        assert torch.equal(p1[k][:P0], p0[k]) and torch.equal(a1[k][:P0], a0[k]) and torch.equal(b1[k][:P0], b0[k]), k
        assert torch.equal(p1[k][P0:], want[k].reshape(3 * S, n)), k
        assert not a1[k][P0:].any() and not b1[k][P0:].any(), k
    for stat, shape in ((m.xyz_gradient_accum, (m.P, 1)), (m.denom, (m.P, 1)), (m.max_radii2D, (m.P,))):
        assert tuple(stat.shape) == shape and not stat.any()
    assert all(p.grad is None for p in m.params.values())
    if S:
        # new row j: neighbour entry j of the flattened lists, midway to selected row j % S (the reference's tiling)
        rows = sel.nonzero().squeeze(1)
        j = 3 * S - 1
        assert torch.equal(p1["xyz"][P0 + j], (p0["xyz"][rows[j % S]] + p0["xyz"][nearest[rows[j // 3], j % 3].long()]) / 2)
        assert torch.equal(p1["rotation"][P0:], torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(3 * S, 1))


def test_proximity_keeps_the_spatial_order(oracle):
    """With spatial_order the rows end up in Morton order of the centres, as after densify_and_prune."""
    from gsplat_amd import synthetic
    m = _model(oracle, spatial_order=True)
    P0 = m.P
    old = sorted(map(tuple, m.params["xyz"].detach().tolist()))
    n_new = m.proximity(0.02)
    assert n_new > 0 and m.P == P0 + n_new
    xyz = m.params["xyz"].detach()
    assert torch.equal(synthetic.morton_order(xyz), torch.arange(m.P))
    assert set(old) <= set(map(tuple, xyz.tolist()))
    assert not m.xyz_gradient_accum.any() and not m.denom.any() and not m.max_radii2D.any()


def test_proximity_with_nir_raises(oracle):
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import GaussianModelLite
    m = GaussianModelLite(synthetic.trained_like(64, seed=0), torch.device("cpu"), api=oracle.api, with_nir=True)
    with pytest.raises(NotImplementedError):
        m.proximity(0.02)
