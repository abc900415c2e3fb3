"""FSGS's depth-correlation term (csrc/gs_pearson.hip through the fsgs_loss package) and GaussianModelLite.proximity on the
MI355X, against the float64 restatement (tests/fsgs_loss_reference.py).

(a) values: loss within 1e-5 max(1, |loss|), gradient within 1e-4 of the tensor's largest entry, no element exempt (the bars
    of tests/test_gpu_dng_depth.py).
(b) the chosen branch equals the restatement's on every A / B scene (tests/test_fsgs_loss_cpu.py holds the two forms of
    these very scenes at least 0.01 apart: a wrong branch cannot pass (a)).
(c) exact scenes (r = +-1): loss within the bar of 0 or 2, gradient finite and every entry within
    1e-4 max|y_i - mean y| / sqrt(Sxx Syy) - the size of the gradient's first term, which its second cancels; a bar
    relative to the true gradient means nothing where that is zero.
(d) a constant sequence: NaN loss, all-zero gradient.
(e) two runs give the same bits.
(f) an upstream factor of 2 doubles the gradient exactly, one of 0.3 scales it within (a).
(g) the pseudo-view loss gives both gradients; the one to the target is minus what pearson_corrcoef(d, -m) sends to m.
(h) proximity on a CUDA model = the CPU run of the same model with the oracle's kNN, bit for bit.
(i) forward and backward on a side stream, no synchronize in between: they complete, with the default stream's bits.
Sizes: 2 (exact scenes only), a wave +- 1, what one workgroup sweeps +- 1, what the largest grid sweeps in one pass +- 1
(from the kernel's constants), 378x504, 1080x1920.  Every restatement result is computed once and shared.
The measured distances go to profiles/fsgs_loss_parity.json (or to the file FSGS_LOSS_PARITY_OUT names)."""
import json
import os

import pytest
import torch

import fsgs_loss_reference as ref
from gsplat_amd import pearson as _k

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BAR, GRAD_BAR = 1e-5, 1e-4
BLOCK, GRID = _k.BLOCK_ELEMS, _k.BLOCK_ELEMS * _k.MAX_BLOCKS
AB_SIZES = (63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, GRID - 1, GRID, GRID + 1, (378, 504), (1080, 1920))
OTHER_SIZES = (65, BLOCK + 1, (378, 504))
PARITY = {}
_inputs, _wants = {}, {}


def _hw(size):
    return size if isinstance(size, tuple) else (1, size)


def _sid(size):
    return "%dx%d" % size if isinstance(size, tuple) else str(size)


def inputs(size, kind):
    """(x, m) float64 CPU [H, W], the same numbers as their float32 form."""
    key = (size, kind)
    if key not in _inputs:
        H, W = _hw(size)
        _inputs[key] = ref.scene(H, W, kind, seed=H + W + len(kind))
    return _inputs[key]


def want(fn, size, kind):
    """The float64 restatement, once per (function, scene): dict(value, branch, gx, gm, first) - first = the size of the
    gradient's first term, max|y_i - mean y| / sqrt(Sxx Syy) over the chosen form."""
    key = (fn, size, kind)
    if key in _wants:
        return _wants[key]
    x, m = inputs(size, kind)
    xs = x.clone().requires_grad_(True)
    ms = m.clone().requires_grad_(fn != "depth")
    branch = None
    if fn == "depth":
        value, branch = ref.depth_pearson_loss(xs, ms, return_branch=True)
        y = ref.form(m, ("NEG", "RECIP200")[branch])
    elif fn == "pseudo":
        value, y = ref.pseudo_depth_pearson_loss(xs, ms), -m
    else:
        value, y = ref.pearson(xs, ms), m
    if not bool(torch.isnan(value)):
        value.backward()
    _, yc, sxx, syy, _ = ref.sums(x, y)
    _wants[key] = dict(value=float(value.detach()), branch=branch, gx=xs.grad, gm=ms.grad,
                       first=float(yc.abs().max() / torch.sqrt(sxx * syy)), r_abs=abs(float(ref.pearson(x, y))))
    return _wants[key]


def run_hip(fn, size, kind, upstream=None, stream=None):
    """-> (value, branch or None, grad x, grad m or None), all on the CPU."""
    import fsgs_loss
    dev = torch.device("cuda:0")
    x64, m64 = inputs(size, kind)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        x = x64.float().to(dev).requires_grad_(True)
        m = m64.float().to(dev).requires_grad_(fn != "depth")
        branch = None
        if fn == "depth":
            value, branch = fsgs_loss.depth_pearson_loss(x, m, return_branch=True)
        elif fn == "pseudo":
            value = fsgs_loss.pseudo_depth_pearson_loss(x, m)
        else:
            value = fsgs_loss.pearson_corrcoef(x.reshape(-1, 1), m.reshape(-1))
        if upstream is None:
            value.backward()
        else:
            value.backward(torch.tensor(upstream, device=dev))
        gx, gm = x.grad, m.grad
    if stream is not None:
        stream.synchronize()
    assert gx.shape == x.shape and (gm is None or gm.shape == m.shape)
    return (value.detach().cpu(), None if branch is None else branch.cpu(), gx.cpu(), None if gm is None else gm.cpu())


def _record(key, **kw):
    PARITY[key] = kw
    try:
        out = os.environ.get("FSGS_LOSS_PARITY_OUT") or os.path.join(ROOT, "profiles", "fsgs_loss_parity.json")
        json.dump(PARITY, open(out, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def check_values(tag, got, w):
    """(a): loss and every gradient the restatement has."""
    value, _, gx, gm = got
    loss_err = abs(float(value) - w["value"]) / max(1.0, abs(w["value"]))
    errs = dict(loss_err=loss_err)
    for name, g, g64 in (("grad_x_err", gx, w["gx"]), ("grad_m_err", gm, w["gm"])):
        if g64 is not None:
            assert bool(torch.isfinite(g).all())
            errs[name] = float((g.double() - g64).abs().max()) / float(g64.abs().max())
    print("%s: value %.9g (want %.9g) %s" % (tag, float(value), w["value"], " ".join("%s %.2e" % kv for kv in errs.items())))
    _record(tag, **errs)
    assert loss_err <= LOSS_BAR
    for name in ("grad_x_err", "grad_m_err"):
        assert errs.get(name, 0.0) <= GRAD_BAR, name


def test_sizes_come_from_the_kernels_constants(hip):
    """One 64-byte partial per workgroup, the scratch rounded up to 256 bytes: it grows with every fourth workgroup, and stops
    growing where the grid does."""
    size = hip.api.raw("pearson_tmp_bytes")
    assert size(GRID) == size(GRID + 1) == size(100 * GRID)
    assert size(GRID - 4 * BLOCK) < size(GRID - 4 * BLOCK + 1) == size(GRID)
    assert size(BLOCK) < size(4 * BLOCK + 1)


@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("size", AB_SIZES, ids=_sid)
def test_depth_loss_against_the_restatement(hip, size, kind):
    w = want("depth", size, kind)
    got = run_hip("depth", size, kind)
    assert got[1].dtype == torch.int32 and int(got[1]) == w["branch"] == ("A", "B").index(kind)   # (b)
    check_values("%s %s depth_pearson_loss" % (_sid(size), kind), got, w)                       # (a)
    again = run_hip("depth", size, kind)                                                         # (e)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and torch.equal(got[2], again[2])
    twice = run_hip("depth", size, kind, upstream=2.0)                                           # (f)
    assert torch.equal(twice[2], 2.0 * got[2])
    scaled = run_hip("depth", size, kind, upstream=0.3)
    assert float((scaled[2].double() - 0.3 * w["gx"]).abs().max()) <= GRAD_BAR * 0.3 * float(w["gx"].abs().max())


@pytest.mark.parametrize("fn", ["pearson", "pseudo"])
@pytest.mark.parametrize("kind", ["A", "B"])
@pytest.mark.parametrize("size", (65, BLOCK + 1, GRID + 1, (378, 504)), ids=_sid)
def test_single_form_functions_against_the_restatement(hip, size, kind, fn):
    got = run_hip(fn, size, kind)
    check_values("%s %s %s" % (_sid(size), kind, fn), got, want(fn, size, kind))
    again = run_hip(fn, size, kind)
    assert torch.equal(got[0], again[0]) and torch.equal(got[2], again[2]) and torch.equal(got[3], again[3])
    twice = run_hip(fn, size, kind, upstream=2.0)
    assert torch.equal(twice[2], 2.0 * got[2]) and torch.equal(twice[3], 2.0 * got[3])


@pytest.mark.parametrize("fn", ["depth", "pearson", "pseudo"])
@pytest.mark.parametrize("size", OTHER_SIZES, ids=_sid)
def test_offset_scene(hip, size, fn):
    """x = 1000 + 0.01 noise: raw fp32 moments would give NaN here (tests/test_fsgs_loss_cpu.py)."""
    check_values("%s offset %s" % (_sid(size), fn), run_hip(fn, size, "offset"), want(fn, size, "offset"))


@pytest.mark.parametrize("fn", ["depth", "pearson", "pseudo"])
@pytest.mark.parametrize("kind", ["exact+", "exact-"])
@pytest.mark.parametrize("size", (2,) + OTHER_SIZES, ids=_sid)
def test_exact_scenes(hip, size, kind, fn):
    w = want(fn, size, kind)
    value, _, gx, gm = run_hip(fn, size, kind)
    loss_err = abs(float(value) - w["value"]) / max(1.0, abs(w["value"]))
    print("%s %s %s: value %.9g (want %.9g)" % (_sid(size), kind, fn, float(value), w["value"]))
    assert loss_err <= LOSS_BAR
    if fn == "pseudo":
        assert abs(float(value) - (0.0 if kind == "exact+" else 2.0)) <= LOSS_BAR * 2.0
    if fn == "pearson":
        assert abs(float(value) - (-1.0 if kind == "exact+" else 1.0)) <= LOSS_BAR
    assert bool(torch.isfinite(gx).all()) and (gm is None or bool(torch.isfinite(gm).all()))
    if w["r_abs"] >= 1.0 - 1e-9:
        # (c): the true gradient is zero up to the rounding of the inputs
        worst = float(gx.abs().max())
        _record("%s %s %s" % (_sid(size), kind, fn), loss_err=loss_err, grad_x_max=worst, first_term=w["first"])
        assert worst <= GRAD_BAR * w["first"]
    else:
        # the depth loss took a form in which these inputs are not collinear (1 / (m + 200) against z): the ordinary bar
        assert fn == "depth"
        check_values("%s %s %s" % (_sid(size), kind, fn), (value, None, gx, gm), w)


@pytest.mark.parametrize("fn", ["depth", "pearson", "pseudo"])
@pytest.mark.parametrize("size", OTHER_SIZES, ids=_sid)
def test_constant_sequence_is_nan_with_a_zero_gradient(hip, size, fn):
    value, _, gx, gm = run_hip(fn, size, "constant")
    assert bool(torch.isnan(value))
    assert float(gx.abs().max()) == 0.0 and not bool(torch.isnan(gx).any())
    assert gm is None or (float(gm.abs().max()) == 0.0 and not bool(torch.isnan(gm).any()))


def test_pseudo_target_gradient_is_minus_the_id_form_gradient(hip):
    """(g)"""
    import fsgs_loss
    dev = torch.device("cuda:0")
    size = (378, 504)
    _, _, gx, gm = run_hip("pseudo", size, "A")
    w = want("pseudo", size, "A")
    assert gm is not None and float((gm.double() - w["gm"]).abs().max()) <= GRAD_BAR * float(w["gm"].abs().max())
    x64, m64 = inputs(size, "A")
    d = x64.float().to(dev).requires_grad_(True)
    m = m64.float().to(dev).requires_grad_(True)
    fsgs_loss.pearson_corrcoef(d.reshape(-1), (-m).reshape(-1)).backward()
    assert torch.equal(gm, -m.grad.cpu()) and torch.equal(gx, -d.grad.cpu())


def test_only_the_target_requires_grad_and_no_grad(hip):
    import fsgs_loss
    dev = torch.device("cuda:0")
    x64, m64 = inputs(65, "A")
    x = x64.float().to(dev)
    m = m64.float().to(dev).requires_grad_(True)
    r = fsgs_loss.pearson_corrcoef(x.reshape(-1), m.reshape(-1))
    r.backward()
    w = want("pearson", 65, "A")
    assert float((m.grad.cpu().double() - w["gm"]).abs().max()) <= GRAD_BAR * float(w["gm"].abs().max())
    with torch.no_grad():
        r2 = fsgs_loss.pearson_corrcoef(x.reshape(-1), m.reshape(-1))
    assert float(r2) == float(r) and not r2.requires_grad


def test_views_and_unaligned_storage(hip):
    """A [H,W] view that is not contiguous is made so; a tensor whose storage does not start on 16 bytes takes the scalar loads
    and gives the same bits (the element-to-lane assignment does not change)."""
    import fsgs_loss
    dev = torch.device("cuda:0")
    x64, m64 = inputs((378, 504), "B")
    x, m = x64.float().to(dev), m64.float().to(dev)
    outs = []
    for form in ("plain", "transposed", "offset"):
        if form == "plain":
            xa, ma = x.clone(), m
        elif form == "transposed":
            xa, ma = x.t().contiguous().t(), m.t().contiguous().t()
            assert not xa.is_contiguous()
        else:
            xa = torch.empty(x.numel() + 1, device=dev)[1:].view_as(x).copy_(x)
            ma = torch.empty(m.numel() + 1, device=dev)[1:].view_as(m).copy_(m)
            assert xa.data_ptr() % 16 != 0
        xa = xa.detach().requires_grad_(True)
        loss = fsgs_loss.depth_pearson_loss(xa, ma)
        loss.backward()
        outs.append((loss.detach().cpu(), xa.grad.cpu()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


def test_side_stream_without_a_synchronize(hip):
    """(i): nothing in the node waits for the host - forward and backward enqueued on a side stream complete, same bits."""
    base = run_hip("depth", (378, 504), "A")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = run_hip("depth", (378, 504), "A", stream=side)
    assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]) and torch.equal(base[2], got[2])


@pytest.mark.parametrize("extent", [0.02, 0.05, 0.1])
def test_proximity_on_the_gpu_equals_the_cpu_run(hip, oracle, extent):
    """(h): the kNN is bit-exact against the oracle's (tests/test_gpu_knn*.py), so any difference is the new code's."""
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import FIELDS, GaussianModelLite
    sc = synthetic.trained_like(400, seed=3, scale_mult=1.5)
    models = []
    for dev, api in ((torch.device("cpu"), oracle.api), (torch.device("cuda:0"), hip.api)):
        m = GaussianModelLite(sc, dev, api=api, spatial_order=False)
        g = torch.Generator().manual_seed(1)
        m.optimizer.exp_avg.copy_(torch.randn(m.optimizer.exp_avg.shape, generator=g).to(dev))
        m.optimizer.exp_avg_sq.copy_(torch.rand(m.optimizer.exp_avg_sq.shape, generator=g).to(dev))
        m.max_radii2D += 1.0
        models.append((m, m.proximity(extent)))
    (c, nc), (h, nh) = models
    assert nc == nh and c.P == h.P and (nc == 0) == (extent == 0.1)
    ov, hv = c.optimizer, h.optimizer
    for k, _ in FIELDS:
        assert torch.equal(c.params[k].detach(), h.params[k].detach().cpu()), k
        assert torch.equal(ov.field_views(ov.exp_avg)[k], hv.field_views(hv.exp_avg)[k].cpu()), k
        assert torch.equal(ov.field_views(ov.exp_avg_sq)[k], hv.field_views(hv.exp_avg_sq)[k].cpu()), k
    assert h.max_radii2D.is_cuda and not h.max_radii2D.any() and not h.denom.any() and not h.xyz_gradient_accum.any()
