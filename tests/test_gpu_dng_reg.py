"""DNGaussian's per-Gaussian regulariser, view directions and near-camera mask (csrc/gs_dng_reg.hip through the dng_reg
package) on the MI355X, against the float64 restatement (tests/dng_reg_reference.py) evaluated on the same fp32 inputs.

Bars, derived and not tuned:
(a) activated regulariser: every term and the total within 1e-6 relative of the float64 result - each element's ratio or square
    is one fp32 rounding (2^-24 relative; (1 - o)^2 two), the sums are float64, the final rounding adds 2^-24; every gradient
    element within 1e-6 x that element's scale (the sum of the absolute contributions added into it: the kernel evaluates them
    in float64 and rounds once); a structurally zero element (scale 0: a column that is neither max nor min, o == 0.2) is
    exactly 0; NaN where, and only where, the restatement has it.
(b) raw regulariser: the device's exp and sigmoid come on top.  Their accuracy is not documented in the installed ROCm tree, so
    it was measured: tests/tools/dng_reg_act_probe.hip, the kernel's own activation functions against float64 over
    scaling [-7, 1.5] and opacity [-7, 7] (4 194 304 arguments each; the scenes here stay inside).  The largest relative error
    of exp, sigmoid and 1 - sigmoid is ACT_ERR_MEASURED; ACT_ERR = 2 x that (the margin).  A term multiplies at most two
    activated values, a gradient contribution at most three, so the bars are 1e-6 + 2 ACT_ERR relative for the terms and
    (1e-6 + 3 ACT_ERR) x scale for the gradients: the factors RAW_TERM_FACTOR = 1.73 and RAW_GRAD_FACTOR = 2.09 on (a)'s
    1e-6 below (ACT_ERR_MEASURED = 1.8161e-07, ACT_ERR = 3.6322e-07).
    Membership in H / L cannot differ: the raw scenes keep sigmoid 1.5e-3 away from 0.2 (tests/test_dng_reg_cpu.py).
(c) view directions: forward within 1e-6 absolute, backward within 1e-6 x scale; a row at the camera centre is NaN, alone.
(d) near mask: equal to the restatement, after asserting in float64 that no distance lies within 1e-5 relative of `near`.
(e) two calls give the same bits, forward and backward; an unaligned base (the element-by-element loads) gives the aligned
    run's bits; [P,1] and [P] opacities the same bits.
(f) forward and backward enqueued on a side stream without a synchronize complete with the default stream's bits: nothing in
    the nodes waits for the host (the way tests/test_gpu_fsgs_loss.py establishes it).
Sizes: 1, 2, a wave +- 1, what one workgroup sweeps +- 1, and three sweeps + 7 rows on a grid capped at 2 workgroups (the
grid-stride loop and several partials).  Every restatement result is computed once and shared.
Largest distances on one MI355X run: terms 5.0e-08 (raw 8.5e-08), gradients 9.8e-08 (raw 3.0e-07) of the scale, directions
3.0e-08 forward and 5.7e-08 of the scale backward."""
import pytest
import torch

import dng_reg_reference as ref
from gsplat_amd import dng_reg as _k

pytestmark = pytest.mark.gpu

F64 = torch.float64
TOL = 1e-6
ACT_ERR_MEASURED = 1.8161e-07   # sigmoid and 1 - sigmoid: 3.05 x 2^-24; exp: 8.38e-08 = 1.41 x 2^-24 (one MI355X run of the probe)
ACT_ERR = 2.0 * ACT_ERR_MEASURED
RAW_TERM_FACTOR = 1.0 + 2.0 * ACT_ERR / TOL
RAW_GRAD_FACTOR = 1.0 + 3.0 * ACT_ERR / TOL
CHUNK = _k.BLOCK_ROWS
STRIDED = 3 * CHUNK + 7
SIZES = (1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, STRIDED)
NEAR = 0.5
_scenes, _closed, _points = {}, {}, {}


def _max_blocks(P):
    return 2 if P == STRIDED else 0


def scene(P, kind, raw):
    key = (P, kind, raw)
    if key not in _scenes:
        if kind == "tied":
            s, o = ref.scene(P, "mixed", seed=9, raw=raw)
            s = s[:, :1].expand(P, 3).clone()
        else:
            s, o = ref.scene(P, kind, seed=9, raw=raw)
        _scenes[key] = (s, o)
    return _scenes[key]


def closed(P, kind, raw, g_terms, g_total):
    key = (P, kind, raw, g_terms, g_total)
    if key not in _closed:
        s, o = scene(P, kind, raw)
        w = ref.regulariser_closed(s, o, ref.coefficients(g_terms, g_total), raw=raw)
        w["total"] = ref.total(w["terms"])
        _closed[key] = w
    return _closed[key]


def points(P, K):
    if (P, K) not in _points:
        _points[(P, K)] = ref.points(P, K, near=NEAR, seed=11)
    return _points[(P, K)]


def _place(t64, dev, offset):
    """The fp32 tensor on the device; offset: its storage starts 4 bytes off a 16-byte boundary."""
    t = t64.float()
    if not offset:
        return t.to(dev)
    out = torch.empty(t.numel() + 1, device=dev)[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def run_reg(P, kind, raw, g_terms=None, g_total=1.0, offset=False, column=True, need=(True, True), stream=None):
    """-> dict(terms, total, g_scaling, g_opacity) on the CPU; a gradient that was not asked for is None."""
    dev = torch.device("cuda:0")
    s64, o64 = scene(P, kind, raw)
    fn = _k.gaussian_regulariser_raw if raw else _k.gaussian_regulariser
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        s = _place(s64, dev, offset).requires_grad_(need[0])
        o = _place(o64.reshape(P, 1) if column else o64, dev, offset).requires_grad_(need[1])
        total, terms = fn(s, o, *ref.WEIGHTS, return_terms=True, max_blocks=_max_blocks(P))
        assert total.shape == () and terms.shape == (3,)
        if g_terms is None:
            total.backward(torch.tensor(g_total, device=dev))
        elif g_total is None and sum(1 for v in g_terms if v) == 1:
            k = [i for i, v in enumerate(g_terms) if v][0]
            terms[k].backward(torch.tensor(g_terms[k], device=dev))
        else:
            ((terms * torch.tensor(g_terms, device=dev)).sum() + g_total * total).backward()
        gs, go = s.grad, o.grad
    if stream is not None:
        stream.synchronize()
    assert gs is None or gs.shape == s.shape
    assert go is None or go.shape == o.shape
    return dict(terms=terms.detach().cpu(), total=total.detach().cpu(), g_scaling=None if gs is None else gs.cpu(),
                g_opacity=None if go is None else go.cpu().reshape(-1))


def check_reg(tag, got, w, raw):
    term_tol = TOL * (RAW_TERM_FACTOR if raw else 1.0)
    grad_tol = TOL * (RAW_GRAD_FACTOR if raw else 1.0)
    values = torch.cat((got["terms"].to(F64), got["total"].to(F64).reshape(1)))
    wants = torch.cat((w["terms"], w["total"].reshape(1)))
    assert torch.isnan(values).tolist() == torch.isnan(wants).tolist(), (tag, values, wants)
    ok = ~torch.isnan(wants)
    rel = ((values[ok] - wants[ok]).abs() / wants[ok].abs())
    worst = {"value": float(rel.max())}
    for name in ("g_scaling", "g_opacity"):
        g = got[name]
        if g is None:
            continue
        want, scale = w[name].reshape(g.shape), w[name + "_scale"].reshape(g.shape)
        assert bool(torch.isfinite(g).all()), (tag, name)
        zero = scale == 0
        assert not bool(g[zero].any()), (tag, name, "a structurally zero element is not 0")
        err = (g.to(F64) - want).abs()[~zero] / scale[~zero]
        worst[name] = float(err.max()) if err.numel() else 0.0
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["value"] <= term_tol, (tag, worst)
    assert worst.get("g_scaling", 0.0) <= grad_tol and worst.get("g_opacity", 0.0) <= grad_tol, (tag, worst)


def _same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) or
               (k in ("terms", "total") and torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and
                torch.equal(a[k].nan_to_num(7.0), b[k].nan_to_num(7.0))) for k in a)


# ---- regulariser ----
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", SIZES)
def test_regulariser_against_the_restatement(hip, P, raw):
    """A gradient on the total only (what a training step sends), every size; ties, every max / min column, o on both
    sides of 0.2 and exactly 0.2 are in the scene (P = 1: one of the sets is empty, so opa and total are NaN there, as in the restatement)."""
    s64, o64 = scene(P, "mixed", raw)
    if P >= 8 and not raw:
        assert bool((o64 == ref.THRESHOLD).any())
    w = closed(P, "mixed", raw, None, 1.0)
    got = run_reg(P, "mixed", raw)
    check_reg("P=%d %s total" % (P, "raw" if raw else "activated"), got, w, raw)             # (a), (b)
    assert _same(got, run_reg(P, "mixed", raw))                                                # (e)
    assert _same(got, run_reg(P, "mixed", raw, offset=True))
    assert _same(got, run_reg(P, "mixed", raw, column=False))
    assert _same(got, run_reg(P, "mixed", raw, offset=True, column=False))


def test_the_capped_grid_strides_and_changes_only_the_order_of_the_sums(hip):
    s64, o64 = scene(STRIDED, "mixed", False)
    dev = torch.device("cuda:0")
    outs = []
    for mb in (2, 0, 1):
        total, terms = _k.gaussian_regulariser(s64.float().to(dev), o64.float().to(dev), return_terms=True, max_blocks=mb)
        outs.append(torch.cat((terms, total.reshape(1))).cpu().to(F64))
    w = closed(STRIDED, "mixed", False, None, 1.0)
    want = torch.cat((w["terms"], w["total"].reshape(1)))
    for o in outs:
        assert float(((o - want).abs() / want.abs()).max()) <= TOL


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("g_terms,g_total", [((1.0, 0.0, 0.0), None), ((0.0, 1.0, 0.0), None), ((0.0, 0.0, 1.0), None),
                                             ((0.3, -2.0, 0.7), 1.5), (None, -0.25)],
                         ids=["shape", "scale", "opa", "terms+total", "total"])
@pytest.mark.parametrize("P", [65, CHUNK + 1])
def test_gradient_arriving_on_single_terms_and_on_both(hip, P, g_terms, g_total, raw):
    got = run_reg(P, "mixed", raw, g_terms=g_terms, g_total=g_total)
    check_reg("P=%d raw=%d g=%s/%s" % (P, raw, g_terms, g_total), got, closed(P, "mixed", raw, g_terms, g_total), raw)
    if g_terms is not None and g_total is None:
        other = got["g_opacity"] if g_terms[2] == 0.0 else got["g_scaling"]
        assert not bool(other.any())   # a term the gradient does not reach leaves exact zeros


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", [1, 65, CHUNK + 1])
def test_all_rows_tied(hip, P, raw):
    """Three equal scales per row, the state training starts in: max and min are column 0, the other two columns get 0."""
    got = run_reg(P, "tied", raw)
    check_reg("P=%d raw=%d tied" % (P, raw), got, closed(P, "tied", raw, None, 1.0), raw)
    assert float(got["terms"][0]) == 1.0 and not bool(got["g_scaling"][:, 1:].any())


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("kind", ["H_empty", "L_empty"])
@pytest.mark.parametrize("P", [1, 65, CHUNK + 1])
def test_an_empty_set_is_nan_with_finite_gradients(hip, P, kind, raw):
    got = run_reg(P, kind, raw)
    assert torch.isnan(got["terms"]).tolist() == [False, False, True] and bool(torch.isnan(got["total"]))
    assert bool((got["g_opacity"] != 0).all())
    check_reg("P=%d raw=%d %s" % (P, raw, kind), got, closed(P, kind, raw, None, 1.0), raw)


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("need", [(True, False), (False, True)], ids=["scaling-only", "opacity-only"])
def test_one_input_not_requiring_grad(hip, need, raw):
    P = CHUNK + 1
    both = run_reg(P, "mixed", raw)
    got = run_reg(P, "mixed", raw, need=need)
    for name, asked in zip(("g_scaling", "g_opacity"), need):
        assert (got[name] is not None) == asked
        if asked:
            assert torch.equal(got[name], both[name])
    assert torch.equal(got["terms"], both["terms"])


def test_no_grad_and_the_package_call(hip):
    import dng_reg
    dev = torch.device("cuda:0")
    s64, o64 = scene(65, "mixed", False)
    s, o = s64.float().to(dev).requires_grad_(True), o64.float().reshape(-1, 1).to(dev).requires_grad_(True)
    total = dng_reg.gaussian_regulariser(s, o)
    with torch.no_grad():
        again = dng_reg.gaussian_regulariser(s, o)
    assert total.requires_grad and not again.requires_grad and torch.equal(total.detach(), again)
    w = closed(65, "mixed", False, None, 1.0)
    assert abs(float(total.detach()) - float(w["total"])) <= TOL * abs(float(w["total"]))
    rs64, ro64 = scene(65, "mixed", True)
    raw_total, raw_terms = dng_reg.gaussian_regulariser_raw(rs64.float().to(dev), ro64.float().to(dev), return_terms=True)
    wr = closed(65, "mixed", True, None, 1.0)
    assert abs(float(raw_total) - float(wr["total"])) <= TOL * RAW_TERM_FACTOR * abs(float(wr["total"]))
    assert raw_terms.shape == (3,)


def test_side_stream_without_a_synchronize(hip):
    """(f)"""
    base = run_reg(CHUNK + 1, "mixed", True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert _same(base, run_reg(CHUNK + 1, "mixed", True, stream=side))


# ---- view directions ----
def run_dirs(P, offset=False, centre_row=None, need=True):
    import dng_reg
    dev = torch.device("cuda:0")
    xyz64, _, campos64 = points(P, 2)
    xyz64 = xyz64.clone()
    if centre_row is not None:
        xyz64[centre_row] = campos64
    g64 = torch.randn((P, 3), generator=torch.Generator().manual_seed(P), dtype=F64).float().to(F64)
    x = _place(xyz64, dev, offset).requires_grad_(need)
    c = campos64.float().to(dev)
    out = dng_reg.view_dirs(x, c)
    assert out.shape == (P, 3) and out.requires_grad == need
    if need:
        out.backward(_place(g64, dev, offset))
    return out.detach().cpu(), None if x.grad is None else x.grad.cpu(), ref.view_dirs_closed(xyz64, campos64, g64)


@pytest.mark.parametrize("P", SIZES)
def test_view_dirs_against_the_restatement(hip, P):
    out, gx, w = run_dirs(P)
    fwd = float((out.to(F64) - w["out"]).abs().max())
    bwd = float(((gx.to(F64) - w["g_xyz"]).abs() / w["g_xyz_scale"]).max())
    print("view_dirs P=%d: forward %.2e absolute, backward %.2e of the scale" % (P, fwd, bwd))
    assert fwd <= TOL and bwd <= TOL                                                          # (c)
    again = run_dirs(P)
    assert torch.equal(out, again[0]) and torch.equal(gx, again[1])                           # (e)
    off = run_dirs(P, offset=True)
    assert torch.equal(out, off[0]) and torch.equal(gx, off[1])
    assert run_dirs(P, need=False)[1] is None


@pytest.mark.parametrize("P,row", [(1, 0), (65, 64), (CHUNK + 1, 5)])
def test_view_dirs_at_the_camera_centre_is_nan_in_that_row_only(hip, P, row):
    out, gx, w = run_dirs(P, centre_row=row)
    want = [i == row for i in range(P)]
    assert torch.isnan(out).all(dim=1).tolist() == want == torch.isnan(out).any(dim=1).tolist()
    assert torch.isnan(w["out"]).all(dim=1).tolist() == want
    assert torch.isnan(gx).any(dim=1).tolist() == want == torch.isnan(w["g_xyz"]).any(dim=1).tolist()
    keep = [i for i in range(P) if i != row]
    if keep:
        assert float((out[keep].to(F64) - w["out"][keep]).abs().max()) <= TOL


# ---- near-camera mask ----
@pytest.mark.parametrize("K", [1, 2, 120, 256, 257, 600])
@pytest.mark.parametrize("P", [1, 2, 65, CHUNK - 1, CHUNK + 1, STRIDED])
def test_near_mask_equals_the_restatement(hip, P, K):
    """K = 256 / 257 / 600: one full tile of centres in LDS, one more centre, three tiles."""
    import dng_reg
    dev = torch.device("cuda:0")
    xyz64, centers64, _ = points(P, K)
    want, gap = ref.near_mask(xyz64, centers64, NEAR)
    assert gap >= 1e-5, "a distance within 1e-5 relative of `near`: the fp32 norm may fall on either side"   # (d)
    assert bool(want[-1]) and (P == 1 or not bool(want[0]))
    if K > 1:
        assert not bool(ref.near_mask(xyz64[-1:], centers64[:-1], NEAR)[0][0])   # the last row: the last camera alone
    outs = []
    for offset in (False, True):
        m = dng_reg.near_camera_mask(_place(xyz64, dev, offset), _place(centers64, dev, offset), NEAR)
        assert m.dtype == torch.bool and m.shape == (P,) and not m.requires_grad
        outs.append(m.cpu())
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want)
    if P >= 65 and K >= 2:
        assert 1 < int(want.sum()) < P
