"""tests/model_ops_reference.py proved on the CPU: its float64 restatement against torch's CPU autograd in float64 (tight) and in
float32 (within the bars), torch's answer at the clamp's tie asserted outright, the case table's own margins, and the oracle's
gso_activations_fwd / gso_activations_bwd held to the restatement at the bars on every case and every row count."""
import numpy as np
import pytest
import torch

import model_ops_reference as mr
from test_model_ops import run_api


def tensors(c, P):
    """the case's inputs as torch views into ONE copy of its flat buffer, and its cotangents"""
    t = {k: torch.from_numpy(v) for k, v in mr.views(c["flat"].copy(), P).items()}
    grads = tuple(torch.from_numpy(c[k].copy()) for k in ("g_scales", "g_rot", "g_opac"))
    return t, grads


def torch_autograd(c, P, dtype):
    t, grads = tensors(c, P)
    s, r, o = (t[k].to(dtype).clone().requires_grad_(True) for k in ("scaling", "rotation", "opacity"))
    out = (torch.exp(s), torch.nn.functional.normalize(r, eps=mr.EPS), torch.sigmoid(o))
    torch.autograd.backward(out, [g.to(dtype) for g in grads])
    vals = [x.detach() for x in out] + [s.grad, r.grad, o.grad]
    return dict(zip(("scales", "v", "opacity", "d_scaling", "d_rotation", "d_opacity"), (x.numpy() for x in vals)))


def api_outputs(api, c, P, device="cpu"):
    """activations_fwd / activations_bwd of `api` on views into one flat buffer on `device`"""
    t = mr.views(torch.from_numpy(c["flat"].copy()).to(device), P)
    grads = tuple(torch.from_numpy(c[k].copy()) for k in ("g_scales", "g_rot", "g_opac"))
    outs, d = run_api(api, t["scaling"], t["rotation"], t["opacity"], grads)
    vals = [outs[0], outs[1], outs[2], d[0], d[1], d[2]]
    return dict(zip(("scales", "v", "opacity", "d_scaling", "d_rotation", "d_opacity"), (x.cpu().numpy() for x in vals)))


def test_the_case_table_holds_its_margins():
    mr._check_table()
    kinds = set()
    for P in mr.SIZES:
        c = mr.cases(P)
        kinds |= set(c["kind"])
        v = mr.views(c["flat"], P)
        base = c["flat"].__array_interface__["data"][0]
        assert v["rotation"].__array_interface__["data"][0] - base == 220 * P
        assert np.shares_memory(v["scaling"], c["flat"]) and not c["flat"].flags.writeable
        # the reference's branch is the table's
        want = np.isin(c["kind"], ("tie", "above", "projected"))
        assert np.array_equal(c["ref"]["projected"], want)
    assert kinds == {"tie", "below", "above", "clamped", "projected"}
    c = mr.cases(1023)
    t = mr.views(c["flat"], 1023)
    # every rotation row met every cotangent kind; inf and NaN are among the references, and values below FLT_MIN
    for r in range(len(mr.ROTATIONS)):
        rows = np.arange(1023) % len(mr.ROTATIONS) == r
        g = c["g_rot"][rows, 0]
        assert (g == 0).any() and (np.abs(g) == np.float32(1e30)).any() and (np.abs(g) == np.float32(1e-30)).any()
    with np.errstate(over="ignore"):
        assert np.isinf(c["ref"]["scales"].astype(np.float32)).any() and np.isnan(c["ref"]["opacity"]).any()
        assert np.isinf(c["ref"]["d_rotation"].astype(np.float32)).any()
    assert ((c["ref"]["scales"] < mr.FLT_MIN) & (c["ref"]["scales"] > 0)).any()
    assert np.isinf(t["opacity"]).sum() >= 2 and np.signbit(c["g_rot"][c["g_rot"] == 0]).any()


@pytest.mark.parametrize("P", mr.SIZES)
def test_the_restatement_is_torch_autograd_in_float64(P):
    """1e-14 relative.  d_rotation: relative to the absolute contributions |g_k| + |v_k| sum |v_j g_j| over |q| (the difference
    cancels); d_opacity: torch's own 1 - s cancels in float64 too, |g| 2^-52 on top."""
    c = mr.cases(P)
    got, ref, bar = torch_autograd(c, P, torch.float64), c["ref"], c["bar"]
    g_o = np.abs(c["g_opac"].astype(np.float64))
    for k in mr.OUTPUTS:
        a, b = got[k], ref[k]
        if k == "d_scaling":    # (in float64 the result of exp does not overflow: no g * inf here)
            b = c["g_scales"].astype(np.float64) * ref["scales"]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), k
        fin = np.isfinite(b)
        tol = 1e-14 * np.abs(b)
        if k == "d_rotation":
            tol = np.where(ref["projected"][:, None], 1e-14 * bar[k] / (24 * mr.U), tol)
        if k == "d_opacity":
            tol = tol + g_o * 2.0 ** -52
        assert np.all(np.abs(a[fin] - b[fin]) <= tol[fin]), (k, float(np.abs(a[fin] - b[fin]).max()))


@pytest.mark.parametrize("P", mr.SIZES)
def test_torch_autograd_in_float32_is_within_the_bars(P):
    """Every output at the bars, with one exemption that is torch's and not the kernels': where a row's rotation gradient
    overflows fp32 (cotangent 1e30 over a norm near eps32), torch's composition (g / n - q (q.g) / n^3, term by term) forms
    inf - inf = NaN; those rows of d_rotation are left out here.  The oracle and the HIP kernels are held on them: they form
    the finite difference first and overflow to the reference's inf.  On the clamped branch torch adds the clamp's zero
    gradient to g / eps32, which turns a -0 into +0: equal as numbers here, bit for bit for the oracle and the kernels."""
    c = mr.cases(P)
    got = torch_autograd(c, P, torch.float32)
    with np.errstate(over="ignore"):
        ref32 = c["ref"]["d_rotation"].astype(np.float32)
    over = np.isinf(ref32).any(1)
    assert np.all(np.abs(c["g_rot"][over]) == np.float32(1e30))
    got["d_rotation"] = np.where(over[:, None], ref32, got["d_rotation"])
    worst = mr.check_all(got, c, "torch fp32 ", bits=False)
    print("P = %d, torch fp32, largest distance / bar: %s" % (P, {k: round(v, 3) for k, v in worst.items()}))


def tie_example():
    q = np.zeros((1, 4), np.float32)
    q[0, 0] = mr.EPS32
    return q, np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)


def test_torch_projects_at_the_tie():
    """|q| == eps32: clamp_min passes the gradient (norm >= eps), so the gradient is the PROJECTED one - its component along q is
    exactly 0 - and not g / eps32."""
    q, g = tie_example()
    r = torch.from_numpy(q).clone().requires_grad_(True)
    torch.nn.functional.normalize(r).backward(torch.from_numpy(g))
    d = r.grad.numpy()[0]
    assert float(torch.from_numpy(q).norm()) == float(mr.EPS32)
    assert d[0] == 0.0
    want = g[0].astype(np.float64) / mr.EPS
    assert np.all(np.abs(d[1:] - want[1:]) <= 2 * mr.U * want[1:])
    ref = mr.restate(np.zeros((1, 3)), q, np.zeros((1, 1)), np.zeros((1, 3)), g, np.zeros((1, 1)))
    assert bool(ref["projected"][0]) and ref["d_rotation"][0, 0] == 0.0
    # every tie of the table, in float32: the component along q is within its bar of 0, far from g / eps32
    c = mr.cases(1023)
    got = torch_autograd(c, 1023, torch.float32)["d_rotation"]
    ties = c["kind"] == "tie"
    along = mr.views(c["flat"], 1023)["rotation"][ties] != 0
    clamped_answer = np.abs(c["g_rot"][ties][along].astype(np.float64)) / mr.EPS
    with np.errstate(over="ignore"):
        fin = np.isfinite(clamped_answer.astype(np.float32))      # (cotangent 1e30: the row overflows, see above)
    assert np.all(np.abs(got[ties][along][fin]) <= np.maximum(c["bar"]["d_rotation"][ties][along][fin], mr.FLT_MIN))
    big = fin & (clamped_answer > 1.0)
    assert big.sum() > 20 and np.all(np.abs(got[ties][along][big]) < 1e-3 * clamped_answer[big])


def test_the_oracle_projects_at_the_tie(oracle):
    q, g = tie_example()
    z3, z1 = torch.zeros((1, 3)), torch.zeros((1, 1))
    _, d = run_api(oracle.api, z3, torch.from_numpy(q), z1, (z3, torch.from_numpy(g), z1))
    d = d[1].numpy()[0]
    print("oracle at q = (eps32, 0, 0, 0), g = (1, 2, 3, 4):", d)
    # (q inv)^2 is within 4 u of 1: what is left along q is within the bar's 48 u g / eps32 of 0; g / eps32 itself is 1e12
    assert abs(float(d[0])) <= 48 * mr.U * 1.0 / mr.EPS
    assert np.all(np.abs(d[1:] - g[0, 1:] / mr.EPS) <= 2 * mr.U * g[0, 1:] / mr.EPS)


@pytest.mark.parametrize("P", mr.SIZES)
def test_the_oracle_is_within_the_bars_of_the_restatement(oracle, P):
    c = mr.cases(P)
    worst = mr.check_all(api_outputs(oracle.api, c, P), c, "oracle ")
    print("P = %d, oracle, largest distance / bar: %s" % (P, {k: round(v, 3) for k, v in worst.items()}))
