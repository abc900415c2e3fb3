"""DNGaussian's grid / SH encoders on the GPU (csrc/gs_encoding.hip) on the constructed cases of tests/encoding_cases.py
(what each case is for: tests/test_encoding_cases_cpu.py), against the float64 oracle of tests/encoding_reference.py:

* exact cases (every path of the segmented embedding reduction, named in the test id): outputs, embedding gradient and
  input gradient are the oracle's bits, twice;
* form cases (all sixteen (D, C) instantiations, decision-edge rows, degenerate calls): every output element and every
  embedding slot inside its derived bar, the input gradient inside the bar measured on the fp32 restatement, outside rows
  and untouched slots exactly zero.  No element is exempt;
* the raw ABI: 1, 2, 3 and 4 sort passes, gradient-only calls, scratch of exactly gs_grid_encode_tmp_bytes behind a guard,
  the return codes of a short scratch and of unsupported L / D;
* SH: per output column (l, m) and per input component, at the poles, the axes, the zero vector and B off the 256 grid.
The measured bars and distances go to profiles/encoding_parity.json (or to the file ENCODING_PARITY_OUT names)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import encoding_cases as ec
import gridencoder
import shencoder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = {}
GS_E_SCRATCH, GS_E_UNSUPPORTED = -3, -5
GUARD = 4096


def _record(key, **kw):
    PARITY[key] = kw
    try:
        out = os.environ.get("ENCODING_PARITY_OUT") or os.path.join(ROOT, "profiles", "encoding_parity.json")
        json.dump(PARITY, open(out, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.fixture(scope="module")
def api():
    assert torch.cuda.is_available(), "GPU test running without a GPU"
    from gsplat_amd._lib import hip_api
    return hip_api()


def run_hip(t):
    """The autograd function, forward + backward -> host (outputs, embedding gradient, input gradient)."""
    xi = t.x.to(DEV).requires_grad_(True)
    emb = t.emb.to(DEV).requires_grad_(True)
    offs = torch.tensor(t.offsets, dtype=torch.int32, device=DEV)
    y = gridencoder.grid_encode(xi, emb, offs, t.pls, t.H, True, t.gridtype, t.align, t.interp)
    y.backward(t.g.to(DEV))
    return y.detach().cpu(), emb.grad.cpu(), xi.grad.cpu()


def _ratio(d, bar):
    ok = bar > 0
    return float((d[ok] / bar[ok]).max()) if bool(ok.any()) else 0.0


def check_bars(key, h, e):
    """h: host (outputs, embedding gradient, input gradient) of the GPU; e: encoding_cases.Expect."""
    d_out = (h[0].double() - e.out).abs()
    d_emb = (h[1].double() - e.gemb).abs()
    d_in = float((h[2].double() - e.gin).abs().max()) if e.gin.numel() else 0.0
    top = float(e.gin.abs().max()) if e.gin.numel() else 0.0
    _record(key, out_worst_over_bar=_ratio(d_out, e.bar_out), emb_worst_over_bar=_ratio(d_emb, e.bar_emb),
            out_max_dist=float(d_out.max()) if d_out.numel() else 0.0, emb_max_dist=float(d_emb.max()),
            in_dist=d_in, in_bar=e.bar_in, in_largest=top)
    print("%s: out %.3f of bar, emb %.3f of bar, in %.3e (bar %.3e, largest %.3e)"
          % (key, _ratio(d_out, e.bar_out), _ratio(d_emb, e.bar_emb), d_in, e.bar_in, top))
    assert e.bar_in <= 1e-4 * top
    assert bool((d_out <= e.bar_out).all()), "outputs: %d elements over their bar" % int((d_out > e.bar_out).sum())
    assert bool((d_emb <= e.bar_emb).all()), "embedding gradient: %d slots over their bar" % int((d_emb > e.bar_emb).sum())
    assert d_in <= e.bar_in, "input gradient %.3e over %.3e" % (d_in, e.bar_in)
    # outside rows and the slots nothing landed on: exactly zero
    assert bool((h[0][~e.inside] == 0).all()) and bool((h[2][~e.inside] == 0).all())
    assert bool((h[1][e.n_s == 0] == 0).all())


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("name", list(ec.EXACT), ids=[ec.exact_id(n) for n in ec.EXACT])
def test_exact_case(name):
    t, _, (out, gemb, gin) = ec.exact_expectation(name)
    a = run_hip(t)
    b = run_hip(t)
    for what, got, again, want in zip(("outputs", "embedding gradient", "input gradient"), a, b, (out, gemb, gin)):
        bad = int((got != want.float()).sum())
        assert torch.equal(got, want.float()), "%s: %d entries differ from the oracle's bits" % (what, bad)
        assert torch.equal(got, again), "%s differs between two runs" % what


# ---------------------------------------------------------------- form cases
@pytest.mark.parametrize("name", list(ec.FORM))
def test_form_case(name):
    e = ec.form_expectation(name)
    h = run_hip(e.t)
    check_bars("form/" + name, h, e)
    if ec.FORM[name].kind == "edges":
        # the inside / outside decision, row by row (an inside row's oracle output is non-zero)
        assert torch.equal((h[0] != 0).any(dim=1), e.inside)
    if ec.FORM[name].kind == "outside":
        assert not bool(h[0].any()) and not bool(h[1].any()) and not bool(h[2].any())


def test_empty_batch():
    t = ec.form_tensors(ec.FORM["D3C2-hash-smooth-noac"])
    t = t._replace(x=t.x[:0], g=t.g[:0])
    xi = t.x.to(DEV).requires_grad_(True)
    emb = t.emb.to(DEV).requires_grad_(True)
    offs = torch.tensor(t.offsets, dtype=torch.int32, device=DEV)
    y = gridencoder.grid_encode(xi, emb, offs, t.pls, t.H, True, t.gridtype, t.align, t.interp)
    assert y.shape == (0, t.L * t.C)
    y.backward(t.g.to(DEV))
    assert emb.grad.shape == t.emb.shape and not bool(emb.grad.any())
    assert xi.grad is None or xi.grad.shape == (0, t.D)


# ---------------------------------------------------------------- the raw ABI
class Raw:
    """gs_grid_encode_fwd / _bwd called directly: arbitrary int32 offsets, chosen outputs, chosen scratch."""

    def __init__(self, api, t):
        self.api, self.t = api, t
        self.x, self.emb, self.g = t.x.to(DEV).contiguous(), t.emb.to(DEV).contiguous(), t.g.to(DEV).contiguous()
        self.offs = torch.tensor(t.offsets, dtype=torch.int32, device=DEV)
        self.B, self.n_slots = t.x.shape[0], int(t.offsets[-1])
        self.S = float(np.log2(t.pls))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.nbytes = int(api.raw("grid_encode_tmp_bytes")(self.B, t.D, t.L, t.C, self.n_slots))

    def fwd(self, L=None, D=None, offs=None):
        t = self.t
        out = torch.full((self.B, t.L * t.C), float("nan"), device=DEV)
        dy = torch.full((self.B, t.L * t.D * t.C), float("nan"), device=DEV)
        rc = self.api.raw("grid_encode_fwd")(self.x.data_ptr(), self.B, D or t.D, self.emb.data_ptr(), self.n_slots, t.C,
                                             (self.offs if offs is None else offs).data_ptr(), L or t.L, self.S, t.H,
                                             t.gridtype, int(t.align), t.interp, out.data_ptr(), dy.data_ptr(), self.stream)
        torch.cuda.synchronize()
        return rc, out, dy

    def bwd(self, dy, want_emb=True, want_in=True, tmp=None, tmp_bytes=None, L=None, D=None, offs=None):
        t = self.t
        gemb = torch.full((self.n_slots, t.C), float("nan"), device=DEV) if want_emb else None
        gin = torch.full((self.B, t.D), float("nan"), device=DEV) if want_in else None
        if tmp is None:
            tmp = torch.empty((2 * self.nbytes + 65536,), dtype=torch.uint8, device=DEV)
        rc = self.api.raw("grid_encode_bwd")(self.g.data_ptr(), self.x.data_ptr(), self.B, D or t.D, self.n_slots, t.C,
                                             (self.offs if offs is None else offs).data_ptr(), L or t.L, self.S, t.H,
                                             t.gridtype, int(t.align), t.interp, dy.data_ptr() if want_in else None,
                                             gemb.data_ptr() if want_emb else None, gin.data_ptr() if want_in else None,
                                             tmp.data_ptr(), tmp.numel() if tmp_bytes is None else tmp_bytes, self.stream)
        torch.cuda.synchronize()
        return rc, gemb, gin


@pytest.mark.parametrize("name", [n for n in ec.PASSES if not n.startswith("passes4")])
def test_sort_pass_count(api, name):
    case = ec.PASSES[name]
    assert ec.sort_passes(case.offsets[-1]) == case.passes
    e = ec.expect(ec.pass_tensors(case))
    raw = Raw(api, e.t)
    rc, out, dy = raw.fwd()
    assert rc == 0
    rc, gemb, gin = raw.bwd(dy)
    assert rc == 0
    check_bars("abi/" + name, (out.cpu(), gemb.cpu(), gin.cpu()), e)


@pytest.mark.parametrize("name", [n for n in ec.PASSES if n.startswith("passes4")])
def test_sort_pass_count_sparse(api, name):
    """n_slots = 17 * 2^20 > 2^24: the expectation is sparse, every slot nothing landed on is exactly zero."""
    assert ec.sort_passes(ec.PASSES[name].offsets[-1]) == 4
    s = ec.sparse_expectation(name)
    raw = Raw(api, s.t)
    rc, out, dy = raw.fwd()
    assert rc == 0
    rc, gemb, _ = raw.bwd(dy, want_in=False)
    assert rc == 0
    slots = s.slots.to(DEV)
    d_out = (out.cpu().double() - s.out).abs()
    d_emb = (gemb[slots].cpu().double() - s.gemb).abs()
    _record("abi/" + name, out_worst_over_bar=_ratio(d_out, s.bar_out), emb_worst_over_bar=_ratio(d_emb, s.bar_emb),
            out_max_dist=float(d_out.max()), emb_max_dist=float(d_emb.max()), touched_slots=int(slots.numel()))
    assert bool((d_out <= s.bar_out).all()) and bool((d_emb <= s.bar_emb).all())
    untouched = torch.ones((raw.n_slots,), dtype=torch.bool, device=DEV)
    untouched[slots] = False
    assert int(untouched.sum()) == raw.n_slots - slots.numel()
    assert int(torch.count_nonzero(gemb[untouched])) == 0 and not bool(torch.isnan(gemb).any())


RAW_CASES = ("D3C2-hash-smooth-noac", "D5C8-tiled-linear-ac", "D2C1-tiled-linear-ac")


@pytest.mark.parametrize("name", RAW_CASES)
def test_gradient_only_calls_give_the_combined_call_bits(api, name):
    raw = Raw(api, ec.form_tensors(ec.FORM[name]))
    rc, _, dy = raw.fwd()
    assert rc == 0
    rc, gemb, gin = raw.bwd(dy)
    assert rc == 0 and not bool(torch.isnan(gemb).any()) and not bool(torch.isnan(gin).any())
    rc, gemb_only, none = raw.bwd(dy, want_in=False)          # dy_dx = NULL
    assert rc == 0 and none is None and torch.equal(gemb_only, gemb)
    rc, none, gin_only = raw.bwd(dy, want_emb=False, tmp=torch.empty((0,), dtype=torch.uint8, device=DEV), tmp_bytes=0)
    assert rc == 0 and none is None and torch.equal(gin_only, gin)          # tmp = NULL


@pytest.mark.parametrize("name", RAW_CASES + ("g700-C2-sentinel",))
def test_scratch_of_exactly_tmp_bytes(api, name):
    t = ec.exact_tensors(ec.EXACT[name]) if name in ec.EXACT else ec.form_tensors(ec.FORM[name])
    raw = Raw(api, t)
    rc, _, dy = raw.fwd()
    assert rc == 0
    rc, gemb, _ = raw.bwd(dy, want_in=False)
    assert rc == 0
    tmp = torch.empty((raw.nbytes + GUARD,), dtype=torch.uint8, device=DEV)
    tmp.fill_(0xA5)
    rc, tight, _ = raw.bwd(dy, want_in=False, tmp=tmp, tmp_bytes=raw.nbytes)
    assert rc == 0 and torch.equal(tight, gemb)
    assert bool((tmp[raw.nbytes:] == 0xA5).all()), "the backward wrote beyond gs_grid_encode_tmp_bytes"
    rc, short, _ = raw.bwd(dy, want_in=False, tmp=tmp, tmp_bytes=raw.nbytes - 1)
    assert rc == GS_E_SCRATCH and bool(torch.isnan(short).all())          # a return code: nothing ran


def test_unsupported_shapes_are_return_codes(api):
    t = ec.form_tensors(ec.FORM["D3C2-hash-smooth-noac"])
    raw = Raw(api, t)
    offs65 = torch.arange(66, dtype=torch.int32, device=DEV) * 8
    rc, out, dy = raw.fwd(L=65, offs=offs65)
    assert rc == GS_E_UNSUPPORTED and bool(torch.isnan(out).all()) and bool(torch.isnan(dy).all())
    rc, out, dy = raw.fwd(D=6)
    assert rc == GS_E_UNSUPPORTED and bool(torch.isnan(out).all())
    for kw in (dict(L=65, offs=offs65), dict(D=6)):
        rc, gemb, gin = raw.bwd(dy, **kw)
        assert rc == GS_E_UNSUPPORTED and bool(torch.isnan(gemb).all()) and bool(torch.isnan(gin).all())


# ---------------------------------------------------------------- spherical harmonics
@pytest.mark.parametrize("name", ec.SH_CASES)
@pytest.mark.parametrize("degree", range(1, 9))
def test_sh_case(degree, name):
    e = ec.sh_expectation(name, degree)
    xi = e.v.to(DEV).requires_grad_(True)
    y = shencoder.sh_encode(xi, degree, True)
    assert y.shape == (e.v.shape[0], degree * degree)
    y.backward(e.gout.to(DEV))
    if e.v.shape[0] == 0:
        assert xi.grad is None or xi.grad.shape == (0, 3)
        return
    d_out = (y.detach().cpu().double() - e.out).abs().max(dim=0).values
    d_in = (xi.grad.cpu().double() - e.gin).abs().max(dim=0).values
    _record("sh/%s/deg%d" % (name, degree), out_worst_over_bar=_ratio(d_out, e.bar_out), in_worst_over_bar=_ratio(d_in, e.bar_in),
            out_dist=d_out.tolist(), out_bar=e.bar_out.tolist(), in_dist=d_in.tolist(), in_bar=e.bar_in.tolist())
    print("sh %s deg %d: out %.3f of bar, in %.3f of bar" % (name, degree, _ratio(d_out, e.bar_out), _ratio(d_in, e.bar_in)))
    bad = torch.nonzero(d_out > e.bar_out).flatten().tolist()
    assert not bad, "output columns over their bar: %s" % [(c, float(d_out[c]), float(e.bar_out[c])) for c in bad]
    bad = torch.nonzero(d_in > e.bar_in).flatten().tolist()
    assert not bad, "input-gradient components over their bar: %s" % [(c, float(d_in[c]), float(e.bar_in[c])) for c in bad]
