"""gs_adam_step_tensors (one launch over the reference's six parameter tensors, mask first) and the classes on top of it,
against the numpy restatement of tests/sparse_adam_reference.py and against the older kernels it must agree with bit for bit.

Per row count P, both rules and every mask of sparse_adam_reference.masks: exp_avg and exp_avg_sq carry the float32
restatement's bits, the parameter lies within step_reference.param_tolerance of the float64 restatement, rows that are not
visible keep every bit (NaN is planted in their g, m and v), the gradient is never written and the guard words around every
array keep their bits.  The number of parameter elements that differ from the float32 restatement's bits is printed; on an
MI355X it is zero for every case (sqrtf and the division are correctly rounded), so that is asserted as well."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_adam_reference as ref
from step_reference import BETA1, BETA2, EPS, bits, param_tolerance

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 5, 63, 64, 65, 255, 256, 257, 1023)
STEPS = (1, 2, 3, 5, 8, 4)      # each tensor its own step count
GUARD = 4                       # floats on both sides of every array (16 bytes: the arrays stay aligned)
GUARD_BITS = 0x7fa5c3e1         # (a NaN with a payload: a guard that was read and written back through arithmetic would change)
NAN_BITS = 0x7fc01234


class Arrays:
    """p, g, m, v of the six tensors for P rows, each array between guard words, on the host (numpy) and on the device."""

    def __init__(self, P, dev, seed=0, row_mask=None):
        rng = np.random.default_rng(seed * 7919 + P)
        self.P, self.dev = P, dev
        self.host, self.bufs = [], []
        for w in ref.WIDTHS:
            n = P * w
            h = dict(p=rng.normal(size=n), g=rng.normal(size=n) * 10.0 ** rng.uniform(-4, 1, n), m=rng.normal(size=n) * 0.1,
                     v=rng.normal(size=n) ** 2 * 1e-2)
            h = {k: x.astype(np.float32) for k, x in h.items()}
            if row_mask is not None:     # what must never be read into a result: NaN in every row that is not visible
                off = ~np.repeat(np.asarray(row_mask, bool), w)
                for k in ("g", "m", "v"):
                    h[k].view(np.uint32)[off] = NAN_BITS
            self.host.append(h)
            d = {}
            for k, x in h.items():
                buf = np.full(n + 2 * GUARD, 0, np.uint32)
                buf[:GUARD] = buf[GUARD + n:] = GUARD_BITS
                buf[GUARD:GUARD + n] = x.view(np.uint32)
                d[k] = torch.from_numpy(buf.view(np.int32)).to(dev)
            self.bufs.append(d)

    def view(self, i, k):
        """the tensor proper (float32 view between the guards)"""
        n = self.P * ref.WIDTHS[i]
        return self.bufs[i][k][GUARD:GUARD + n].view(torch.float32)

    def table(self, lrs=ref.LRS, steps=STEPS, row_widths=ref.WIDTHS, only=None):
        from gsplat_amd.capi import GsAdamTensor
        idx = list(range(6)) if only is None else list(only)
        t = (GsAdamTensor * len(idx))()
        for e, i in zip(t, idx):
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = (self.view(i, k).data_ptr() for k in "pgmv")
            e.n, e.row_width, e.step, e.lr = self.P * ref.WIDTHS[i], row_widths[i], steps[i], lrs[i]
        return t

    def read(self, i, k):
        return self.view(i, k).cpu().numpy()

    def guards_intact(self):
        for d in self.bufs:
            for k, buf in d.items():
                b = buf.cpu().numpy().view(np.uint32)
                if not (np.all(b[:GUARD] == GUARD_BITS) and np.all(b[-GUARD:] == GUARD_BITS)):
                    return False
        return True


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _mask_dev(mask, dev):
    return None if mask is None else torch.from_numpy(np.asarray(mask, bool)).to(dev)


def _call(hip, a, flags, mask_t, table=None, nt=None, P=None):
    table = a.table() if table is None else table
    return hip.api.raw("adam_step_tensors")(table, len(table) if nt is None else nt, a.P if P is None else P, BETA1, BETA2, EPS,
                                           flags, None if mask_t is None else mask_t.data_ptr(), _stream())


@pytest.mark.parametrize("P", ROWS)
def test_one_launch_against_the_restatement(hip, P):
    from gsplat_amd.capi import ADAM_NO_BIAS_CORRECTION
    dev = torch.device("cuda:0")
    off32_total = 0
    for bias_correction in (False, True):
        for name, mask in ref.masks(P).items():
            what = "P=%d %s %s" % (P, "torch rule" if bias_correction else "no-bias rule", name)
            a = Arrays(P, dev, seed=1, row_mask=mask)
            mask_t = _mask_dev(mask, dev)
            assert _call(hip, a, 0 if bias_correction else ADAM_NO_BIAS_CORRECTION, mask_t) == 0, what
            torch.cuda.synchronize()
            assert a.guards_intact(), what + ": a guard word changed"
            for i, (w, lr, t) in enumerate(zip(ref.WIDTHS, ref.LRS, STEPS)):
                h = a.host[i]
                p32, m32, v32 = ref.sparse_adam_ref(h["p"], h["g"], h["m"], h["v"], lr, t, w, mask, bias_correction, np.float32)
                p64, _, _ = ref.sparse_adam_ref(h["p"], h["g"], h["m"], h["v"], lr, t, w, mask, bias_correction, np.float64)
                gp, gg, gm, gv = (a.read(i, k) for k in "pgmv")
                assert np.array_equal(bits(gg), bits(h["g"])), "%s %s: the gradient was written" % (what, ref.NAMES[i])
                assert np.array_equal(bits(gm), bits(m32)), "%s %s: exp_avg is not the float32 restatement" % (what, ref.NAMES[i])
                assert np.array_equal(bits(gv), bits(v32)), "%s %s: exp_avg_sq is not the float32 restatement" % (what, ref.NAMES[i])
                on = ref.stepped_elements(P, w, mask)
                assert np.array_equal(bits(gp)[~on], bits(h["p"])[~on]), "%s %s: a row that is not visible moved" % (what, ref.NAMES[i])
                if on.any():
                    tol, own = param_tolerance(p32[on], p64[on])
                    dev_max = float(np.abs(gp[on].astype(np.float64) - p64[on]).max())
                    off32 = int((bits(gp) != bits(p32)).sum())
                    off32_total += off32
                    print("%s %-8s max|p32-p64| %.3e  bar %.3e  largest deviation %.3e  (%d of %d not the float32 restatement's bits)"
                          % (what, ref.NAMES[i], own, tol, dev_max, off32, int(on.sum())))
                    assert dev_max <= tol, "%s %s: parameter off the float64 restatement by %.3e (bar %.3e)" % (
                        what, ref.NAMES[i], dev_max, tol)
                    assert np.any(bits(gp)[on] != bits(h["p"])[on]), "%s %s: nothing was stepped" % (what, ref.NAMES[i])
                    # measured on an MI355X: no parameter element of any case differs from the float32 restatement's bits
                    assert off32 == 0, "%s %s: %d parameter elements are not the float32 restatement's bits" % (what, ref.NAMES[i], off32)
    print("P=%d: %d parameter elements off the float32 restatement's bits in all" % (P, off32_total))


@pytest.mark.parametrize("P", ROWS)
def test_same_bits_as_the_older_kernels(hip, P):
    """flags = 0 without a mask = six gs_adam_step calls; with a mask = gs_adam_step_masked on the same data laid out flat."""
    from gsplat_amd.capi import GsAdamSeg
    dev = torch.device("cuda:0")
    # ---- dense: one launch over six tensors against one gs_adam_step per tensor
    a, b = Arrays(P, dev, seed=2), Arrays(P, dev, seed=2)
    assert _call(hip, a, 0, None) == 0
    for i, (w, lr, t) in enumerate(zip(ref.WIDTHS, ref.LRS, STEPS)):
        seg = (GsAdamSeg * 1)()
        seg[0].begin, seg[0].end, seg[0].lr_a, seg[0].step = 0, P * w, lr, t
        hip.api.call("adam_step", *(b.view(i, k).data_ptr() for k in "pgmv"), P * w, seg, 1, BETA1, BETA2, EPS, t, _stream())
    torch.cuda.synchronize()
    for i in range(6):
        for k in "pgmv":
            assert np.array_equal(bits(a.read(i, k)), bits(b.read(i, k))), "dense %s %s P=%d" % (ref.NAMES[i], k, P)
    assert a.guards_intact() and b.guards_intact()
    # ---- masked: against gs_adam_step_masked over ONE flat buffer holding the six tensors back to back, float mask
    mask = ref.masks(P)["random30"] | (np.arange(P) == P - 1)
    a = Arrays(P, dev, seed=3, row_mask=mask)
    flat = {k: torch.cat([a.view(i, k) for i in range(6)]).clone() for k in "pgmv"}
    assert all(x.data_ptr() % 16 == 0 for x in flat.values())
    segs, off = (GsAdamSeg * 6)(), 0
    for s, w, lr, t in zip(segs, ref.WIDTHS, ref.LRS, STEPS):
        s.begin, s.end, s.lr_a, s.step, s.row_width = off, off + P * w, lr, t, w
        off += P * w
    fmask = torch.from_numpy(mask.astype(np.float32)).to(dev)
    hip.api.call("adam_step_masked", *(flat[k].data_ptr() for k in "pgmv"), off, segs, 6, BETA1, BETA2, EPS, 1, None,
                 fmask.data_ptr(), _stream())
    assert _call(hip, a, 0, _mask_dev(mask, dev)) == 0
    torch.cuda.synchronize()
    for k in "pgmv":
        got = np.concatenate([a.read(i, k) for i in range(6)])
        assert np.array_equal(bits(got), bits(flat[k].cpu().numpy())), "masked %s P=%d" % (k, P)


def test_status_codes(hip):
    from gsplat_amd.capi import ADAM_NO_BIAS_CORRECTION, GsAdamTensor
    dev = torch.device("cuda:0")
    P = 5
    a = Arrays(P, dev, seed=4)
    before = [[a.read(i, k).copy() for k in "pgmv"] for i in range(6)]
    mask_t = _mask_dev(np.ones(P, bool), dev)
    NULL, SHAPE, UNSUPPORTED = -1, -2, -5
    nine = (GsAdamTensor * 9)()
    assert _call(hip, a, 0, None, table=nine, nt=9) == SHAPE
    assert _call(hip, a, 0, None, nt=-1) == SHAPE
    assert _call(hip, a, 0, None, table=a.table(steps=(1, 1, 0, 1, 1, 1))) == SHAPE            # step = 0 with flags = 0 ...
    assert _call(hip, a, 0, mask_t, P=P + 1) == SHAPE                                          # n != P * row_width with a mask
    assert _call(hip, a, 0, mask_t, table=a.table(row_widths=(3, 3, 44, 1, 3, 4))) == SHAPE
    t = a.table()
    t[2].param += 4                                                                            # a base offset by 4 bytes
    assert _call(hip, a, 0, None, table=t) == UNSUPPORTED
    t = a.table()
    t[4].exp_avg_sq = None
    assert _call(hip, a, 0, None, table=t) == NULL
    assert hip.api.raw("adam_step_tensors")(None, 3, P, BETA1, BETA2, EPS, 0, None, _stream()) == NULL
    assert _call(hip, a, 2, None) == UNSUPPORTED                                               # an unknown flag bit
    assert hip.api.raw("adam_step_tensors")(None, 0, P, BETA1, BETA2, EPS, 0, None, _stream()) == 0       # nt = 0: nothing to do
    t = a.table()
    for e in t:
        e.n = 0                                                                                # only empty tensors: no launch
        e.param = e.grad = None
    assert _call(hip, a, 0, None, table=t) == 0
    torch.cuda.synchronize()
    for i in range(6):
        for j, k in enumerate("pgmv"):
            assert np.array_equal(bits(a.read(i, k)), bits(before[i][j])), "a refused call wrote %s %s" % (ref.NAMES[i], k)
    # ... while the rule without bias correction does not read `step`
    assert _call(hip, a, ADAM_NO_BIAS_CORRECTION, None, table=a.table(steps=(0,) * 6)) == 0
    torch.cuda.synchronize()
    assert not np.array_equal(bits(a.read(0, "p")), bits(before[0][0])) and a.guards_intact()


def _groups(P, dev, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = ((P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4))
    return [{"params": [torch.nn.Parameter(torch.randn(s, generator=g).to(dev))], "lr": lr, "name": n}
            for s, lr, n in zip(shapes, ref.LRS, ref.NAMES)]


def _set_grads(groups, seed, skip=()):
    g = torch.Generator().manual_seed(seed)
    for group in groups:
        p = group["params"][0]
        grad = torch.randn(p.shape, generator=g).to(p.device)
        p.grad = None if group["name"] in skip else grad


def _state_bits(opt):
    out = []
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state.get(p, {})
        out.append((bits(p.detach().cpu().numpy()), None if not st else bits(st["exp_avg"].cpu().numpy()),
                    None if not st else bits(st["exp_avg_sq"].cpu().numpy()), None if not st else float(st["step"])))
    return out


def test_fused_adam_with_fused_groups_is_fused_adam(hip):
    from gsplat_amd.optim import FusedAdam
    dev, P = torch.device("cuda:0"), 257
    one = FusedAdam(_groups(P, dev, 11), lr=0.0, eps=1e-15)
    fused = FusedAdam(_groups(P, dev, 11), lr=0.0, eps=1e-15, fuse_groups=True)
    assert one.fuse_groups is False and fused.fuse_groups is True
    for s in range(3):
        for opt in (one, fused):
            _set_grads(opt.param_groups, 20 + s, skip=("opacity",) if s == 1 else ())   # (a group falls a step behind)
            opt.step()
    torch.cuda.synchronize()
    for x, y, name in zip(_state_bits(one), _state_bits(fused), ref.NAMES):
        assert x[3] == y[3] == (2.0 if name == "opacity" else 3.0)
        for u, v in zip(x[:3], y[:3]):
            assert np.array_equal(u, v), name


@pytest.mark.parametrize("bias_correction", [False, True])
def test_class_dense_step_is_the_all_visible_step_and_a_group_without_grad_is_skipped(hip, bias_correction):
    from gsplat_amd.optim import SparseGaussianAdam
    dev, P = torch.device("cuda:0"), 257
    dense = SparseGaussianAdam(_groups(P, dev, 12), lr=0.0, eps=1e-15, bias_correction=bias_correction)
    masked = SparseGaussianAdam(_groups(P, dev, 12), lr=0.0, eps=1e-15, bias_correction=bias_correction)
    start = _state_bits(dense)
    for s in range(2):
        skip = ("scaling",) if s == 1 else ()
        for opt in (dense, masked):
            _set_grads(opt.param_groups, 30 + s, skip=skip)
        dense.step()
        masked.step(torch.ones(P, dtype=torch.bool, device=dev), P)
    torch.cuda.synchronize()
    for x, y, s0, name in zip(_state_bits(dense), _state_bits(masked), start, ref.NAMES):
        assert x[3] == y[3] == (1.0 if name == "scaling" else 2.0), name      # skipped, counter included
        for u, v in zip(x[:3], y[:3]):
            assert np.array_equal(u, v), name
        assert not np.array_equal(x[0], s0[0])
    # the first step, from zero moments, against the restatement (uint8 visibility, every other row)
    opt = SparseGaussianAdam(_groups(P, dev, 13), lr=0.0, eps=1e-15, bias_correction=bias_correction)
    _set_grads(opt.param_groups, 40)
    p0 = [g["params"][0].detach().cpu().numpy().ravel().copy() for g in opt.param_groups]
    g0 = [g["params"][0].grad.cpu().numpy().ravel().copy() for g in opt.param_groups]
    vis = (torch.arange(P) % 2 == 0).to(torch.uint8).to(dev)
    opt.step(vis, P)
    torch.cuda.synchronize()
    for group, p, g, w in zip(opt.param_groups, p0, g0, ref.WIDTHS):
        z = np.zeros_like(p)
        p32, m32, v32 = ref.sparse_adam_ref(p, g, z, z, group["lr"], 1, w, vis.cpu().numpy(), bias_correction, np.float32)
        st = opt.state[group["params"][0]]
        assert float(st["step"]) == 1.0 and st["exp_avg"].shape == group["params"][0].shape
        assert np.array_equal(bits(st["exp_avg"].cpu().numpy().ravel()), bits(m32)), group["name"]
        assert np.array_equal(bits(st["exp_avg_sq"].cpu().numpy().ravel()), bits(v32)), group["name"]
        assert np.array_equal(bits(group["params"][0].detach().cpu().numpy().ravel()), bits(p32)), group["name"]
    # what the class refuses on the GPU names the group
    bad = SparseGaussianAdam([{"params": [torch.nn.Parameter(torch.zeros((8, 3), device=dev).t())], "lr": 0.1, "name": "tilted"}],
                             lr=0.0, eps=1e-15)
    bad.param_groups[0]["params"][0].grad = torch.zeros((3, 8), device=dev)
    with pytest.raises(RuntimeError, match="'tilted'.*contiguous"):
        bad.step()
    half = SparseGaussianAdam([{"params": [torch.nn.Parameter(torch.zeros((8, 3), device=dev, dtype=torch.float16))], "lr": 0.1,
                                "name": "half"}], lr=0.0, eps=1e-15)
    half.param_groups[0]["params"][0].grad = torch.zeros((8, 3), device=dev, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="'half'.*fp32"):
        half.step()
    base = torch.zeros(8 * 3 + 1, device=dev)
    odd = SparseGaussianAdam([{"params": [torch.nn.Parameter(base[1:].view(8, 3))], "lr": 0.1, "name": "odd"}], lr=0.0, eps=1e-15)
    odd.param_groups[0]["params"][0].grad = torch.zeros((8, 3), device=dev)
    with pytest.raises(RuntimeError, match="'odd'.*16-byte"):
        odd.step()
