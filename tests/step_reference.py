"""The tail of one train step on a flat, field-major, 59-float-per-Gaussian model, restated plainly: the arbiter of
tests/test_step_layout_cpu.py, tests/test_gpu_adam_layout.py and tests/test_gpu_step_layout.py.

Written from the reference's statements, not from the kernels' tables:

    LGDWT-GS/scene/gaussian_model.py:183-193   one torch.optim.Adam(lr=0.0, eps=1e-15) over the groups xyz, f_dc, f_rest
                                               (feature_lr / 20), opacity, scaling, rotation
    LGDWT-GS/train.py:266-268                  max_radii2D = max(., radii) and add_densification_stats on the visible rows
    LGDWT-GS/train.py:279-288                  optimizer.step(); with sparse_adam: visible = radii > 0, only those rows
    LGDWT-GS/scene/gaussian_model.py:471-473   xyz_gradient_accum += |viewspace grad .xy|, denom += 1

Every ELEMENT of the flat buffer gets its own learning rate and its own group's step count (element_tables); nothing here
knows about segments, periods, float4s, workgroups or phases.  adam_ref is torch.optim.Adam's update per element:

    m = b1 m + (1 - b1) g ;  v = b2 v + (1 - b2) g g ;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

  * dtype float64: the arbiter for parameters (betas 0.9 / 0.999 as torch holds them, in double);
  * dtype float32: the same statements in IEEE single, one rounding per operation, in the order the kernels spell out
    (b1*m + (1-b1)*g, b2*v + ((1-b2)*g)*g, 1-b1 and 1-b2 formed in single, the two bias corrections formed in double from the
    single betas and rounded once, lr / (1-b1^t) as the single product lr * (1 / (1-b1^t))).  The kernels are compiled
    without FMA contraction, so both moments are pure multiply-add sequences: the restatement is bit-exact for m and v.

The parameter takes a square root and a division more: its bar is MEASURED ON THE RESTATEMENT, never on a kernel -
param_tolerance: 4 x max|p32 - p64| over the field plus one ulp of the field's largest magnitude.  The kernels' sqrtf and
division turned out correctly rounded (MI355X, and the CPU oracle): every parameter of every case carries the float32
restatement's bits, so check_against_restatement asserts THAT for p as well, and prints the bar and the deviation for the record."""
import numpy as np
import torch

from gsplat_amd import synthetic
from gsplat_amd.trainer import FIELDS, LRS

BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
# group of every float of a Gaussian's row of each field (gaussian_model.py:183-193; features = [16, 3]: coefficient 0 is f_dc)
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
W, H = 96, 64


def field_offsets(P, fields=FIELDS):
    """{field: (first element, one past the last, floats per Gaussian)} of the field-major flat buffer"""
    out, off = {}, 0
    for name, n in fields:
        out[name] = (off, off + P * n, n)
        off += P * n
    return out


def element_tables(P, counts, skip=(), lrs=None, fields=FIELDS):
    """Per element of the flat buffer of P Gaussians: learning rate (float64), the step count of its group (int64: how often
    the group has been stepped, this step included), whether its group is stepped at all (`skip`: fields without a gradient this
    iteration - torch leaves such a parameter, its moments and its count alone), and its Gaussian's row index.
    counts: {field: count}."""
    lrs = dict(LRS) if lrs is None else lrs
    n = P * sum(w for _, w in fields)
    lr, t = np.zeros(n, np.float64), np.ones(n, np.int64)
    on, row = np.zeros(n, bool), np.zeros(n, np.int64)
    for name, (lo, hi, w) in field_offsets(P, fields).items():
        if name == "features":
            per_row = np.array([lrs["f_dc"]] * 3 + [lrs["f_rest"]] * (w - 3), np.float64)
        else:
            per_row = np.full(w, lrs[name], np.float64)
        lr[lo:hi] = np.tile(per_row, P)
        t[lo:hi] = max(int(counts[name]), 1)
        on[lo:hi] = name not in skip
        row[lo:hi] = np.repeat(np.arange(P), w)
    return lr, t, on, row


def adam_ref(p, g, m, v, lr, t, stepped, dtype=np.float64, betas=(BETA1, BETA2), eps=EPS):
    """One Adam step per element -> (p, m, v) as numpy arrays of `dtype`; elements with stepped == False keep every bit.
    p, g, m, v: float32 arrays (the model's own numbers); lr: float64 per element; t: int per element."""
    lr, t, stepped = np.asarray(lr, np.float64), np.asarray(t, np.int64), np.asarray(stepped, bool)
    if dtype == np.float64:
        p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))   # (float32 numbers convert exactly)
        b1, b2 = float(betas[0]), float(betas[1])
        pd, gd, md, vd = (x.astype(np.float64) for x in (p, g, m, v))
        m1 = b1 * md + (1.0 - b1) * gd
        v1 = b2 * vd + (1.0 - b2) * gd * gd
        bc1, bc2 = 1.0 - b1 ** t.astype(np.float64), 1.0 - b2 ** t.astype(np.float64)
        p1 = pd - (lr / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps))
        return np.where(stepped, p1, pd), np.where(stepped, m1, md), np.where(stepped, v1, vd)
    assert dtype == np.float32
    p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
    f = np.float32
    b1, b2, e = f(betas[0]), f(betas[1]), f(eps)     # (the C ABI takes them as float)
    one_b1, one_b2 = f(1.0) - b1, f(1.0) - b2
    td = t.astype(np.float64)
    inv_bc1 = (1.0 / (1.0 - np.float64(b1) ** td)).astype(f)             # double, rounded once
    inv_sqrt_bc2 = (1.0 / np.sqrt(1.0 - np.float64(b2) ** td)).astype(f)
    lr_bc1 = lr.astype(f) * inv_bc1
    with np.errstate(under="ignore"):
        m1 = b1 * m + one_b1 * g
        v1 = b2 * v + (one_b2 * g) * g
        denom = np.sqrt(v1) * inv_sqrt_bc2 + e
        p1 = p - lr_bc1 * (m1 / denom)
    for x in (m1, v1, p1):
        assert x.dtype == np.float32
    return np.where(stepped, p1, p), np.where(stepped, m1, m), np.where(stepped, v1, v)


def ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def param_tolerance(p32, p64):
    """(bar, max|p32 - p64|) of one field: four times the float32 restatement's own distance from the float64 one (room for a
    last-bit difference in sqrtf and the division) plus one ulp of the field's largest magnitude."""
    own = float(np.abs(p32.astype(np.float64) - p64).max()) if p32.size else 0.0
    big = float(np.abs(p64).max()) if p64.size else 0.0
    return 4.0 * own + ulp(big), own


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def same_bits(a, b):
    return bool(np.array_equal(bits(a), bits(b)))


def check_against_restatement(got_p, got_m, got_v, p0, g, m0, v0, lr, t, stepped, slices, what="", report=None):
    """got_*: float32 arrays after one step from (p0, m0, v0) with gradient g.  m and v must carry the float32 restatement's
    bits, p must lie within param_tolerance of the float64 restatement - per named slice {name: (lo, hi)}; elements that are
    not stepped must keep their bits.  Prints measured max|p32 - p64|, the bar and the largest deviation per slice."""
    p32, m32, v32 = adam_ref(p0, g, m0, v0, lr, t, stepped, np.float32)
    p64, _, _ = adam_ref(p0, g, m0, v0, lr, t, stepped, np.float64)
    got_p, got_m, got_v = (np.asarray(x, np.float32) for x in (got_p, got_m, got_v))
    for name, (lo, hi) in slices.items():
        if hi <= lo:
            continue
        s = slice(lo, hi)
        bad_m, bad_v = bits(got_m[s]) != bits(m32[s]), bits(got_v[s]) != bits(v32[s])
        assert not bad_m.any(), "%s %s: exp_avg differs from the float32 restatement at %d elements, first at %d (%r / %r)" % (
            what, name, int(bad_m.sum()), lo + int(np.argmax(bad_m)), got_m[s][bad_m][0], m32[s][bad_m][0])
        assert not bad_v.any(), "%s %s: exp_avg_sq differs from the float32 restatement at %d elements, first at %d (%r / %r)" % (
            what, name, int(bad_v.sum()), lo + int(np.argmax(bad_v)), got_v[s][bad_v][0], v32[s][bad_v][0])
        tol, own = param_tolerance(p32[s], p64[s])
        dev = np.abs(got_p[s].astype(np.float64) - p64[s])
        worst = float(dev.max())
        off32 = int((bits(got_p[s]) != bits(p32[s])).sum())
        line = "%s %-9s max|p32-p64| %.3e  bar %.3e  largest deviation %.3e  (%d of %d not the float32 restatement's bits)" % (
            what, name, own, tol, worst, off32, hi - lo)
        print(line)
        if report is not None:
            r = report.setdefault(name, dict(own=0.0, tol=0.0, dev=0.0, off32=0, n=0))
            r["own"], r["tol"], r["dev"] = max(r["own"], own), max(r["tol"], tol), max(r["dev"], worst)
            r["off32"] += off32
            r["n"] += hi - lo
        assert worst <= tol, "%s %s: parameter off the float64 restatement by %.3e at element %d (bar %.3e)" % (
            what, name, worst, lo + int(np.argmax(dev)), tol)
        # On an MI355X and on the CPU oracle every parameter of every case turned out to carry the float32 restatement's very
        # bits (sqrtf and the division are correctly rounded on both): that is what is asserted; the bar above is implied.
        bad_p = bits(got_p[s]) != bits(p32[s])
        assert not bad_p.any(), "%s %s: parameter differs from the float32 restatement at %d elements, first at %d (%r / %r)" % (
            what, name, int(bad_p.sum()), lo + int(np.argmax(bad_p)), got_p[s][bad_p][0], p32[s][bad_p][0])
        keep = ~np.asarray(stepped, bool)[s]
        if keep.any():
            assert np.array_equal(bits(got_p[s])[keep], bits(np.asarray(p0, np.float32)[s])[keep]), "%s %s: an element that is not stepped moved" % (what, name)


def stats_ref(accum, denom, max_radii, radii, mean2d_grad):
    """train.py:266-268 + gaussian_model.py:471-473 on the visible rows (radii > 0); the others are untouched.
    accum, denom: [P] float32, max_radii: [P] float32, radii: [P] int, mean2d_grad: [P, >=2] float32 -> new (accum, denom, max_radii).
    The norm in the kernels' single arithmetic: sqrtf(x*x + y*y)."""
    accum, denom, max_radii = (np.asarray(x, np.float32).reshape(-1).copy() for x in (accum, denom, max_radii))
    radii = np.asarray(radii).reshape(-1)
    g = np.asarray(mean2d_grad, np.float32)
    vis = radii > 0
    norm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(np.float32)
    accum[vis] = accum[vis] + norm[vis]
    denom[vis] = denom[vis] + np.float32(1.0)
    max_radii[vis] = np.maximum(max_radii[vis], radii[vis].astype(np.float32))
    return accum, denom, max_radii


# ---------------------------------------------------------------------------------------------------------------- the scene
_BASE = {}


WALL_ROWS = tuple(i for i in range(200, 223) if i % 3 != 1)      # 15 rows below 253, none of them lifted
WALL_DISTANCE, WALL_SIGMA, WALL_OPACITY = 0.3, 0.15, 0.99


def scene(P, lifted=slice(1, None, 3), wall=None):
    """The first P rows of synthetic.trained_like(1024, seed=3, sh_degree=3) with rows 1::3 lifted by 50 in z (outside every
    frustum): invisible rows interleave with visible ones inside float4s, row 0 stays visible.

    wall (default: P >= 253): five of WALL_ROWS in front of each of the cameras 0..2 - round, opaque, 0.3 in front of the eye and
    a quarter of the image to the side, 66 pixels wide there.  Five layers of alpha >= 0.84 saturate every pixel within 38
    pixels of their centre, a block of 3 x 3 tiles: a Gaussian whose footprint lies inside that block is visible, listed, and
    never reached by the backward blend - a VISIBLE Gaussian WITHOUT instances on full and on the reference's lists, where the
    scene alone (nothing saturates at a few hundred Gaussians) has none.  The rest of the image stays unsaturated."""
    if "sc" not in _BASE:
        _BASE["sc"] = synthetic.trained_like(1024, seed=3, sh_degree=3)
    assert 1 <= P <= 1024
    sc = {k: (v[:P].clone() if torch.is_tensor(v) else v) for k, v in _BASE["sc"].items()}
    sc["means3D"][lifted, 2] += 50.0
    if wall is None:
        wall = P >= 253
    if wall:
        assert P > max(WALL_ROWS)
        px = WALL_DISTANCE * np.tan(0.5 * 0.6911112070083618) / (W / 2)      # world units per pixel at the wall
        for ci, cam in enumerate(cameras(3)):
            eye = cam.camera_center.double().numpy()
            fwd = -eye / np.linalg.norm(eye)                    # (the orbit cameras look at the origin)
            right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
            right /= np.linalg.norm(right)
            up = np.cross(right, fwd)
            rows = list(WALL_ROWS[5 * ci:5 * ci + 5])
            for k, row in enumerate(rows):      # (2 mm apart in depth: no ties in the depth order)
                centre = eye + (WALL_DISTANCE + 0.002 * k) * fwd + 24 * px * right + 8 * px * up
                sc["means3D"][row] = torch.from_numpy(centre).float()
            sc["scales"][rows] = WALL_SIGMA
            sc["opacities"][rows] = WALL_OPACITY
            sc["rotations"][rows] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    return sc


def cameras(n=4):
    return synthetic.orbit_cameras(W, H)[:n]


def mixed_float4s(flags, width):
    """Number of float4s of a [P, width] row array (from an aligned base) that hold elements of rows with different flags"""
    f = np.repeat(np.asarray(flags).astype(np.int64), width)
    n = 0
    for lo in range(0, f.size, 4):    # (the last float4 may be a partial one)
        n += int(f[lo:lo + 4].min() != f[lo:lo + 4].max())
    return n


# -------------------------------------------------------------------------------------- the stand-alone kernel's case table
class AdamCase:
    """One call of gs_adam_step / _masked / _gated: n elements, a hand-made segment table, optional row mask and gate."""

    def __init__(self, name, n, segs, step=7, mask=None, gate=None, seed=0):
        self.name, self.n, self.segs, self.step, self.mask, self.gate, self.seed = name, int(n), segs, step, mask, gate, seed

    def data(self):
        """p, g, m, v (float32, non-zero starting moments; every 5th gradient exactly zero)"""
        r = np.random.RandomState(1000 + self.seed + self.n)
        n = self.n
        p = r.standard_normal(n).astype(np.float32)
        g = (r.standard_normal(n) * 10.0 ** r.uniform(-6, 0, n)).astype(np.float32)
        g[::5] = 0.0
        m = (r.standard_normal(n) * 1e-3).astype(np.float32)
        v = (r.random_sample(n) * 1e-5).astype(np.float32)
        return p, g, m, v

    def tables(self):
        """Per element, from the segment list alone and by a plain loop over elements: lr, step count, stepped"""
        n = self.n
        lr, t, stepped = np.zeros(n, np.float64), np.ones(n, np.int64), np.zeros(n, bool)
        gated = self.gate is not None and self.gate != 0.0
        for s in self.segs:
            for i in range(max(s["begin"], 0), min(s["end"], n)):
                k = i - s["begin"]
                lr[i] = s["lr_b"] if (s.get("period", 0) > 0 and k % s["period"] >= s["split"]) else s["lr_a"]
                t[i] = s["step"] if s.get("step", 0) > 0 else self.step
                on = True
                if self.mask is not None and s.get("row_width", 0) > 0:
                    on = self.mask[k // s["row_width"]] > 0
                stepped[i] = on and not gated
        return lr, t, stepped

    def seg_array(self):
        from gsplat_amd.capi import GsAdamSeg
        arr = (GsAdamSeg * max(len(self.segs), 1))()
        for k, s in enumerate(self.segs):
            arr[k].begin, arr[k].end, arr[k].lr_a, arr[k].lr_b = s["begin"], s["end"], s["lr_a"], s.get("lr_b", 0.0)
            arr[k].period, arr[k].split, arr[k].step = s.get("period", 0), s.get("split", 0), s.get("step", 0)
            arr[k].row_width = s.get("row_width", 0)
        return arr


def _seg(begin, end, lr_a, lr_b=0.0, period=0, split=0, step=0, row_width=0):
    return dict(begin=begin, end=end, lr_a=lr_a, lr_b=lr_b, period=period, split=split, step=step, row_width=row_width)


SIZES = (1, 2, 3, 5, 1023, 1025, 4099)


def adam_cases():
    """The case table of the stand-alone kernel (part of the arbiter: validated on the CPU oracle before a GPU sees it)."""
    cases = []
    for n in SIZES:
        # one segment over everything: the n & 3 tail, fewer elements than a float4, more than one workgroup (n > 1024)
        cases.append(AdamCase("whole_n%d" % n, n, [_seg(0, n, 0.01, step=3)]))
        # a segment that ends 1..3 elements before n
        for short in (1, 2, 3):
            if n > short:
                cases.append(AdamCase("ends_%d_early_n%d" % (short, n), n, [_seg(0, n - short, 0.02, step=2)]))
    for n in (1023, 1025, 4099):
        k4 = 4 * (n // 8)
        for r in (1, 2, 3):
            # two segments meeting at 4k + r: different rates, different step counts (different bias corrections)
            cases.append(AdamCase("edge_4k+%d_n%d" % (r, n), n,
                                  [_seg(0, k4 + r, 0.01, step=1), _seg(k4 + r, n, 0.003, step=9)]))
            # ... with a gap of r elements no segment covers
            cases.append(AdamCase("gap_%d_n%d" % (r, n), n,
                                  [_seg(0, k4 + 1, 0.01, step=4), _seg(k4 + 1 + r, n, 0.003, step=2)]))
        for b in (0, 1, 2, 3):
            # learning-rate phase: begin % 4 = b puts the lr_a -> lr_b change and the period wrap at every place in a float4
            cases.append(AdamCase("phase48_begin%d_n%d" % (b, n), n,
                                  [_seg(b, n, 0.0025, 0.0025 / 20, 48, 3, step=5)]))
            cases.append(AdamCase("phase5_begin%d_n%d" % (b, n), n, [_seg(b, n, 0.02, 0.001, 5, 2, step=6)]))
        # a negative begin (the chunked data-parallel step shifts the table): the phase is kept
        cases.append(AdamCase("phase48_negative_begin_n%d" % n, n, [_seg(-52, n, 0.0025, 0.0025 / 20, 48, 3, step=2)]))
        for width in (1, 3):
            for b in (1, 2, 3):
                rows = (n - b) // width
                mask = np.zeros(rows, np.float32)
                mask[::2] = 1.0                      # alternates inside float4s
                mask[rows // 2:rows // 2 + 5] = 0.0  # ... and a run of rows that are off
                cases.append(AdamCase("mask_w%d_begin%d_n%d" % (width, b, n), n,
                                      [_seg(b, b + rows * width, 0.005, step=3, row_width=width)], mask=mask))
        cases.append(AdamCase("gate_closed_n%d" % n, n, [_seg(0, n, 0.01, step=3)], gate=1.0))
        cases.append(AdamCase("gate_open_n%d" % n, n, [_seg(1, n - 2, 0.01, step=3)], gate=0.0))
    w = 3
    rows = 341
    mask = (np.arange(rows) % 3 != 1).astype(np.float32)
    cases.append(AdamCase("mask_and_open_gate", 1025, [_seg(2, 2 + rows * w, 0.005, 0.0007, 5, 2, step=4, row_width=w)], mask=mask, gate=0.0))
    cases.append(AdamCase("mask_and_closed_gate", 1025, [_seg(2, 2 + rows * w, 0.005, step=4, row_width=w)], mask=mask, gate=-2.0))
    return cases


GUARD = 4


def run_adam_case(case, call, device="cpu"):
    """Runs `case` once through `call(kind, p, g, m, v, n, segs, nseg, b1, b2, eps, step, gate, mask)` (pointers; kind
    "adam_step" / "adam_step_gated" / "adam_step_masked") on buffers that start on 16 bytes, with GUARD guard floats before the
    start and behind element n -> dict of float32 numpy arrays after the call (guards included: keys p, m, v, g) and the
    inputs.  device: where the buffers live."""
    n = case.n
    p, g, m, v = case.data()
    bufs, views = {}, {}
    for key, x in (("p", p), ("g", g), ("m", m), ("v", v)):
        # over-allocate and start the array at the first address = 0 mod 16 that leaves GUARD floats before it
        raw = torch.full((n + 2 * GUARD + 8,), float("nan"), dtype=torch.float32, device=device)
        skew = (-(raw.data_ptr() // 4) - GUARD) % 4
        lo = skew                      # guard words lo .. lo + GUARD - 1, array from lo + GUARD
        assert (raw.data_ptr() + 4 * (lo + GUARD)) % 16 == 0
        guard = torch.tensor([1.5, -2.5, 3.25, -4.75], dtype=torch.float32)
        raw[lo:lo + GUARD] = guard.to(device)
        raw[lo + GUARD + n:lo + 2 * GUARD + n] = (guard * 3).to(device)
        raw[lo + GUARD:lo + GUARD + n] = torch.from_numpy(x).to(device)
        bufs[key], views[key] = raw, (lo, raw[lo + GUARD:lo + GUARD + n])
    gate_t = None if case.gate is None else torch.tensor([case.gate], dtype=torch.float32, device=device)
    mask_t = None if case.mask is None else torch.from_numpy(case.mask).to(device)
    kind = "adam_step_masked" if case.mask is not None else ("adam_step_gated" if case.gate is not None else "adam_step")
    segs = case.seg_array()
    call(kind, views["p"][1].data_ptr(), views["g"][1].data_ptr(), views["m"][1].data_ptr(), views["v"][1].data_ptr(), n, segs,
         len(case.segs), BETA1, BETA2, EPS, case.step, None if gate_t is None else gate_t.data_ptr(),
         None if mask_t is None else mask_t.data_ptr())
    if device != "cpu":
        torch.cuda.synchronize()
    out = dict(inputs=(p, g, m, v))
    for key in ("p", "g", "m", "v"):
        lo, _ = views[key]
        whole = bufs[key][lo:lo + 2 * GUARD + n].cpu().numpy()
        out[key] = whole[GUARD:GUARD + n]
        out[key + "_guards"] = np.concatenate((whole[:GUARD], whole[GUARD + n:]))
    want = np.concatenate((np.array([1.5, -2.5, 3.25, -4.75], np.float32), np.array([1.5, -2.5, 3.25, -4.75], np.float32) * 3))
    out["guards_want"] = want
    return out


def check_adam_case(case, out, report=None):
    """The arbiter's verdict on one run of a case (run_adam_case)."""
    p, g, m, v = out["inputs"]
    lr, t, stepped = case.tables()
    for key in ("p", "g", "m", "v"):
        assert same_bits(out[key + "_guards"], out["guards_want"]), "%s: a guard word of %s changed" % (case.name, key)
    assert same_bits(out["g"], g), "%s: the gradients were written" % case.name
    off = ~stepped
    for key, x0 in (("p", p), ("m", m), ("v", v)):
        assert np.array_equal(bits(out[key])[off], bits(x0)[off]), "%s: an element of %s outside every stepped row moved" % (case.name, key)
    check_against_restatement(out["p"], out["m"], out["v"], p, g, m, v, lr, t, stepped, {"all": (0, case.n)}, what=case.name,
                              report=report)
    if stepped.any():
        assert not same_bits(out["m"], m), "%s: nothing moved" % case.name
