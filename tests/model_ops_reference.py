"""The parameter activations of csrc/gs_model.hip (act_fwd_kernel / act_bwd_kernel) and of their copies (activate_* in
csrc/gs_math.h, the activation backward of preprocess_bwd_step_kernel in csrc/gs_preprocess_bwd.hip, gso_activations_* in
oracle/gs_oracle_loss.cpp): a float64 restatement of the torch semantics the kernels claim, a per-element bar for every output,
and one table of constructed rows.  tests/test_model_ops_cases_cpu.py proves the restatement against torch and holds the oracle
to it; tests/test_gpu_model_ops.py holds the HIP kernels to it.

The restatement (float64, from the fp32 inputs; eps32 = float32(1e-12), the value F.normalize's eps has in fp32)
    scales     = exp(x)
    v          = q / max(|q|, eps32)
    s          = 1 / (1 + exp(-x))
    d_scaling  = g exp(x)                 (torch: grad * result - where the fp32 result is inf it is g * inf: NaN for g = 0)
    d_opacity  = g s (1 - s)              (1 - s formed as 1 / (1 + exp(x)): no cancellation in the reference)
    d_rotation = (g - v (v.g)) / |q|      where |q| >= eps32 - torch's clamp_min passes the gradient at the tie -
                 g / eps32                elsewhere

The bars.  u = 2^-24 (half an ulp of 1).  Every fp32 operation of the kernels (+, *, /, sqrtf) is correctly rounded: relative
error u.  expf is not: the installed ROCm documents no bound for it, so E u is MEASURED - the maximum of
tests/tools/dng_reg_act_probe.hip (the math library's function alone against float64) times the 2 x margin
tests/test_gpu_dng_reg.py took for gs_dng_reg.hip: profiles/dng_reg_timing.txt, "exp over [-7, 1.5] ... 1.406 x 2^-24" and
"exp over [-104, 89] ... 1.381 x 2^-24"; EXPF_E = 2 x the larger.  Host expf (glibc) is within 1 ulp = 2 u, so the same bars
hold for the oracle and for torch's CPU fp32.  Counts are first order in u; the second-order terms are below 1e-6 of them and are
covered by rounding each count up to a whole number (2 x 1.406 = 2.812 enters as it is, the whole-number roundings are the added
integers).  No bar is scaled by anything but the element's own reference value and cotangent.

    scales      E u |ref|                       one expf
    d_scaling   (E + 1) u |ref|                 expf, one product
    opacity     (E + 2) u |ref|                 expf (E; halved or less by the 1 + . for x > 0), the sum 1, the quotient 1
    d_opacity   |g| ( |1 - 2 s| ds + 3 u s (1 - s) ),  ds = (E + 2) u s
                                                d/ds [s (1 - s)] = 1 - 2 s carries the forward's error ds into the product -
                                                this is the cancellation of torch's own 1 - s, and with it s rounding to
                                                exactly 1 (x >= 17: gradient 0) is inside the bar; then the roundings of
                                                1 - s and of the two products, 3 u
    v           projected: 4 u |ref|            a square (1) and three sums (3) on the largest path, every term >= 0 so the
                                                sum's relative error is at most its worst term's: 4 -> sqrtf halves it and rounds:
                                                3 -> the quotient: 4
                clamped (|q| < eps32 in fp32 and in float64): bit-equal to float32(q64 / eps32) - fmaxf returns eps32 and q / eps32
                                                is ONE correctly rounded division
    d_rotation  projected: 24 u (1 / |q|) ( |g_k| + |v_k| sum_j |v_j g_j| )
                                                inv = 1 / norm: 3 + 1 = 4; v_j = q_j inv: 5; v_j g_j: 6, three sums: 9 on
                                                sum_j |v_j g_j|; v_k dot: 5 + 9 + 1 = 15; the difference: 1 on both terms; the
                                                product with inv: 4 + 1.  g_k collects 1 + 5 = 6, v_k dot 15 + 1 + 5 = 21.  The
                                                kernel's errors are relative to the ABSOLUTE contributions (the difference can
                                                cancel), so the bar is 21 -> 24 times their sum, not times |ref|
                clamped: bit-equal to float32(g64 / eps32), one correctly rounded division
    floor       every bar is at least FLT_MIN = 2^-126: below the normal numbers any value within FLT_MIN of the reference
                passes (gradual underflow, or a flush to zero, of the result).  The same floor holds for the INTERMEDIATE a
                gradient is formed from: where exp(x) (d_scaling) or s (d_opacity) is below FLT_MIN the forward's bar lets it
                be anywhere within FLT_MIN, and the backward cannot be held to more - 1 / (1 + expf(89.5)) is 1 / inf = 0 in
                fp32 (torch's CPU kernel included) where s = 1.4e-39.  So ds and the error of exp(x) are FLT_MIN there,
                multiplied by |g| like the relative terms
    overflow    +-inf and NaN must appear where, and only where, float32(reference) has them.  cases() asserts that no finite
                reference lies within its bar of the overflow threshold, so that decision is the reference's

The case table (rows(), cycled to P rows by cases(P)): see ROTATIONS, OPACITIES, SCALINGS, COTANGENT_KINDS below; the periods of
the cycles are pairwise coprime, so every (row, cotangent kind) pair occurs within 7 x 57 = 399 rows.
"""
import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)
TO_INF = 2.0 ** 128 * (1.0 - 2.0 ** -25)    # float32(x) is infinite from here on (round to nearest even)
LN_FLT_MAX = float(np.log(np.float64(FLT_MAX)))    # 88.72
EPS32 = np.float32(1e-12)
EPS = float(EPS32)
# profiles/dng_reg_timing.txt: "exp over [-7, 1.5] ... (1.406 x 2^-24)", "exp over [-104, 89] ... (1.381 x 2^-24)"; x 2 margin
EXPF_MEASURED = 1.406
EXPF_E = 2.0 * EXPF_MEASURED
SIZES = (1, 63, 64, 255, 256, 257, 1023)
WIDTHS = (3, 48, 1, 3, 4)     # the model's flat order: xyz, features, opacity, scaling, rotation
OUTPUTS = ("scales", "v", "opacity", "d_scaling", "d_rotation", "d_opacity")


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _rotations():
    g = np.random.default_rng(11)
    rows, kinds = [], []

    def add(kind, r):
        rows.append(_f32(r))
        kinds.append(kind)

    z = {False: np.float32(0.0), True: np.float32(-0.0)}
    # the ties: +-eps32 in each position, the other three +0 or -0 (sqrt(fl(e e)) == e: the fp32 norm IS eps32)
    for pos in range(4):
        for sign in (1.0, -1.0):
            for neg in (False, True):
                r = np.full(4, z[neg], np.float32)
                r[pos] = np.float32(sign) * EPS32
                add("tie", r)
    # one ulp either side of it, axis-aligned (exact norms again): below - clamped; above - projected
    below, above = np.nextafter(EPS32, np.float32(0)), np.nextafter(EPS32, np.float32(1))
    for pos in range(4):
        for e, kind in ((below, "below"), (above, "above")):
            r = np.zeros(4, np.float32)
            r[pos] = e if pos % 2 == 0 else -e
            add(kind, r)
    # the clamped branch: 1e-13; 1e-20 (the squares are subnormal); 1e-30 (they underflow); the zero quaternion
    for n in (1e-13, 1e-20, 1e-30):
        for _ in range(2):
            d = g.standard_normal(4)
            add("clamped", d / np.linalg.norm(d) * n)
    add("clamped", np.zeros(4))
    add("clamped", [0.0, -0.0, 0.0, -0.0])
    # the projected branch at the ends of its range and in the middle
    for n in (1e18, 1e-6, 1e-11):
        for _ in range(2):
            d = g.standard_normal(4)
            add("projected", d / np.linalg.norm(d) * n)
    add("projected", [1.0, 0.0, 0.0, 0.0])
    for _ in range(4):
        d = g.standard_normal(4)
        add("projected", d / np.linalg.norm(d))
    for _ in range(8):
        add("projected", g.standard_normal(4))
    for _ in range(4):
        add("projected", g.standard_normal(4) * 1e-3)
    return np.stack(rows), np.array(kinds)


ROTATIONS, ROTATION_KINDS = _rotations()
_mag = [1e-8, 1.0, 5.0, 10.0, 16.6, 17.5, 30.0, 87.0, 88.0, 89.5, 104.0, 1e4, np.inf]
OPACITIES = _f32([0.0] + [s * m for m in _mag for s in (1.0, -1.0)] + [np.nan])
SCALINGS = _f32([-104.0, -88.0, -20.0, -7.0, -3.0, 0.0, 1.5, 10.0, 88.0, 89.5])
# cotangents: N(0,1), exact 0 and -0, 1e30, 1e-30 (signs of the last two drawn)
COTANGENT_KINDS = ("normal", "normal", "zero", "normal", "big", "negzero", "tiny")


def _check_table():
    """the margins the bars lean on"""
    q = ROTATIONS.astype(np.float64)
    norm = np.sqrt((q * q).sum(1))
    axis = (ROTATIONS != 0).sum(1) == 1
    # axis-aligned rows: the fp32 norm is exact, so the branch is decided on the row's one entry in fp32 as in float64
    e = np.abs(ROTATIONS[axis]).max(1)
    assert np.array_equal(np.sqrt(e * e), e)
    assert set(ROTATION_KINDS[axis]) >= {"tie", "below", "above"} and np.all(norm[ROTATION_KINDS == "tie"] == EPS)
    # every other row: the fp32 norm (4 u) cannot land on the other side of eps32
    assert np.all(np.abs(norm[~axis] / EPS - 1.0) > 1e-6)
    assert np.all(np.isin(ROTATION_KINDS[~axis], ("clamped", "projected")))
    # fp32 squares overflow nowhere float64's do not
    assert float(np.abs(ROTATIONS).max()) <= 1e18
    assert len(ROTATIONS) % 7 != 0 and len(OPACITIES) % 5 != 0     # the cycles below are coprime
    # the overflow decision of expf is the reference's: nothing within 0.5 of ln(FLT_MAX)
    for t in (SCALINGS, OPACITIES[np.isfinite(OPACITIES)]):
        assert np.all(np.abs(np.abs(t.astype(np.float64)) - LN_FLT_MAX) > 0.5)


_check_table()


def views(flat, P):
    """the model's tensors as views into its flat buffer (xyz 3P, features 48P, opacity P, scaling 3P, rotation 4P): the
    rotation rows start at byte 220 P, 16-byte aligned only when P % 4 == 0"""
    out, off = [], 0
    for w in WIDTHS:
        out.append(flat[off:off + P * w].reshape(P, w))
        off += P * w
    assert off == flat.shape[0]
    return dict(zip(("xyz", "features", "opacity", "scaling", "rotation"), out))


def _cotangent(g, kinds, shape_tail):
    n = len(kinds)
    out = g.standard_normal((n,) + shape_tail).astype(np.float32)
    sign = np.where(g.random((n,) + shape_tail) < 0.5, np.float32(-1), np.float32(1))
    for kind, value in (("zero", 0.0), ("negzero", -0.0), ("big", 1e30), ("tiny", 1e-30)):
        rows = kinds == kind
        out[rows] = np.float32(value) * (sign[rows] if kind in ("big", "tiny") else np.float32(1))
    return out


_CASES = {}


def cases(P):
    """P rows of the table -> dict(flat [59 P] fp32 with the rows in the model's order, g_scales [P,3], g_rot [P,4],
    g_opac [P,1], kind [P] (the rotation row's branch)).  Built once per P; treat as read-only."""
    if P in _CASES:
        return _CASES[P]
    g = np.random.default_rng(1000 + P)
    flat = g.standard_normal(59 * P).astype(np.float32)
    t = views(flat, P)
    i = np.arange(P)
    t["rotation"][:] = ROTATIONS[i % len(ROTATIONS)]
    t["opacity"][:, 0] = OPACITIES[i % len(OPACITIES)]
    e = np.arange(3 * P)
    t["scaling"][:] = SCALINGS[e % len(SCALINGS)].reshape(P, 3)
    ck = np.array(COTANGENT_KINDS)
    c = dict(flat=flat, kind=ROTATION_KINDS[i % len(ROTATIONS)],
             g_scales=_cotangent(g, ck[e % 7], ()).reshape(P, 3),
             g_rot=_cotangent(g, ck[i % 7], (4,)),
             g_opac=_cotangent(g, ck[(i % 5) + 2], (1,)))      # period 5: zero, normal, big, negzero, tiny
    ref = restate(t["scaling"], t["rotation"], t["opacity"], c["g_scales"], c["g_rot"], c["g_opac"])
    bar = bars(t["scaling"], t["rotation"], t["opacity"], c["g_scales"], c["g_rot"], c["g_opac"], ref)
    # the overflow decision is the reference's: no finite reference within its bar of the threshold
    for k in OUTPUTS:
        r = np.abs(ref[k])
        near = np.isfinite(r) & (np.abs(r - TO_INF) <= np.maximum(bar[k], FLT_MIN) + 2.0 ** 104)
        assert not near.any(), (P, k)
    for a in c.values():
        a.setflags(write=False)
    c.update(ref=ref, bar=bar)
    _CASES[P] = c
    return c


def restate(scaling, rotation, opacity, g_scales, g_rot, g_opac):
    """float64 from the fp32 inputs -> dict of OUTPUTS, plus `projected` [P] (the rotation row's branch: |q| >= eps32)"""
    x, q, o = (np.asarray(t, np.float32).astype(np.float64) for t in (scaling, rotation, opacity))
    gs, gr, go = (np.asarray(t, np.float32).astype(np.float64) for t in (g_scales, g_rot, g_opac))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ex = np.exp(x)
        norm = np.sqrt((q * q).sum(1, keepdims=True))
        projected = norm >= EPS
        v = q / np.maximum(norm, EPS)
        s, one_minus_s = 1.0 / (1.0 + np.exp(-o)), 1.0 / (1.0 + np.exp(o))
        d_proj = (gr - v * (v * gr).sum(1, keepdims=True)) / np.where(projected, norm, 1.0)
        d_rot = np.where(projected, d_proj, gr / EPS)
        # exp's backward is grad * RESULT, and the result is an fp32 number: where it overflowed, 0 * inf is NaN in torch too
        result = np.where(ex >= TO_INF, np.inf, ex)
        out = dict(scales=ex, v=v, opacity=s, d_scaling=gs * result, d_rotation=d_rot, d_opacity=go * s * one_minus_s)
    out["projected"] = projected[:, 0]
    return out


def bars(scaling, rotation, opacity, g_scales, g_rot, g_opac, ref):
    """per element, float64 (the module docstring derives them).  Rows of the clamped branch get 0 for v and d_rotation:
    check() compares their bits."""
    q = np.asarray(rotation, np.float32).astype(np.float64)
    gs, gr, go = (np.abs(np.asarray(t, np.float32).astype(np.float64)) for t in (g_scales, g_rot, g_opac))
    E = EXPF_E
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        ex, s = ref["scales"], ref["opacity"]
        d_ex = np.where(ex >= FLT_MIN, E * U * ex, FLT_MIN)
        d_s = np.where(s >= FLT_MIN, (E + 2) * U * s, FLT_MIN)
        one_minus_s = 1.0 / (1.0 + np.exp(np.asarray(opacity, np.float32).astype(np.float64)))
        norm = np.sqrt((q * q).sum(1, keepdims=True))
        proj = ref["projected"][:, None]
        v = np.abs(ref["v"])
        contrib = (gr + v * (v * gr).sum(1, keepdims=True)) / np.where(proj, norm, 1.0)
        out = dict(scales=E * U * np.abs(ex),
                   d_scaling=gs * d_ex + U * np.abs(ref["d_scaling"]),
                   opacity=(E + 2) * U * np.abs(s),
                   d_opacity=go * (np.abs(1.0 - 2.0 * s) * d_s + 3 * U * s * one_minus_s),
                   v=np.where(proj, 4 * U * v, 0.0),
                   d_rotation=np.where(proj, 24 * U * contrib, 0.0))
    return out


def check(name, got, ref, bar, exact_rows=None, bits=True):
    """`got` (fp32) against the float64 `ref` within `bar` per element (floor FLT_MIN); rows of `exact_rows` bit for bit
    against float32(ref) (bits=False: equal as numbers, the sign of a zero left open); inf and NaN exactly where float32(ref)
    has them.  -> the largest distance / bar over the finite
    elements held to a bar (for the reports)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        ref32 = ref.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(ref32)), "%s: NaN at other places than the reference's" % name
    inf = np.isinf(ref32)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], ref32[inf]), "%s: inf at other places" % name
    exact = np.zeros(ref.shape, bool)
    if exact_rows is not None:
        exact[exact_rows] = True
    same = got.view(np.int32)[exact] == ref32.view(np.int32)[exact] if bits else got[exact] == ref32[exact]
    assert same.all(), "%s: %d elements of the clamped branch are not the one division's bits" % (name, int((~same).sum()))
    held = np.isfinite(ref32) & ~exact
    dist = np.abs(got[held].astype(np.float64) - ref[held])
    b = np.maximum(bar[held], FLT_MIN)
    worst = float((dist / b).max()) if dist.size else 0.0
    if worst > 1.0:
        k = int(np.argmax(dist / b))
        raise AssertionError("%s: %.3f of its bar (got %r, reference %r, bar %.3e, %d elements over)"
                             % (name, worst, got[held][k], ref[held][k], b[k], int((dist > b).sum())))
    return worst


def check_all(got, c, what="", bits=True):
    """got: dict of OUTPUTS (fp32 arrays) against cases(P) or any dict with ref / bar -> {output: worst distance / bar}"""
    clamped = ~c["ref"]["projected"]
    return {k: check(what + k, got[k], c["ref"][k], c["bar"][k], clamped if k in ("v", "d_rotation") else None, bits)
            for k in OUTPUTS}
