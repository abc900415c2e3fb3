"""A float64 restatement of three per-Gaussian pieces of a DNGaussian training step, written from their formulas:

  regulariser   mx_i, mn_i = row max / min of scaling [P,3]; H = {o_i > 0.2}, L = {o_i < 0.2}
                shape = mean mx / mn, scale = mean mx^2, opa = 1 - mean_H o^2 + mean_L (1 - o)^2, total = w . (shape, scale, opa)
  view_dirs     n_i = (x_i - c) / |x_i - c|
  near_mask     m_i = OR_k |x_i - c_k| < near

each as a COMPOSITION torch autograd differentiates, and the regulariser and the directions also in CLOSED FORM: the gradient
every kernel evaluates, with, per gradient element, its SCALE - the sum of the absolute values of the contributions added into
that element (two or three for a scaling entry that is a row's max and min at once, one for an opacity, four for a direction).
A structurally zero element has scale 0.  0.2 is the fp32 0.2 an fp32 opacity is compared with."""
import math

import torch

F64 = torch.float64
THRESHOLD = float(torch.tensor(0.2, dtype=torch.float32))
WEIGHTS = (0.001, 0.001, 0.01)
LOGIT_THRESHOLD = math.log(THRESHOLD / (1.0 - THRESHOLD))


# ---- compositions (for autograd) ----
def terms(scaling, opacity):
    """-> [3] = shape, scale, opa.  An empty H or L gives NaN (the mean of nothing)."""
    o = opacity.reshape(-1)
    mx, mn = scaling.max(dim=1).values, scaling.min(dim=1).values
    shape = (mx / mn).sum() / scaling.shape[0]
    scale = (mx ** 2).sum() / scaling.shape[0]
    hi, lo = o > THRESHOLD, o < THRESHOLD
    opa = 1 - (o[hi] ** 2).sum() / int(hi.sum()) + ((1 - o[lo]) ** 2).sum() / int(lo.sum())
    return torch.stack((shape, scale, opa))


def terms_raw(raw_scaling, raw_opacity):
    return terms(torch.exp(raw_scaling), torch.sigmoid(raw_opacity))


def total(t, weights=WEIGHTS):
    return (t * torch.tensor(weights, dtype=t.dtype)).sum()


def view_dirs(xyz, campos):
    d = xyz - campos.reshape(1, 3)
    return d / d.norm(dim=1, keepdim=True)


def near_mask(xyz, centers, near):
    """-> (bool [P], the smallest | |x_i - c_k| - near | / near over all pairs)."""
    dist = (xyz.to(F64)[:, None, :] - centers.to(F64)[None, :, :]).norm(dim=2)
    return (dist < near).any(dim=1), float(((dist - near).abs() / near).min())


# ---- closed forms ----
def _arg(s, greater):
    """Column of the row max (min); a tie goes to the lowest column."""
    idx = torch.zeros(s.shape[0], dtype=torch.long)
    best = s[:, 0].clone()
    for c in (1, 2):
        better = s[:, c] > best if greater else s[:, c] < best
        idx[better] = c
        best = torch.where(better, s[:, c], best)
    return idx


def regulariser_closed(scaling, opacity, c, raw=False):
    """c [3] = dL/d(shape, scale, opa) -> dict(terms [3], g_scaling [P,3], g_scaling_scale, g_opacity (opacity's shape),
    g_opacity_scale).  raw: the inputs are the raw rows, the gradients are with respect to them."""
    s, o = scaling.to(F64), opacity.to(F64).reshape(-1)
    c = [float(v) for v in c]
    P = s.shape[0]
    amax, amin = _arg(s, True), _arg(s, False)
    if raw:
        s, om, o = torch.exp(s), torch.sigmoid(-o), torch.sigmoid(o)
    else:
        om = 1 - o
    rows = torch.arange(P)
    mx, mn = s[rows, amax], s[rows, amin]
    hi, lo = o > THRESHOLD, o < THRESHOLD
    n_hi, n_lo = int(hi.sum()), int(lo.sum())
    nan = torch.tensor(float("nan"), dtype=F64)
    t = torch.stack(((mx / mn).sum() / P, (mx ** 2).sum() / P,
                     1 - ((o[hi] ** 2).sum() / n_hi if n_hi else nan) + ((om[lo] ** 2).sum() / n_lo if n_lo else nan)))
    at_max = [c[0] / (P * mn), c[1] * 2 * mx / P]
    at_min = [-c[0] * mx / (P * mn ** 2)]
    if raw:
        at_max = [v * mx for v in at_max]
        at_min = [v * mn for v in at_min]
    gs, gs_scale = torch.zeros((P, 3), dtype=F64), torch.zeros((P, 3), dtype=F64)
    for where, parts in ((amax, at_max), (amin, at_min)):
        for v in parts:
            gs[rows, where] += v
            gs_scale[rows, where] += v.abs()
    go = torch.zeros(P, dtype=F64)
    if n_hi:
        go[hi] = -2 * c[2] * o[hi] / n_hi
    if n_lo:
        go[lo] = -2 * c[2] * om[lo] / n_lo
    if raw:
        go = go * o * om
    return dict(terms=t, g_scaling=gs, g_scaling_scale=gs_scale, g_opacity=go.reshape(opacity.shape),
                g_opacity_scale=go.abs().reshape(opacity.shape))


def coefficients(g_terms=None, g_total=None, weights=WEIGHTS):
    """dL/d(shape, scale, opa) from a gradient on the terms and one on the total, which fans out through the weights."""
    return [(0.0 if g_terms is None else float(g_terms[k])) + (0.0 if g_total is None else float(g_total) * weights[k])
            for k in range(3)]


def view_dirs_closed(xyz, campos, g):
    """-> dict(out [P,3], g_xyz, g_xyz_scale): (g - n (n . g)) / |x - c|."""
    d = xyz.to(F64) - campos.to(F64).reshape(1, 3)
    r = d.norm(dim=1, keepdim=True)
    n = d / r
    g = g.to(F64)
    gx = (g - n * (n * g).sum(dim=1, keepdim=True)) / r
    scale = (g.abs() + n.abs() * (n.abs() * g.abs()).sum(dim=1, keepdim=True)) / r
    return dict(out=n, g_xyz=gx, g_xyz_scale=scale)


# ---- inputs: float64 tensors holding fp32 numbers ----
def _f32(t):
    return t.float().to(F64)


def scene(P, kind="mixed", seed=0, raw=False):
    """(scaling [P,3], opacity [P]) - activated, or raw when `raw`.  Rows cycle through: all three scales tied, the max in
    column 0 / 1 / 2 with the other two tied, the min in column 0 / 1 / 2 with the other two tied, all distinct.  Opacities:
    'mixed' both sides of 0.2 (activated: every seventh exactly 0.2), 'H_empty' all below, 'L_empty' all above.  Raw opacities
    keep sigmoid 1.6e-3 away from 0.2: membership must not hang on the device's sigmoid."""
    g = torch.Generator().manual_seed(seed * 7919 + P)
    base = torch.rand((P, 1), generator=g, dtype=F64) * 1.5 + 0.05
    s = base * (1 + torch.rand((P, 3), generator=g, dtype=F64))
    for i in range(P):
        case = i % 8
        if case == 0:
            s[i] = base[i]
        elif case <= 3:
            s[i] = base[i]
            s[i, case - 1] = base[i, 0] * 1.75
        elif case <= 6:
            s[i] = base[i] * 1.5
            s[i, case - 4] = base[i, 0]
    u = torch.rand(P, generator=g, dtype=F64)
    if kind == "H_empty":
        o = 0.001 + 0.198 * u
    elif kind == "L_empty":
        o = 0.201 + 0.798 * u
    else:
        o = 0.001 + 0.998 * u
        o[1::2] = 0.001 + 0.19 * u[1::2]   # both sets are populated from P = 2 on
        if P > 1:
            o[0] = 0.9
    s, o = _f32(s), _f32(o)
    if not raw:
        if kind == "mixed":
            o[6::7] = THRESHOLD
        return s, o
    rs, ro = _f32(torch.log(s)), _f32(torch.log(o / (1 - o)))
    for i in range(P):           # the float32 rounding of log may have split a tie: restore the pattern on the raw values
        case = i % 8
        if case == 0:
            rs[i] = float(rs[i, 0])
        elif case <= 3:
            rs[i, [c for c in range(3) if c != case - 1]] = float(rs[i, case % 3])
        elif case <= 6:
            rs[i, [c for c in range(3) if c != case - 4]] = float(rs[i, (case - 3) % 3])
    close = (ro - LOGIT_THRESHOLD).abs() < 0.01
    away = torch.where(ro < LOGIT_THRESHOLD, LOGIT_THRESHOLD - 0.02, LOGIT_THRESHOLD + 0.02)   # on its own side
    ro[close] = _f32(away)[close]
    return rs, ro


def points(P, K, near=0.5, seed=0):
    """(xyz [P,3], centers [K,3], campos [3]) for the directions and the mask.  Row P - 1 lies within `near` of the LAST centre
    alone, row 0 (P > 1) of none, every other row sits 0.3 or 0.8 from one of the centres, the rest are spread over a cube; every distance keeps
    1e-4 relative away from `near` (tests assert 1e-5 before they compare)."""
    g = torch.Generator().manual_seed(seed * 104729 + 31 * P + K)
    centers = torch.rand((K, 3), generator=g, dtype=F64) * 4 - 2
    centers[K - 1] = torch.tensor([9.0, 9.0, 9.0], dtype=F64)   # far from the others' cube
    xyz = torch.rand((P, 3), generator=g, dtype=F64) * 5 - 2.5
    d = torch.randn((P, 3), generator=g, dtype=F64)
    d = d / d.norm(dim=1, keepdim=True)
    for i in range(1, P - 1, 2):   # every other row sits 0.3 or 0.8 from one of the centres
        xyz[i] = centers[(i // 2) % K] + d[i] * (0.3 if i % 4 == 1 else 0.8)
    xyz[P - 1] = centers[K - 1] + torch.tensor([0.1, -0.2, 0.05], dtype=F64)
    if P > 1:
        xyz[0] = torch.tensor([-30.0, 20.0, 10.0], dtype=F64)
    xyz, centers = _f32(xyz), _f32(centers)
    for _ in range(8):
        dist = (xyz[:, None, :] - centers[None, :, :]).norm(dim=2)
        bad = (((dist - near).abs() / near) < 1e-4).any(dim=1)
        if not bool(bad.any()):
            break
        xyz[bad] = _f32(xyz[bad] * 1.01 + 0.003)
    return xyz, centers, centers[0].clone()
