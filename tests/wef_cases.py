"""Cases and bars for the Wavelet Error Field kernels (csrc/gs_wef.hip, gsplat_amd/wef.py), pure torch / numpy.  The fixture
generator (tests/golden/make_golden_wef.py), tests/test_wef_cpu.py and tests/test_gpu_wef.py all take their inputs from here.

Inputs.  gt = torch.rand from the case's seed, pred = gt + residual, both float32 [C,H,W]:
  "rand"    residual uniform in [-0.125, 0.125]; images of at least 32 x 32 also carry one impulse of amplitude 1 at (9, 10) in
            every channel: every band of both levels has its largest coefficient there (|band| = the bound A below), so no map
            of a large image is nearly flat and the combined field spans [0, 1]
  "same"    pred == gt: every map exactly 0
  "corner"  one non-zero residual pixel at (0, 0); "padded": one at (H - 1, W - 1) of an odd-sized image, the sample both
            levels repeat - the border clamps of the upsample
  "nan"     "rand" with one NaN pixel: every map NaN everywhere (amin / amax propagate it)
2 x 2 and 4 x 4 hold one level-2 coefficient: every level-2 plane is one number, every level-2 map exactly 0 = 0 / (0 + 1e-8)
(at 2 x 2 the level-1 planes as well).

The float64 twin of a case is gsplat_amd.wef.wef_maps_torch on the same inputs cast to float64 (held to the reference's own
float64 result by the fixture).  A map whose twin is flat before normalisation (max == min: a plane of one coefficient, or
bands that an image of one row or one column, or a repeated sample, makes exactly zero) must be exactly 0 in float32 as well
and has no bar.

Bar for one element of a map that is not flat, any evaluation order, first order in u = 2^-24.  b is a band coefficient, A the
same coefficient of the LL transform of |residual| (|b| <= A), both in float64:
  residual                1 rounding
  one Haar level          a band is a sum of four terms c * (c * a), each through 2 multiplies, 2 adds and twice the rounded
                          constant c: 6 u on sum |terms| = A
                          -> level 1: |db| <= k u A1, k = 7; level 2 (bands of LL1): k = 13 on A2 = LL(A1)
  square, scale           2 |b| |db| + u b^2 (the scale is a power of two)
  channel mean            C - 1 adds and a divide: C u on e
                          -> |de| <= u (2 k M + (C + 1) e_max),   M = max mean_c(scale |b_c| A_c), e_max = max e over the plane
  four-tap bilinear       weights are convex, so |de| passes through; 2 multiplies and 2 adds on a tap's path: 4 u e_max;
                          l0 = 1 - l1 rounds once per axis: 2 u e_max; the source index scale * (o + 0.5) - 0.5 carries 3
                          roundings of numbers below n_in, |dl1| <= 3 n_in u, and moves the value by dl1 times the difference
                          of two neighbours <= R = max e - min e:  3 (h_in + w_in) u R
                          -> |du| <= u (2 k M + (C + 7) e_max + 3 (h_in + w_in) R)
  normalisation           n = (x - min) / (max - min + 1e-8) in [0, 1]: to first order dn = (dx - n dmax - (1 - n) dmin) / D with
                          each of dx, dmin, dmax within |du|; the subtraction, the denominator's two operations, the divide: 4 u
                          -> bar = 2 |du| / D + 4 u,   D = max - min + 1e-8 of the twin's upsampled map
  combined field          |dc| <= mean_k(bar_k) + K u (K - 1 adds, a divide; flat maps add nothing), normalised again:
                          bar = 2 |dc| / D_c + 4 u
The bar is proportional to (energy scale) / (max - min + 1e-8) plus a few u, as it must be: a nearly flat map amplifies every
rounding.  tests/test_wef_cpu.py holds it to two conditions: the reference's own float32 result lies within it, and it is at
most 1e-3 on every map that is not flat."""
import functools
from collections import namedtuple

import torch

U = 2.0 ** -24
Case = namedtuple("Case", "name C H W kind seed")

CASES = (
    Case("one_coeff_2x2", 3, 2, 2, "rand", 11),
    Case("one_coeff_4x4", 3, 4, 4, "rand", 12),
    Case("row_1x9", 3, 1, 9, "rand", 13),
    Case("odd_5x7", 3, 5, 7, "rand", 14),
    Case("even_odd_6x9", 3, 6, 9, "rand", 15),
    Case("even_8x8", 3, 8, 8, "rand", 16),
    Case("odd_37x53", 3, 37, 53, "rand", 17),
    Case("same_5x7", 3, 5, 7, "same", 18),
    Case("corner_9x11", 3, 9, 11, "corner", 19),
    Case("padded_9x11", 3, 9, 11, "padded", 20),
    Case("nan_6x9", 3, 6, 9, "nan", 21),
    Case("wide_3x130", 3, 3, 130, "rand", 22),
    Case("aligned_64x96", 3, 64, 96, "rand", 23),
    Case("partials_70x300", 3, 70, 300, "rand", 24),
    Case("partials_270x480_c1", 1, 270, 480, "rand", 25),
    Case("partials_270x480_c4", 4, 270, 480, "rand", 26),
)
BY_NAME = {c.name: c for c in CASES}
FIXTURE_CASES = tuple(c for c in CASES if c.H <= 37 and c.W <= 53)   # what tests/golden/wef_maps.npz records
ALL_FLAT = (("one_coeff_2x2", False), ("one_coeff_2x2", True), ("one_coeff_4x4", False), ("same_5x7", False),
            ("same_5x7", True))                                      # (case, all bands): every map exactly 0
LEVEL2_KEYS = ("LL2", "LH2", "HL2", "WEF")
ALL_KEYS = ("LL1", "LH1", "HL1", "HH1", "LL2", "LH2", "HL2", "HH2", "COMBINED")
SCALE = {"LL1": 1.0, "LH1": 1.0, "HL1": 1.0, "HH1": 1.0, "LL2": 4.0, "LH2": 2.0, "HL2": 2.0, "HH2": 2.0}


def keys_of(all_bands):
    return ALL_KEYS if all_bands else LEVEL2_KEYS


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(c.seed)
    gt = torch.rand((c.C, c.H, c.W), generator=g)
    if c.kind == "same":
        return gt.clone(), gt
    if c.kind in ("corner", "padded"):
        pred = gt.clone()
        y, x = (0, 0) if c.kind == "corner" else (c.H - 1, c.W - 1)
        pred[1, y, x] = pred[1, y, x] + 0.5
        return pred, gt
    res = (torch.rand((c.C, c.H, c.W), generator=g) - 0.5) * 0.25
    if c.H >= 32 and c.W >= 32:
        res[:, 9, 10] = 1.0
    pred = gt + res
    if c.kind == "nan":
        pred[1, 2, 3] = float("nan")
    return pred, gt


def inputs(case):
    """-> (pred, gt) float32 [C,H,W] (fresh copies)"""
    pred, gt = _inputs(case.name if isinstance(case, Case) else case)
    return pred.clone(), gt.clone()


@functools.lru_cache(maxsize=None)
def _twin(name, all_bands):
    from gsplat_amd import wef
    pred, gt = (t.double() for t in _inputs(name))
    keys = keys_of(all_bands)[:-1]
    return wef.wef_maps_torch(pred, gt, all_bands), wef.upsampled_energies(pred, gt, keys)


def twin(case, all_bands):
    """-> the float64 maps {key: [1,1,H,W]} (shared, read-only)"""
    return _twin(case.name, bool(all_bands))[0]


@functools.lru_cache(maxsize=None)
def _bars(name, all_bands):
    from gsplat_amd import wef
    c = BY_NAME[name]
    pred, gt = (t.double() for t in _inputs(name))
    maps, ups = _twin(name, all_bands)
    a1 = wef.haar_level((pred - gt).abs())[0]
    a2 = wef.haar_level(a1)[0]
    bands = wef.residual_bands(pred, gt)
    keys = keys_of(all_bands)
    out, acc = {}, 0.0
    for k in keys[:-1]:
        level2 = k.endswith("2")
        a, b = (a2 if level2 else a1), bands[k]
        u = ups[k]
        mn, mx = float(u.min()), float(u.max())
        if mx == mn:
            out[k] = None            # flat: exactly 0, no bar
            continue
        e = (SCALE[k] * b * b).mean(dim=0)
        M = float((SCALE[k] * b.abs() * a).mean(dim=0).max())
        e_max, R = float(e.max()), float(e.max() - e.min())
        du = U * (2 * (13 if level2 else 7) * M + (c.C + 7) * e_max + 3 * (a.shape[-2] + a.shape[-1]) * R)
        out[k] = 2 * du / (mx - mn + 1e-8) + 4 * U
        acc += out[k]
    K = len(keys) - 1
    comb = None
    for k in keys[:-1]:
        comb = maps[k] if comb is None else comb + maps[k]
    comb = comb / float(K)
    mn, mx = float(comb.min()), float(comb.max())
    out[keys[-1]] = None if mx == mn else 2 * (acc / K + K * U) / (mx - mn + 1e-8) + 4 * U
    return out


def bars(case, all_bands):
    """-> {key: bar, or None for a map that is flat before its normalisation (it must be exactly 0)}; not for "nan" cases"""
    return _bars(case.name, bool(all_bands))


def check_maps(case, all_bands, got, what):
    """got {key: tensor of H * W elements} against the twin -> {key: largest distance}; asserts the bars, the exact zeros and
    the NaN pattern"""
    dist = {}
    tw = twin(case, all_bands)
    for k in keys_of(all_bands):
        g = got[k].detach().cpu().double().reshape(case.H, case.W)
        if case.kind == "nan":
            assert bool(torch.isnan(g).all()), "%s %s %s: NaN everywhere expected" % (what, case.name, k)
            continue
        bar = bars(case, all_bands)[k]
        if bar is None:
            assert bool((g == 0).all()), "%s %s %s: exactly 0 expected" % (what, case.name, k)
            dist[k] = 0.0
            continue
        dist[k] = float((g - tw[k].reshape(case.H, case.W)).abs().max())
        assert dist[k] <= bar, "%s %s %s: %.3e from float64, bar %.3e" % (what, case.name, k, dist[k], bar)
    return dist
