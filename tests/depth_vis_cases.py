"""The inputs of the coloured-depth tests (tests/golden/make_golden_paths.py, test_depth_vis_cpu.py, test_gpu_depth_vis.py):
the smallest shapes at which a radix select of two percentiles can go wrong.  Seeded; the fixture stores the arrays too and
the CPU test checks that both agree.

  name -> (depth float32 [H,W], alpha float32 [H,W] or None, rules)
Sizes (smooth positive depth with noise, no alpha): 1 x 1; 1 x 199 (the low query lies left of the first node); 1 x 200 (the low
query sits exactly on node 1); 1 x 201; 13 x 17; 257 x 3; 64 x 48 (the plain case, also with alpha); 160 x 128 (five
workgroups of the select).
Values (32 x 24 unless said): a constant image (with alpha: 0/0 under the composite, everything NaN; without alpha not under the
"dng" rule, where hi - lo is two float32 epsilons and the last bit of numpy's float32 logarithm decides every pixel - the
reference never colours such an image either: its "dng" path always composites first; the 1 x 1 image is such an image); two
values whose ties
span both wanted ranks of both queries; values that share their top 11 / top 22 / top 24 key bits; mixed signs with both
zeros (identity rule only: the other curves are singular there by design); one +inf; a few NaN; alpha of exactly 0 and 1."""
import numpy as np

RULES = ("identity", "dng", "fsgs")
SIZES = ((1, 1), (1, 199), (1, 200), (1, 201), (13, 17), (257, 3), (64, 48), (160, 128))


def smooth_depth(H, W, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 2.5 + 1.5 * np.sin(0.11 * x + 0.3) * np.cos(0.07 * y) + 0.9 * (y / max(H, 1)) + 0.05 * rng.randn(H, W)
    return np.maximum(d, 0.2).astype(np.float32)


def smooth_alpha(H, W, seed):
    rng = np.random.RandomState(seed)
    return np.clip(0.85 + 0.3 * rng.rand(H, W) - 0.2, 0.0, 1.0).astype(np.float32)


def key_bits(x):
    """The monotone 32-bit key of a float32 (the select's order: NaN last, -0 = +0)"""
    x = np.asarray(x, dtype=np.float32)
    u = np.where(x == 0, np.float32(0), x).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), np.uint32(0xFFFFFFFF), k)


def cases():
    out = {}
    for i, (H, W) in enumerate(SIZES):
        # (one pixel is a constant image: see below for why "dng" takes it through the composite only)
        out["size_%dx%d" % (H, W)] = (smooth_depth(H, W, 100 + i), None, RULES if H * W > 1 else ("identity", "fsgs"))
    out["size_1x1_alpha"] = (smooth_depth(1, 1, 100), np.full((1, 1), 0.75, dtype=np.float32), RULES)
    H, W = 32, 24
    n = H * W
    rng = np.random.RandomState(7)
    out["plain_alpha_64x48"] = (smooth_depth(64, 48, 106), smooth_alpha(64, 48, 206), RULES)
    out["const"] = (np.full((13, 17), 1.75, dtype=np.float32), None, ("identity", "fsgs"))
    out["const_alpha"] = (np.full((13, 17), 1.75, dtype=np.float32), smooth_alpha(13, 17, 207), RULES)
    two = np.where(rng.rand(H, W) < 0.5, np.float32(1.25), np.float32(3.5)).astype(np.float32)
    out["two_values"] = (two, None, RULES)
    # shared key bits: 2.0 + k ulp.  All share the top 11 bits; k < 1024 shares the top 22; k < 256 the top 24 (8-bit passes:
    # every pass but the last sees one digit).  2 % of the pixels lie far off on one side, so that one query's ranks fall among
    # them and the other's inside the shared prefix: the bounds stay apart by more than float32's resolution of the curve
    base = np.float32(2.0).view(np.uint32)
    far = n // 50
    k = rng.randint(0, 1 << 20, size=n).astype(np.uint32)
    k[: n // 2] = rng.randint(0, 1024, size=n // 2)
    k[: n // 4] = rng.randint(0, 256, size=n // 4)
    sb = (base + k).astype(np.uint32).view(np.float32)
    sb[-far:] = (0.4 + 0.2 * rng.rand(far)).astype(np.float32)          # below: the low query's ranks
    out["shared_bits"] = (rng.permutation(sb).reshape(H, W), None, RULES)
    low = (base + rng.randint(0, 256, size=n).astype(np.uint32)).astype(np.uint32).view(np.float32)
    low[-far:] = (7.0 + 2.0 * rng.rand(far)).astype(np.float32)         # above: the high query's ranks
    out["shared_top24"] = (rng.permutation(low).reshape(H, W), None, RULES)
    mixed = (rng.randn(H, W) * 2).astype(np.float32)
    flat = mixed.reshape(-1)
    flat[rng.choice(n, 60, replace=False)] = np.float32(0.0)
    flat[rng.choice(n, 60, replace=False)] = np.float32(-0.0)
    out["mixed_signs"] = (mixed, None, ("identity",))
    inf = smooth_depth(H, W, 108)
    inf[5, 7] = np.inf
    out["one_inf"] = (inf, None, RULES)
    nan = smooth_depth(H, W, 109)
    nan.reshape(-1)[[3, 77, 400]] = np.nan
    out["few_nan"] = (nan, None, RULES)
    a01 = smooth_alpha(H, W, 210)
    a01[:4] = 0.0
    a01[4:20] = 1.0
    out["alpha_0_1"] = (smooth_depth(H, W, 110), a01, RULES)
    return out


# ---- the "dng" rule's allowance: the reference takes numpy's float32 log of a pixel, the device the double logarithm rounded to
# float32 once.  Measured on every case image on the CPU (test_depth_vis_cpu.py re-measures): at most 3 ulp of the curve's value
# between the two.  Doubled:
LOG_ULP_MEASURED = 3
LOG_ULP_ALLOW = 2 * LOG_ULP_MEASURED
MAX_EXEMPT_FRACTION = 0.005
EPS32 = np.finfo(np.float32).eps


def log_ulp_error(x):
    """x float32 -> per finite pixel |numpy float32 -log(x + eps) - the float64 one rounded once| in ulp of the latter"""
    with np.errstate(all="ignore"):
        xe = x + EPS32
        v32 = -np.log(xe)
        once = (-np.log(xe.astype(np.float64))).astype(np.float32)
        ok = np.isfinite(v32) & np.isfinite(once)
        return np.abs(v32[ok].astype(np.float64) - once[ok].astype(np.float64)) / np.spacing(np.abs(once[ok])).astype(np.float64)


def dng_exempt(x, v, lo, hi):
    """The pixels of a "dng" case that may take a neighbouring table row: 256 v within delta of an interior integer 1..255,
    delta = 256 * LOG_ULP_ALLOW * ulp(curve value) / |curve(hi) - curve(lo)|.  x: the coloured float32 image, v: the fixture's
    float64 normalised image, lo / hi: its bounds.  -> bool [H,W]"""
    with np.errstate(all="ignore"):
        curve = (-np.log((x + EPS32).astype(np.float64))).astype(np.float32)
        span = abs(-np.log(hi + EPS32) - -np.log(lo + EPS32))
        delta = 256.0 * LOG_ULP_ALLOW * np.spacing(np.abs(curve)).astype(np.float64) / span
        t = v * 256.0
        near = np.rint(t)
        return np.isfinite(delta) & (near >= 1) & (near <= 255) & (np.abs(t - near) <= delta)
