"""Restatements for the evaluation from files (gsplat_amd/imageio.py, gsplat_amd/render_set.py, csrc/gs_eval_files.hip), numpy
only: the arbiter of the GPU tests, which may import neither Pillow nor scipy.

SSIM_sk = skimage.metrics.structural_similarity(a, b, channel_axis=2, data_range=1.0), defaults otherwise, from its
documented algorithm (skimage itself is not a dependency of the tests).  Per channel:
  7 x 7 box means ux, uy, uxx, uyy, uxy;  v_ab = 49/48 (u_ab - u_a u_b)            (use_sample_covariance)
  S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = 1
  the mean of S (float64) over the map with a 3-pixel border cropped away = over the windows wholly inside the image
then the mean over the channels.
  ssim_sk_f64     the direct form: every window's 49 values added in float64
  ssim_sk_f32     the chain skimage runs on the reference's float32 arrays: scipy.ndimage.uniform_filter axis by axis (a
                  float64 sum of 7, divided by 7, stored as float32 after each axis), then float32 arithmetic, the final mean
                  in float64.  Its distance from ssim_sk_f64 on a case is the reference's own rounding: the GPU tests' bar.
  ssim_sk_scipy   the same chain through scipy itself (CPU tests, where scipy imports), in either precision

The resize fixture's inputs (tests/golden/pil_resize.npz holds their CRC32 and Pillow's answers): seeded_u8 and content_u8."""
import zlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

WIN = 7
K1, K2, R = 0.01, 0.03, 1.0
C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)


def _check(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 3, (a.shape, b.shape)
    if a.shape[1] < WIN or a.shape[2] < WIN:
        raise ValueError("win_size exceeds image extent: %s" % (a.shape,))   # as skimage raises
    return a, b


def _s_map(ux, uy, uxx, uyy, uxy, c1, c2, cov_norm):
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    A1, A2, B1, B2 = 2 * ux * uy + c1, 2 * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    return (A1 * A2) / (B1 * B2)


def ssim_sk_f64(a, b):
    """[C,H,W] arrays (any float type; promoted) -> python float"""
    a, b = _check(a, b)
    vals = []
    for x, y in zip(a.astype(np.float64), b.astype(np.float64)):
        box = lambda t: sliding_window_view(t, (WIN, WIN)).sum(axis=(-1, -2)) / (WIN * WIN)  # noqa: E731
        S = _s_map(box(x), box(y), box(x * x), box(y * y), box(x * y), C1, C2, COV_NORM)
        vals.append(S.mean(dtype=np.float64))
    return float(np.mean(np.array(vals, dtype=np.float64)))


def _box32(t):
    """uniform_filter of a float32 image, valid part: per axis a float64 mean of 7 stored as float32"""
    assert t.dtype == np.float32
    rows = (sliding_window_view(t.astype(np.float64), WIN, axis=0).sum(axis=-1) / WIN).astype(np.float32)
    return (sliding_window_view(rows.astype(np.float64), WIN, axis=1).sum(axis=-1) / WIN).astype(np.float32)


def ssim_sk_f32(a, b):
    """[C,H,W] float32 arrays -> python float: the float32 chain"""
    a, b = _check(a, b)
    assert a.dtype == np.float32 and b.dtype == np.float32
    c1, c2, cn = np.float32(C1), np.float32(C2), np.float32(COV_NORM)
    vals = []
    for x, y in zip(a, b):
        S = _s_map(_box32(x), _box32(y), _box32(x * x), _box32(y * y), _box32(x * y), c1, c2, cn)
        assert S.dtype == np.float32
        vals.append(S.mean(dtype=np.float64))
    return float(np.mean(np.array(vals, dtype=np.float64)))


def ssim_sk_scipy(a, b, dtype):
    """The chain as skimage writes it, through scipy.ndimage.uniform_filter (default border mode) and the 3-pixel crop"""
    from scipy.ndimage import uniform_filter
    a, b = _check(a, b)
    vals = []
    for x, y in zip(a.astype(dtype), b.astype(dtype)):
        f = lambda t: uniform_filter(t, size=WIN)  # noqa: E731
        S = _s_map(f(x), f(y), f(x * x), f(y * y), f(x * y), dtype(C1), dtype(C2), dtype(COV_NORM))
        vals.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(np.array(vals, dtype=np.float64)))


# ------------------------------------------------------------------------------- the SSIM_sk cases of the GPU tests
# 38 = 32 windows + 6: the last size one tile of windows covers; 39 needs a second tile along that axis
SK_SIZES = [(7, 7), (7, 8), (8, 7), (9, 9), (33, 40), (38, 38), (39, 39), (38, 39), (39, 38), (71, 70)]
SK_CHANNELS = [1, 3, 4]
SK_FLAGS = {"none": (False, False, False), "clamp": (True, False, False), "quantise": (False, True, False),
            "masked": (False, False, True), "all": (True, True, True)}   # (clamp, quantise, masked)
SK_FLOOR = 1e-12


def sk_case_key(Cn, H, W, form):
    return "%dx%dx%d_%s" % (Cn, H, W, form)


# ----------------------------------------------------------------------------------------------- the resize fixture
# (H, W) -> (H2, W2); mode L and RGB each
SIZE_CASES = [((8, 8), (2, 2)), ((5, 4), (1, 1)), ((13, 29), (3, 7)), ((37, 64), (9, 16)), ((75, 101), (18, 25)),
              ((300, 400), (75, 100)), ((300, 400), (77, 133)), ((300, 400), (300, 400)),
              ((37, 64), (37, 16)), ((37, 64), (9, 64))]   # the last two: one axis changes
CONTENT_SIZES = [((37, 64), (9, 16)), ((300, 400), (75, 100)), ((12, 10), (30, 27))]   # the last: an upscale
CONTENTS = ("zeros", "full", "checker1", "checker3", "masklike")


def seeded_u8(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, C), dtype=np.uint8)


def content_u8(kind, H, W, C):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "zeros":
        img = np.zeros((H, W), dtype=np.uint8)
    elif kind == "full":
        img = np.full((H, W), 255, dtype=np.uint8)
    elif kind == "checker1":
        img = (((x + y) & 1) * 255).astype(np.uint8)
    elif kind == "checker3":    # the negative lobes overshoot both ways: the clamp decides
        img = ((((x // 3) + (y // 3)) & 1) * 255).astype(np.uint8)
    elif kind == "masklike":    # large flat areas, sharp edges
        disc = ((y - 0.45 * H) ** 2 + (x - 0.55 * W) ** 2) < (0.3 * min(H, W)) ** 2
        bar = (x > 0.1 * W) & (x < 0.2 * W) & (y > 0.2 * H)
        img = ((disc | bar) * 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.repeat(img[:, :, None], C, axis=2))


def fixture_cases():
    """-> [(key, maker of the input, (H, W), (H2, W2), C)] in the generator's order"""
    out = []
    for i, ((H, W), (H2, W2)) in enumerate(SIZE_CASES):
        for C in (1, 3):
            key = "rand_%dx%d_%dx%d_c%d" % (H, W, H2, W2, C)
            out.append((key, (lambda H=H, W=W, C=C, s=1000 + 10 * i + C: seeded_u8(H, W, C, s)), (H, W), (H2, W2), C))
    for (H, W), (H2, W2) in CONTENT_SIZES:
        for kind in CONTENTS:
            # (a content image's channels are equal by construction: at 300 x 400 mode RGB would only store mode L three times)
            for C in ((1,) if H * W > 10000 else (1, 3)):
                key = "%s_%dx%d_%dx%d_c%d" % (kind, H, W, H2, W2, C)
                out.append((key, (lambda k=kind, H=H, W=W, C=C: content_u8(k, H, W, C)), (H, W), (H2, W2), C))
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF
