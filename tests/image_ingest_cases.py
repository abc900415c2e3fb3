"""The cases of tests/golden/pil_resize_alpha.npz (Pillow's Image.resize bytes for modes LA and RGBA), shared by the generator
tests/golden/make_golden_image_ingest.py, tests/test_image_ingest_cpu.py and tests/test_gpu_image_ingest.py.  No Pillow here.

Sizes are (H, W) -> (H2, W2):
  down on both axes 53x37 -> 26x19 (W2 odd: an LA row is then no whole number of words), up 16x16 -> 40x31, one axis unchanged
  each way (the horizontal pass alone, W2 even; the vertical pass alone from an even and from an odd width: with and without
  word loads for LA), the same size (a copy: no premultiply round trip), 1x1 -> 3x3, and 200 -> 3 on either axis (long runs).
Alpha contents, at the first two sizes: random, all 255, all 0, only the values 1 and 254 (the division's extremes), whole rows
and whole columns transparent; everywhere else random with a sprinkling of 0 and 255."""
import zlib

import numpy as np

SIZE_CASES = (((53, 37), (26, 19)), ((16, 16), (40, 31)), ((37, 53), (37, 26)), ((53, 26), (19, 26)), ((53, 37), (26, 37)),
              ((21, 17), (21, 17)), ((1, 1), (3, 3)), ((200, 9), (3, 9)), ((9, 200), (9, 3)))
CONTENT_SIZES = SIZE_CASES[:2]
ALPHAS = ("a255", "a0", "a1_254", "rows_cols")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def seeded(H, W, C, seed, alpha="random"):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    if alpha == "random":
        pick = rng.integers(0, 8, size=(H, W))
        img[:, :, -1][pick == 0] = 0
        img[:, :, -1][pick == 1] = 255
    elif alpha == "a255":
        img[:, :, -1] = 255
    elif alpha == "a0":
        img[:, :, -1] = 0
    elif alpha == "a1_254":
        img[:, :, -1] = np.where(rng.integers(0, 2, size=(H, W)) == 0, 1, 254)
    elif alpha == "rows_cols":
        img[::3, :, -1] = 0
        img[:, 1::4, -1] = 0
    else:
        raise ValueError(alpha)
    return img


def fixture_cases():
    """-> [(key, maker of the input, (H, W), (H2, W2), C)] in the generator's order"""
    out = []
    for i, ((H, W), (H2, W2)) in enumerate(SIZE_CASES):
        for C in (2, 4):
            key = "random_%dx%d_%dx%d_c%d" % (H, W, H2, W2, C)
            out.append((key, (lambda H=H, W=W, C=C, s=2000 + 10 * i + C: seeded(H, W, C, s)), (H, W), (H2, W2), C))
    for i, ((H, W), (H2, W2)) in enumerate(CONTENT_SIZES):
        for k, kind in enumerate(ALPHAS):
            for C in (2, 4):
                key = "%s_%dx%d_%dx%d_c%d" % (kind, H, W, H2, W2, C)
                out.append((key, (lambda H=H, W=W, C=C, kind=kind, s=3000 + 100 * i + 10 * k + C: seeded(H, W, C, s, kind)),
                            (H, W), (H2, W2), C))
    return out


def expected(z, key, a):
    """Pillow's bytes for the case: the recorded ones, or - the same size, where Pillow returns a copy - the input"""
    return np.ascontiguousarray(z[key + "_out"] if key + "_out" in z.files else a)
