"""The case table of the depth-prior tests (tests/test_depth_priors_cpu.py, tests/test_gpu_depth_priors.py): COLMAP-like
scenes for depth_scales and source maps for prepare_invdepth, each built for one edge of the statements.  The CPU test proves
every `expect` entry on the twin before the case is used.

Bars (u = 2^-53 for the fit's float64 sums, v = 2^-24 for the camera's float32 map):

depth_scales, device against the twin's float64 form.  n_valid, both medians and the gate's zero answers are exact: integer
counts, the bits of selected elements, IEEE operations in the same order.  A mean absolute deviation is sum(t_i) / n over the
same n non-negative terms (|inv - t_colmap| in float64; |float32(mono - t_mono)| widened).  The twin sums them exactly and
rounds twice (the sum, the division); the device adds them in a fixed order of its own.  Any order of n - 1 rounded additions
is within (n - 1) u of the exact sum, relative, because the terms share a sign; with the division's u and the twin's two:
    |dev_device - dev_twin| <= (n + 2) u dev_twin                                                      DEV_REL(n)
    scale = s_colmap / s_mono:       relative 2 DEV_REL(n) + u  (both deviations, the quotient's rounding)   SCALE_REL(n)
    offset = t_colmap - t_mono scale: absolute |t_mono scale| (SCALE_REL(n) + u) + |offset| u               offset_bar
A non-finite answer (one observation at z = +0) must be the same non-finite value.
The host path's mono deviation is numpy's float32 mean; against the float64 form it is held to the any-order float32 bound
n v (relative, one more for the division), and the measured distance is recorded: the origin of "s_mono differs" between the
host path and the device.

prepare_invdepth against the float64 twin.  The source / divisor is exact (65536, 512).  With M = max |source| / divisor:
a row sample a0 S0 + a1 S1 rounds a0 = 1 - fx, two products and a sum - each product's operand chain is at most 2 v, the sum one
more: 3 v M (a0 + a1 = 1, S of one sign).  The column pass does the same to values that already carry 3 v: 6 v M.  Scaling by
float32(scale) adds one rounding, the offset one on the sum: every pixel within
    8 v (M |float32(scale)| + |float32(offset)|)           (scale 1, offset 0 where nothing is applied)     prepare_bar
Exact cases (bar 0): equal sizes (a copy), and an exact halving of even sizes of uint16 samples without a scale (weights 1/2:
sums of two 17-bit values).  The mask plane is always exact.
"""
import collections
import math

import numpy as np

from gsplat_amd import io as gio

U, V = 2.0 ** -53, 2.0 ** -24
IDENT = (1.0, 0.0, 0.0, 0.0)
GENERAL_Q = np.array([0.9, 0.2, -0.3, 0.1]) / np.linalg.norm([0.9, 0.2, -0.3, 0.1])
GENERAL_T = (0.3, -0.2, 0.7)
WIDTH, HEIGHT = 64, 48

ScaleCase = collections.namedtuple("ScaleCase", ["name", "images", "cams", "xyz", "ids", "maps", "expect"])
PrepareCase = collections.namedtuple("PrepareCase", ["name", "src", "size", "entry", "divisor", "exact", "reliable"])


def DEV_REL(n):
    return (n + 2) * U


def SCALE_REL(n):
    return 2 * DEV_REL(n) + U


def offset_bar(n, t_mono, scale, offset):
    return abs(t_mono * scale) * (SCALE_REL(n) + U) + abs(offset) * U


def prepare_bar(src, divisor, entry):
    M = float(np.abs(np.asarray(src).astype(np.float64)).max()) / divisor
    if entry is not None and entry["scale"] > 0:
        return 8 * V * (M * abs(float(np.float32(entry["scale"]))) + abs(float(np.float32(entry["offset"]))))
    return 8 * V * M


def random_map(rng, h, w):
    return rng.integers(200, 65536, size=(h, w)).astype(np.uint16)


def camera(cid=1, width=WIDTH, height=HEIGHT):
    return gio.ColmapCamera(cid, "PINHOLE", width, height, np.array([50.0, 50.0, width / 2, height / 2]))


def world_points(z_cam, rng, q, t):
    """points whose view-space z under (q, t) is z_cam (up to rounding), at random view-space x, y"""
    n = len(z_cam)
    pc = np.column_stack((rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.asarray(z_cam, dtype=np.float64)))
    return (pc - np.asarray(t)) @ gio.qvec2rotmat(q)        # R^T (p - t), row-wise


def inside_xys(rng, n, width=WIDTH, height=HEIGHT):
    return np.column_stack((rng.uniform(1, width - 2, n), rng.uniform(1, height - 2, n)))


def one_image(name, n_good, rng, map_hw=(48, 64), q=IDENT, t=(0.0, 0.0, 0.0), z=None, xys=None, extra=None, expect=None):
    """One image with n_good observations that pass every test (ids 1..n_good of a dense table), then `extra`: a function
    (ids, xys, xyz) -> (ids, xys, xyz) that appends or edits."""
    z = rng.uniform(2.0, 10.0, n_good) if z is None else np.asarray(z, dtype=np.float64)
    xyz = world_points(z, rng, q, t)
    ids = np.arange(1, n_good + 1, dtype=np.int64)
    xys = inside_xys(rng, n_good) if xys is None else np.asarray(xys, dtype=np.float64)
    obs_ids = ids.copy()
    if extra is not None:
        obs_ids, xys, xyz, ids = extra(obs_ids, xys, xyz, ids)
    image = gio.ColmapImage(1, np.array(q, dtype=np.float64), np.array(t, dtype=np.float64), 1, name + ".jpg", xys, obs_ids)
    exp = dict(n_valid=n_good, zero=n_good <= 10)
    exp.update(expect or {})
    return ScaleCase(name, {1: image}, {1: camera()}, xyz, ids, {name: random_map(rng, *map_hw)}, {name: exp})


def _append(obs_ids, xys, xyz, ids, new_obs_ids, new_xys, new_xyz=None, new_ids=None):
    obs_ids = np.concatenate((obs_ids, np.asarray(new_obs_ids, dtype=np.int64)))
    xys = np.concatenate((xys, np.asarray(new_xys, dtype=np.float64).reshape(-1, 2)))
    if new_xyz is not None:
        xyz = np.concatenate((xyz, np.asarray(new_xyz, dtype=np.float64).reshape(-1, 3)))
        ids = np.concatenate((ids, np.asarray(new_ids, dtype=np.int64)))
    return obs_ids, xys, xyz, ids


def scale_cases():
    rng = np.random.default_rng(2024)
    out = []
    # the gate's count, odd and even medians
    for n in (10, 11, 12):
        out.append(one_image("n%d" % n, n, rng, q=GENERAL_Q, t=GENERAL_T))
    # ties across the median position, in both sequences: repeated depths, and a map that is constant where the samples fall
    for n in (12, 13):
        z = [2.0] * 2 + [4.0] * (n - 6) + [8.0] * 4
        c = one_image("ties%d" % n, n, rng, z=z, xys=np.column_stack((np.linspace(3, 40, n), np.full(n, 7.0))))
        m = c.maps["ties%d" % n].copy()
        m[:, :10], m[:, 10:30], m[:, 30:] = rng.integers(100, 500, size=(48, 10)), 30000, rng.integers(60000, 65536, size=(48, 34))
        out.append(c._replace(maps={"ties%d" % n: m}, expect={"ties%d" % n: dict(n_valid=n, zero=False, ties=True)}))
    # counts either side of the workgroup's width and of its multiples
    for n in (255, 256, 257, 1023, 4097):
        out.append(one_image("n%d" % n, n, rng, q=GENERAL_Q, t=GENERAL_T, map_hw=(48, 64) if n != 1023 else (24, 32)))

    # ids: -1, >= len(table), and 7, in range but absent from the model (the table's zero row: z = t2 = 0.5, used and valid)
    def bad_ids(obs_ids, xys, xyz, ids):
        keep = ids != 7
        obs_ids, xys, xyz, ids = obs_ids, xys, xyz[keep], ids[keep]     # the observation of id 7 stays, the point goes
        return _append(obs_ids, xys, xyz, ids, [-1, -1, len(obs_ids) + 1, 10 ** 6], inside_xys(rng, 4))
    out.append(one_image("ids", 20, rng, t=(0.0, 0.0, 0.5), extra=bad_ids, expect=dict(n_valid=20, absent_used=True)))

    # z < 0: not valid, but they widen max - min of the USED observations - the only reason the gate opens here
    def behind(obs_ids, xys, xyz, ids):
        return _append(obs_ids, xys, xyz, ids, [101, 102], inside_xys(rng, 2), [[0, 0, -5.0], [0, 0, -7.0]], [101, 102])
    out.append(one_image("z_negative", 15, rng, z=np.linspace(4.0, 4.001, 15), extra=behind,
                         expect=dict(n_valid=15, zero=False, valid_range_below_gate=True)))
    # z == +0 on every observation: inv = inf everywhere, inf - inf = NaN fails the gate although every one is "valid"
    out.append(one_image("z_zero_all", 14, rng, z=np.zeros(14), expect=dict(n_valid=14, zero=True, range_nan=True)))
    # z == +0 on one: numpy's statements give an infinite deviation and scale - the same non-finite answers are asked
    out.append(one_image("z_zero_one", 15, rng, z=[0.0] + list(np.linspace(2.0, 9.0, 14)), expect=dict(n_valid=15, zero=False, nonfinite=True)))

    # coordinates: on width * s (excluded), between w - 1 and w (included, replicated), negative (excluded); s = 0.5
    def on_edge(obs_ids, xys, xyz, ids):
        return _append(obs_ids, xys, xyz, ids, [1, 2, 3, 4], [[64.0, 10.0], [10.0, 48.0], [-0.25, 10.0], [10.0, -1e-9]])
    out.append(one_image("edge_excluded_s05", 12, rng, map_hw=(24, 32), extra=on_edge, expect=dict(n_valid=12)))

    def near_edge(obs_ids, xys, xyz, ids):
        return _append(obs_ids, xys, xyz, ids, [1, 2, 3], [[63.5, 10.0], [63.99, 47.99], [0.0, 0.0]])
    out.append(one_image("edge_included_s1", 12, rng, extra=near_edge, expect=dict(n_valid=15, replicated=True)))

    # max - min exactly 1e-3 (1 / 1000 - 1 / 1e30 rounds to 1 / 1000 = 0.001): not "> 1e-3"; and the next double above
    z_exact = [1000.0, 1e30] + list(np.linspace(1200.0, 5000.0, 12))
    out.append(one_image("range_exact", 14, rng, z=z_exact, expect=dict(n_valid=14, zero=True, range_is=1e-3)))
    z_next = math.nextafter(1000.0, 0.0)
    while not 1.0 / z_next > 1e-3:          # (the first z whose reciprocal rounds above 0.001)
        z_next = math.nextafter(z_next, 0.0)
    z_above = [z_next] + z_exact[1:]
    out.append(one_image("range_above", 14, rng, z=z_above, expect=dict(n_valid=14, zero=False, range_above=1e-3)))

    # several images in one call: three map sizes (s = 1, 0.5, 0.25), one image without observations, one without a map
    images, maps, expect = {}, {}, {}
    n_pts = 60
    xyz = world_points(rng.uniform(2.0, 10.0, n_pts), rng, GENERAL_Q, GENERAL_T)
    ids = np.arange(1, n_pts + 1, dtype=np.int64)
    for k, (name, hw, n) in enumerate((("a", (48, 64), 40), ("b", (24, 32), 31), ("c", (12, 16), 60), ("empty", (48, 64), 0),
                                       ("nomap", None, 20))):
        obs = rng.permutation(ids)[:n]
        images[k + 1] = gio.ColmapImage(k + 1, np.array(GENERAL_Q), np.array(GENERAL_T), 1, name + ".png", inside_xys(rng, n), obs)
        maps[name] = None if hw is None else random_map(rng, *hw)
        if hw is not None:
            expect[name] = dict(n_valid=n, zero=n <= 10)
    out.append(ScaleCase("several", images, {1: camera()}, xyz, ids, maps, expect))
    return out


# ------------------------------------------------------------------------------------------------ the camera's map
def fma_case(rng):
    """(src uint16 [4,4], entry) where float32 fma(x, s, o) differs from the two roundings at pixel [0,0]"""
    for _ in range(10000):
        v = int(rng.integers(1, 65536))
        s, o = np.float32(rng.uniform(0.5, 2.0)), np.float32(rng.uniform(0.1, 1.0))
        x = np.float32(v) / np.float32(65536)
        two = np.float32(np.float32(x * s) + o)
        exact = float(x) * float(s) + float(o)                       # the product is exact in double
        one = np.float32(exact)
        if two != one and float(np.float64(one)) != exact:           # (the double sum sits off a float32 tie: one rounding)
            src = rng.integers(0, 65536, size=(4, 4)).astype(np.uint16)
            src[0, 0] = v
            return src, dict(scale=float(s), offset=float(o), med_scale=float(s)), float(two), float(one)
    raise AssertionError("no case found")


def prepare_cases():
    rng = np.random.default_rng(77)
    u16 = lambda h, w: rng.integers(0, 65536, size=(h, w)).astype(np.uint16)  # noqa: E731
    mid = dict(scale=1.25, offset=0.125, med_scale=1.0)
    out = [
        PrepareCase("same_size", u16(6, 7), (7, 6), None, 65536.0, True, True),
        PrepareCase("half_of_even", u16(8, 12), (6, 4), None, 65536.0, True, True),
        PrepareCase("one_column_out", u16(5, 9), (1, 3), None, 65536.0, False, True),
        PrepareCase("one_row_source", u16(1, 9), (4, 3), None, 65536.0, False, True),
        PrepareCase("w7_to_5", u16(7, 7), (5, 5), mid, 65536.0, False, True),
        PrepareCase("w5_to_7", u16(5, 5), (7, 7), mid, 65536.0, False, True),
        PrepareCase("largest_64x48", u16(48, 64), (37, 29), mid, 65536.0, False, True),
        PrepareCase("nerf_synthetic_512", u16(6, 6), (4, 4), None, 512.0, False, True),
        PrepareCase("negative_source", (rng.uniform(-30000, 30000, size=(6, 6))).astype(np.float32), (4, 5), None, 65536.0, False, True),
        PrepareCase("scale_zero_unscaled", u16(5, 5), (5, 5), dict(scale=0.0, offset=9.0, med_scale=0.0), 65536.0, True, True),
        PrepareCase("scale_negative_unscaled", u16(5, 5), (3, 3), dict(scale=-1.0, offset=9.0, med_scale=1.0), 65536.0, False, False),
        PrepareCase("edge_low_on", u16(4, 4), (4, 4), dict(scale=0.2, offset=0.0, med_scale=1.0), 65536.0, False, True),
        PrepareCase("edge_low_below", u16(4, 4), (4, 4), dict(scale=math.nextafter(0.2, 0.0), offset=0.0, med_scale=1.0), 65536.0, False, False),
        PrepareCase("edge_high_on", u16(4, 4), (4, 4), dict(scale=5.0, offset=0.0, med_scale=1.0), 65536.0, False, True),
        PrepareCase("edge_high_above", u16(4, 4), (4, 4), dict(scale=math.nextafter(5.0, 6.0), offset=0.0, med_scale=1.0), 65536.0, False, False),
    ]
    src, entry, _, _ = fma_case(np.random.default_rng(5))
    out.append(PrepareCase("no_fma", src, (4, 4), entry, 65536.0, False, True))
    return out
