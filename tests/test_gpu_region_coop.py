"""Region mode of the forward geometry kernel (csrc/gs_preprocess.hip, GsView.tile_cull = 2) in its cooperative form: a
Gaussian whose region rectangle holds more than four regions publishes it, and the lanes of its wave take the (region,
Gaussian) pairs of all published rectangles one pair per lane, GS_COOP_PAIRS per lane and round.  Against the LSD lists
(tests/test_gpu_regionbin.py pins the per-lane form the same way) and against the per-lane form itself
(RasterBackend.region_coop = False, gs_region_coop), bit for bit: bucket order is arbitrary in both, region_bin_kernel sorts.

Scenes are constructed: a camera that looks along +z with its axes on the world's, Gaussians flat in z placed by pixel
centre and pixel sigma, so that the region rectangle of each planted one is known - its `tiles_touched` (the number of
regions, in region mode) is asserted.  An image of 256 x 160 has 4 x 3 regions; a rectangle count of 5 does not exist
there (5 = 1 x 5), so the first count past the batch of four is planted in a 320 x 160 image (5 x 3 regions) as well."""

import numpy as np
import pytest
import torch

from gsplat_amd import synthetic
from helpers import canonical_lists
from test_gpu_raster_parity import forward_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FOVX = 0.6911112070083618
PIXELS = ("color", "invdepth", "final_T", "n_contrib", "radii")
RECORD = ("depths", "means2D", "conic_opacity", "rgb", "cov3D", "clamped")


@pytest.fixture(autouse=True)
def region_lists(hip):
    names = ("tile_cull", "binning", "depth_limit_on", "_capacity_hint", "_capacity_hint_limited")
    old = {k: getattr(hip, k) for k in names}
    coop = hip.region_coop
    hip.tile_cull, hip.binning, hip.depth_limit_on = True, "region", False
    hip.region_coop = True
    hip._cam_cache.clear()
    hip._region_off.clear()
    yield
    for k, v in old.items():
        setattr(hip, k, v)
    hip.region_coop = coop
    hip._cam_cache.clear()
    hip._region_off.clear()


# ---- constructed scenes ---------------------------------------------------------------------------------------------------
def front_camera(W, H):
    """axes = the world's, 4 in front of the plane z = 0"""
    fovy = synthetic.focal2fov(synthetic.fov2focal(FOVX, W), H)
    return synthetic.make_camera(np.eye(3), (0.0, 0.0, 4.0), FOVX, fovy, W, H)


def small_ones(P, seed):
    """P Gaussians of a few pixels, as synthetic.trained_like makes them (full SH rows, random rotations)"""
    return synthetic.trained_like(P, seed=seed, sh_degree=3, scale_mult=0.1)


def plant(sc, cam, row, cx, cy, sx, sy, depth=4.0, opacity=0.9):
    """row `row` of the scene becomes a Gaussian flat in z with pixel centre (cx, cy) and pixel sigmas (sx, sy) at `depth`"""
    W, H = cam.image_width, cam.image_height
    focal = synthetic.fov2focal(FOVX, W)
    x = ((2.0 * cx + 1.0) / W - 1.0) * cam.tanfovx * depth
    y = ((2.0 * cy + 1.0) / H - 1.0) * cam.tanfovy * depth
    sc["means3D"][row] = torch.tensor([x, y, depth - 4.0])
    sc["scales"][row] = torch.tensor([sx * depth / focal, sy * depth / focal, 1.0e-4])
    sc["rotations"][row] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc["opacities"][row] = opacity


# (cx, cy, sigma x, sigma y) -> regions of a 256 x 160 image: the reference square of radius ceil(3 sigma_max) cut by the
# alpha >= 1/255 box (3.3 sigma + 1 px per axis at opacity 0.9), edges at least 2 px away from a region border
FOOTPRINT = {1: (40, 40, 3, 3), 2: (64, 40, 3, 3), 3: (96, 40, 11, 2), 4: (64, 64, 3, 3), 6: (96, 64, 11, 3),
             8: (128, 64, 22, 3), 9: (96, 96, 11, 11), 12: (128, 88, 22, 22)}
ALL12 = FOOTPRINT[12]
ALL12_DIM = (128, 88, 24, 24)   # the same twelve at opacity 0.3, where the alpha >= 1/255 box (2.9 sigma + 1 px) is the inner one


def all12_rows(sc, cam, rows):
    for i, row in enumerate(rows):   # (different centres and depths: the bucket sort has something to order)
        plant(sc, cam, row, ALL12_DIM[0] + i % 3 - 1, ALL12_DIM[1] - i % 2, ALL12_DIM[2], ALL12_DIM[3], depth=3.0 + 0.02 * i,
              opacity=0.3)
    return {row: 12 for row in rows}


def build(name):
    """-> scene, camera, {row: regions its Gaussian reaches}"""
    if name == "batch_edge":
        cam, sc = front_camera(256, 160), small_ones(208, 1)
        want = {}
        for row, n in zip((3, 40, 77, 101, 130, 166, 190, 207), sorted(FOOTPRINT)):
            plant(sc, cam, row, *FOOTPRINT[n])
            want[row] = n
    elif name == "five_regions":
        cam, sc = front_camera(320, 160), small_ones(100, 2)
        plant(sc, cam, 50, 168, 40, 40, 2)
        want = {50: 5}
    elif name == "rows_0_63":
        cam, sc = front_camera(256, 160), small_ones(200, 3)
        want = all12_rows(sc, cam, range(0, 64))
    elif name == "rows_60_123":
        cam, sc = front_camera(256, 160), small_ones(200, 4)
        want = all12_rows(sc, cam, range(60, 124))
    elif name == "partial_workgroup":
        cam, sc = front_camera(256, 160), small_ones(256 + 37, 5)
        want = all12_rows(sc, cam, (270, 292))
    elif name == "sixty_regions":
        cam, sc = front_camera(640, 384), small_ones(150, 6)
        plant(sc, cam, 17, 328, 200, 120, 120, opacity=0.3)
        want = {17: 60}
    else:
        raise KeyError(name)
    return sc, cam, want


CONSTRUCTED = ("batch_edge", "five_regions", "rows_0_63", "rows_60_123", "partial_workgroup", "sixty_regions")
BG = torch.tensor([0.3, 0.1, 0.2])


def assert_same_forward(a, b, what, lists=True):
    assert a["num_rendered"] == b["num_rendered"], what
    assert torch.equal(a["tiles_touched"], b["tiles_touched"]), what
    seen = a["tiles_touched"] > 0
    for k in RECORD:
        assert torch.equal(a[k][seen], b[k][seen]), (what, k)
    if lists:
        ca, ka = canonical_lists(a)
        cb, kb = canonical_lists(b)
        assert np.array_equal(ca, cb) and np.array_equal(ka, kb), what
    for k in PIXELS:
        assert torch.equal(a[k], b[k]), (what, k)


# ---- against the LSD lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONSTRUCTED)
def test_cooperative_lists_equal_the_lsd_lists_tile_by_tile(hip, name):
    sc, cam, want = build(name)
    hip.binning = "lsd"
    a = forward_state(hip, sc, cam, DEV, BG, False)
    hip.binning = "region"
    assert hip.region_coop
    b = forward_state(hip, sc, cam, DEV, BG, False)
    for row, n in want.items():
        assert int(b["tiles_touched"][row]) == n, (row, n, int(b["tiles_touched"][row]))
    assert a["num_rendered"] == b["num_rendered"] > 0
    ca, ka = canonical_lists(a)
    cb, kb = canonical_lists(b)
    assert np.array_equal(ca, cb), "tile list lengths differ"
    assert np.array_equal(ka, kb), "a tile's list differs"
    for k in PIXELS:
        assert torch.equal(a[k], b[k]), k


# ---- against the per-lane form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONSTRUCTED + ("init_10000",))
def test_both_forms_build_the_same_state(hip, name):
    if name == "init_10000":   # large isotropic splats: many regions per Gaussian
        sc, cam = synthetic.init_like(10000, seed=0, sh_degree=0), synthetic.orbit_cameras(400, 400)[3]
    else:
        sc, cam, _ = build(name)
    hip.region_coop = False
    assert not hip.region_coop
    old = forward_state(hip, sc, cam, DEV, BG, False)
    hip.region_coop = True
    new = forward_state(hip, sc, cam, DEV, BG, False)
    again = forward_state(hip, sc, cam, DEV, BG, False)
    assert new["num_rendered"] > 0 and int((new["tiles_touched"] > 4).sum()) > 0
    assert_same_forward(old, new, name + ": per-lane / cooperative")
    assert_same_forward(new, again, name + ": cooperative twice")


# ---- depth limits ---------------------------------------------------------------------------------------------------------
def walled_scene():
    """256 x 160: two opaque layers at depth 4 / 4.05 saturate every pixel left of x = 148 - tile columns 0 .. 8, so the tiles
    of region columns 0 and 1 get finite bounds and region columns 2 and 3 none (a bound is the largest stop depth of the
    tile's 3 x 3 neighbourhood, a region's the largest of its tiles').  Planted, all of more than four regions: a near one over
    all twelve (keeps them), a far one over all twelve (loses region columns 0 and 1) and a far one inside region
    columns 0 and 1 (loses everything)."""
    cam = front_camera(256, 160)
    xs, ys = range(-12, 151, 6), range(-12, 173, 6)
    n_wall = 2 * len(xs) * len(ys)
    P = 100 + n_wall + 64
    sc = small_ones(P, 7)
    row = 100
    for layer in range(2):
        for cy in ys:
            for cx in xs:
                plant(sc, cam, row, cx, cy, 6, 6, depth=4.0 + 0.05 * layer, opacity=0.99)
                row += 1
    near, far_some, far_all = 10, 50, P - 1
    plant(sc, cam, near, *ALL12_DIM, depth=3.0, opacity=0.3)
    plant(sc, cam, far_some, *ALL12, depth=6.0)
    plant(sc, cam, far_all, 64, 80, 18, 18, depth=6.0)
    return sc, cam, near, far_some, far_all


def test_depth_limited_lists_of_both_forms(hip):
    from test_gpu_depth_limit import assert_prefix_property
    sc, cam, near, far_some, far_all = walled_scene()
    W, H = cam.image_width, cam.image_height
    hip.depth_limit_on = True
    full, cut = {}, {}
    for arm in ("lsd", "per_lane", "coop"):
        hip.binning = "lsd" if arm == "lsd" else "region"
        hip.region_coop = arm == "coop"
        hip._cam_cache.clear()
        used0 = hip.depth_limit_stats["used"]
        full[arm] = forward_state(hip, sc, cam, DEV, BG, False)   # first visit measures the stop depths
        cut[arm] = forward_state(hip, sc, cam, DEV, BG, False)    # second visit: cut lists
        assert hip.depth_limit_stats["used"] == used0 + 1 and hip.last_status()[2] == 0, arm
        for k in PIXELS:
            assert torch.equal(full[arm][k], cut[arm][k]), (arm, k)
    assert_same_forward(full["per_lane"], full["coop"], "first visit")
    assert_same_forward(cut["per_lane"], cut["coop"], "second visit")
    t = cut["coop"]["tiles_touched"]
    assert int(full["coop"]["tiles_touched"][near]) == int(t[near]) == 12, "the near one keeps every region"
    assert int(full["coop"]["tiles_touched"][far_some]) == 12 and int(t[far_some]) == 6, int(t[far_some])
    assert int(full["coop"]["tiles_touched"][far_all]) == 6 and int(t[far_all]) == 0
    # no record: gs_export_geom reports it as invisible, the radius is the reference's
    assert int(cut["coop"]["radii"][far_all]) > 0 and float(cut["coop"]["depths"][far_all]) == 0.0
    assert not cut["coop"]["conic_opacity"][far_all].any() and float(full["coop"]["depths"][far_all]) > 5.9
    # the subset rule against the LSD path (test_gpu_regionbin.test_depth_limited_region_lists)
    assert torch.equal(full["lsd"]["color"], full["coop"]["color"])
    kf = canonical_lists(full["coop"])[1]
    kl, kr = canonical_lists(cut["lsd"])[1], canonical_lists(cut["coop"])[1]
    assert np.array_equal(kf[np.isin(kf, kr)], kr), "limited region list is not a subsequence of the full list"
    assert np.isin(kr, kl).all(), "the exact per-tile cut must lie inside the LSD path's span-trimmed cut"
    assert len(kr) <= len(kl) < len(kf)
    assert_prefix_property(full["coop"], cut["coop"], W, H)


# ---- bucket overflow ------------------------------------------------------------------------------------------------------
def test_bucket_overflow_is_detected_and_the_view_rendered_again(hip):
    sc, cam, _ = build("rows_60_123")     # 64 Gaussians in each of the 12 region buckets, on top of the small ones
    ref = forward_state(hip, sc, cam, DEV, BG, False)
    R = ref["num_rendered"]
    kref = canonical_lists(ref)[1]
    regions = 4 * 3
    # too few instances of room for the region buckets / for the lists / plenty
    for hint in (regions, 40 * regions, R // 3, R - 1, 10 * R):
        hip._capacity_hint = hint
        got = forward_state(hip, sc, cam, DEV, BG, False)
        assert got["num_rendered"] == R, hint
        assert np.array_equal(canonical_lists(got)[1], kref), hint
        assert torch.equal(got["color"], ref["color"]) and torch.equal(got["n_contrib"], ref["n_contrib"]), hint
        assert torch.equal(got["tiles_touched"], ref["tiles_touched"]), hint
        assert hip._capacity_hint >= R
