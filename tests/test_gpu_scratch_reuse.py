"""A forward's outputs do not depend on what its scratch buffers held before it ran.

The kernels skip writes on purpose (a Gaussian the depth limits cut entirely leaves no Splat record behind,
csrc/gs_preprocess.hip), and the geometry / image / binning buffers are fresh torch.empty blocks from the caching allocator -
in a training loop usually the previous camera's.  So nothing downstream may read a byte this forward did not write.
RasterBackend.scratch_fill hands every fresh buffer to the test before the forward runs; it is filled with zeros or with the
raw bytes of an earlier forward of the same scene and image size from another camera (realistic content only: arbitrary
bytes could send indices anywhere).  Checked here:
  1. zero-filled and reused scratch give bit-identical outputs and exported state, on the LSD path (csrc/gs_binning.hip +
     csrc/gs_tilebin.hip) and with region binning, at both sizes of the depth sort (one workgroup up to 16 384 Gaussians,
     multi-pass above), with and without depth limits; the limited views render the un-limited bits;
  2. the header of the geometry buffer (GeomHeader) agrees with the lists: no overflow, every instance counted is in a list,
     and the depth order holds exactly the Gaussians that have instances;
  3. the row-wise entry enumeration builds the same depth-limited lists at both sort sizes;
  4. a 12 288 x 12 288 image, where a full-image splat reaches 36 864 regions - more than the 15-bit entry count in the Splat
     record holds: the culled lists render what the reference's lists render.
(tests/test_gpu_regionbin.py::test_fused_train_step_on_region_lists_is_the_lsd_run runs training through reused buffers.)"""
import functools
import gc

import numpy as np
import pytest
import torch

from gsplat_amd import synthetic
from helpers import canonical_lists
from test_gpu_depth_limit import assert_prefix_property, device_camera
from test_gpu_raster_parity import forward_state, last_contributor_id

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# GeomHeader words (csrc/gs_common.h)
H_NUM_RENDERED, H_OVERFLOW, H_TRUNC_FAILED, H_P, H_SORT_N, H_N_ORDERED, H_REGION_MODE = 0, 1, 2, 4, 5, 6, 7


@pytest.fixture(autouse=True)
def backend_state(hip):
    names = ("tile_cull", "binning", "depth_limit_on", "_capacity_hint", "_capacity_hint_limited", "force_rowwise_entries",
             "scratch_fill")
    old = {k: getattr(hip, k) for k in names}
    hip._cam_cache.clear()
    hip._region_off.clear()
    yield
    for k, v in old.items():
        setattr(hip, k, v)
    hip._cam_cache.clear()
    hip._region_off.clear()


class Fill:
    """RasterBackend.scratch_fill: every fresh buffer gets zeros, or the bytes of the same buffer of an earlier forward
    (geom and img: same scene and image size, so the same length; binning: the common prefix, zeros behind it)."""

    def __init__(self, src=None):
        self.src = src
        self.kinds = []

    def __call__(self, kind, t):
        self.kinds.append(kind)
        if self.src is None:
            t.zero_()
            return
        s = self.src[kind]
        if kind != "binning":
            assert s.numel() == t.numel(), kind
        n = min(s.numel(), t.numel())
        t[:n].copy_(s[:n])
        t[n:].zero_()


def header(buffers):
    return buffers["geom"][:256].view(torch.int32).cpu()


def check_header(st, hdr, lsd):
    """the geometry buffer's header against the lists of the same forward"""
    P = st["tiles_touched"].numel()
    R = st["num_rendered"]
    assert int(hdr[H_OVERFLOW]) == 0 and int(hdr[H_P]) == P
    assert int(hdr[H_NUM_RENDERED]) == R
    counts = torch.bincount(st["point_list"].long(), minlength=P)
    assert int(counts.sum()) == R == st["point_list"].numel()
    if lsd:
        assert int(hdr[H_REGION_MODE]) == 0
        assert int(hdr[H_SORT_N]) == R, "the lists hold another number of instances than the geometry phase counted"
        assert torch.equal(counts.int(), st["tiles_touched"].int()), "a Gaussian is in more or fewer lists than it has tiles"
        assert int(hdr[H_N_ORDERED]) == int((st["tiles_touched"] > 0).sum()), "the depth order holds Gaussians without instances"
    else:
        # (region binning counts regions in tiles_touched: every Gaussian named in a list has some)
        assert int(hdr[H_REGION_MODE]) == 1
        assert bool((st["tiles_touched"][counts > 0] > 0).all())


PIXELS = ("color", "invdepth", "final_T", "n_contrib")
EXPORTS = ("depths", "means2D", "conic_opacity", "rgb", "clamped", "tiles_touched", "cov3D", "radii")


def assert_same_forward(a, b, lsd, what):
    assert a["num_rendered"] == b["num_rendered"], what
    for k in PIXELS + EXPORTS:
        assert torch.equal(a[k], b[k]), (what, k)
    if lsd:
        for k in ("ranges", "point_list", "keys_sorted"):
            assert torch.equal(a[k], b[k]), (what, k)
    else:
        # (region binning places each tile's list wherever its region reserved room, in atomic order: the lists themselves
        #  and their keys are compared tile by tile)
        ca, ka = canonical_lists(a)
        cb, kb = canonical_lists(b)
        assert np.array_equal(ca, cb) and np.array_equal(ka, kb), (what, "lists")
        assert torch.equal(torch.sort(a["keys_sorted"]).values, torch.sort(b["keys_sorted"]).values), (what, "keys_sorted")


SIZES = [(10000, 400, 400), (30000, 800, 600)]   # one-workgroup depth sort (<= 16 384) / multi-pass


@functools.lru_cache(maxsize=None)
def scene(P, seed, deg):
    """(host tensors, never modified: forward_state copies them to the device)"""
    return synthetic.trained_like(P, seed=seed, sh_degree=deg)
MODES = [("lsd", 0, False), ("lsd", 1, False), ("lsd", 1, True), ("region", 1, False), ("region", 1, True)]


@pytest.mark.parametrize("binning,cull,limits", MODES, ids=["lsd-cull0", "lsd-cull1", "lsd-cull1-limits", "region-cull1",
                                                             "region-cull1-limits"])
@pytest.mark.parametrize("P,W,H", SIZES, ids=["P10k", "P30k"])
def test_outputs_do_not_depend_on_what_the_scratch_held(hip, P, W, H, binning, cull, limits):
    sc = scene(P, 0, 3)
    cams = synthetic.orbit_cameras(W, H)
    cam_a, cam_b = device_camera(cams[3]), device_camera(cams[13])
    bg = torch.tensor([0.2, 0.1, 0.3])
    hip.binning, hip.tile_cull, hip.depth_limit_on = binning, bool(cull), limits
    lsd = binning == "lsd" or not cull
    first = forward_state(hip, sc, cam_a, DEV, bg, False)            # A, first visit: full lists (measures the stop depths)
    other = {}
    forward_state(hip, sc, cam_b, DEV, bg, False, buffers=other)     # B: the bytes A's next visits find
    used0, failed0 = hip.depth_limit_stats["used"], hip.depth_limit_stats["failed"]
    got = []
    for src in (None, other):
        hip.scratch_fill = fill = Fill(src)
        bufs = {}
        st = forward_state(hip, sc, cam_a, DEV, bg, False, buffers=bufs)
        hip.scratch_fill = None
        assert {"geom", "img", "binning"} <= set(fill.kinds)
        check_header(st, header(bufs), lsd)
        got.append(st)
    if limits:
        assert hip.depth_limit_stats["used"] == used0 + 2 and hip.depth_limit_stats["failed"] == failed0
        assert got[0]["num_rendered"] < first["num_rendered"]
        # a Gaussian all of whose pairs were cut (no record in this forward) is exported as not visible
        cut = (got[0]["tiles_touched"] == 0) & (got[0]["radii"] > 0)
        assert int(cut.sum()) > 0
        assert not bool(got[0]["depths"][cut].any()) and not bool(got[0]["conic_opacity"][cut].any())
    else:
        assert_same_forward(first, got[0], lsd, "second visit")
    assert_same_forward(got[0], got[1], lsd, "zeroed / reused scratch")
    # against the same camera without limits: the pixels, and every entry the blend visits is in the cut lists
    for k in PIXELS:
        assert torch.equal(first[k], got[1][k]), k
    assert torch.equal(last_contributor_id(first, W, H), last_contributor_id(got[1], W, H))
    if limits:
        assert_prefix_property(first, got[1], W, H)


@pytest.mark.parametrize("P,W,H", SIZES, ids=["P10k", "P30k"])
def test_row_wise_entries_build_the_same_depth_limited_lists(hip, P, W, H):
    sc = scene(P, 0, 3)
    cams = synthetic.orbit_cameras(W, H)
    cam = device_camera(cams[5])
    bg = torch.zeros(3)
    hip.binning, hip.tile_cull, hip.depth_limit_on = "lsd", True, True
    first = forward_state(hip, sc, cam, DEV, bg, False)
    used0 = hip.depth_limit_stats["used"]
    hip.scratch_fill = Fill()
    bufs = {}
    a = forward_state(hip, sc, cam, DEV, bg, False, buffers=bufs)
    check_header(a, header(bufs), True)
    hip.force_rowwise_entries = True
    b = forward_state(hip, sc, cam, DEV, bg, False, buffers=bufs)
    check_header(b, header(bufs), True)
    assert hip.depth_limit_stats["used"] == used0 + 2 and hip.last_status()[2] == 0
    assert a["num_rendered"] < first["num_rendered"]
    assert_same_forward(a, b, True, "row-wise entries")
    for k in PIXELS:
        assert torch.equal(first[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 12 288 x 12 288: 768 x 768 tiles, 192 x 192 = 36 864 regions.  A splat that covers the whole image has 36 864 region entries,
# more than the 15 bits (TB_ENTRIES_MAX) the preprocess kernel leaves the count in: the count must be left to the binning.
# (~151 M pixels: outputs stay on the GPU, a leg's buffers are freed before the next one.)
BIG = 12288


def big_scene():
    sc = synthetic.trained_like(300, seed=4, sh_degree=0)
    # four splats at the centre of the orbit, ~6 000 px standard deviation at this focal length (17 000 px, depth ~4): every
    # tile row of the alpha >= 1/255 ellipse spans the whole image; opacity 0.3 lets the ordinary splats show through
    sc["means3D"][:4] = torch.tensor([[0.0, 0.0, 0.0], [0.05, -0.03, 0.02], [-0.04, 0.02, 0.06], [0.02, 0.05, -0.05]])
    sc["scales"][:4] = torch.tensor([[1.5, 1.5, 1.5], [1.4, 1.6, 1.5], [1.7, 1.3, 1.5], [1.5, 1.5, 1.6]])
    sc["opacities"][:4] = 0.3
    return sc


def big_forward(hip, sc, cam, bg):
    """forward + exports, kept on the GPU; -> (outputs, geometry header)"""
    e = torch.empty(0, device=DEV)
    args = (bg.to(DEV), sc["means3D"].to(DEV), e, sc["opacities"].to(DEV), sc["scales"].to(DEV), sc["rotations"].to(DEV), 1.0, e,
            cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), cam.tanfovx, cam.tanfovy, cam.image_height,
            cam.image_width, sc["shs"].to(DEV), sc["sh_degree"], cam.camera_center.to(DEV), False, False, False)
    R, color, radii, geom, binning, img, invd = hip.rasterize_gaussians(*args)
    P = sc["means3D"].shape[0]
    st = hip.export_state(P, BIG, BIG, R, geom, binning, img)
    hdr = geom[:256].view(torch.int32).cpu()
    del geom, binning, img
    # each pixel's last contributor (test_gpu_raster_parity.last_contributor_id, on the device)
    gx = (BIG + 15) // 16
    ys = torch.arange(BIG, device=DEV)
    tile = ((ys // 16) * gx)[:, None] + (ys // 16)[None, :]
    start = st["ranges"][:, 0].long()[tile]
    n = st["n_contrib"].long()
    pl = st["point_list"].long()
    last = pl[(start + n - 1).clamp(0, max(pl.numel() - 1, 0))] if pl.numel() else torch.zeros_like(n)
    last = torch.where(n > 0, last, torch.full_like(last, -1)).int()
    del tile, start, n
    out = dict(num_rendered=R, color=color, invdepth=invd, final_T=st["final_T"], last=last, radii=radii,
               tiles_touched=st["tiles_touched"].cpu(), point_list=st["point_list"].cpu())
    return out, hdr


def test_splats_that_cover_a_12k_image(hip):
    sc = big_scene()
    cam = synthetic.orbit_cameras(BIG, BIG)[2]
    bg = torch.tensor([0.1, 0.2, 0.3])
    hip.depth_limit_on = False
    hip.binning, hip.tile_cull = "lsd", False
    ref, hdr = big_forward(hip, sc, cam, bg)       # the reference's rectangles: counted through tb_rect_entries
    check_header(ref, hdr, True)
    big = ref["tiles_touched"][:4]
    assert bool((big == 768 * 768).all()), big     # (every tile of the image)
    legs = [("lsd", False), ("lsd", True), ("region", False)]
    for binning, rowwise in legs:
        hip.binning, hip.tile_cull, hip.force_rowwise_entries = binning, True, rowwise
        got, hdr = big_forward(hip, sc, cam, bg)
        what = (binning, rowwise)
        check_header(got, hdr, binning == "lsd")
        if binning == "lsd":
            assert bool((got["tiles_touched"][:4] == 768 * 768).all()), what
        for k in ("color", "invdepth", "final_T", "last", "radii"):
            assert torch.equal(ref[k], got[k]), (what, k)
        del got
        gc.collect()
        torch.cuda.empty_cache()
