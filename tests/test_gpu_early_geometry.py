"""The early geometry pass (gs_forward_geometry_early, RasterBackend.EARLY_GEOMETRY): the geometry kernel of
the NEXT view runs on the side stream over the 256-row blocks without a reached row, in place, and the next forward's own launch
serves the blocks that are left.  Checked here:
  1. the two launches together leave what the single launch leaves - lists tile by tile, records, radii, tiles_touched, image,
     n_contrib - on sizes below, at and above one block, on a size with both kinds of blocks, with block 0 on either side, and
     with an empty early or an empty late launch; the early launch alone writes the unreached blocks and nothing else;
  2. a Trainer with the pass on is the Trainer with it off, bit for bit, over 8 steps on 3 cameras - also through every event
     that makes an early result stale (another camera than the predicted one, limits that fail, a densification, an opacity
     reset) and with the per-lane form of the kernel (GS_REGION_COOP=0).
Region binning places a tile's list inside point_list wherever its region reserved room (csrc/gs_regionbin.hip): ranges[] are
compared as lengths and the lists tile by tile (helpers.canonical_lists), as tests/test_gpu_regionbin.py does.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import reached_scenes
from gsplat_amd import synthetic
from helpers import canonical_lists
from test_gpu_raster_parity import forward_state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
W, H = reached_scenes.W, reached_scenes.H


def _knn(x):
    from simple_knn._C import distCUDA2
    return distCUDA2(x.to(DEV)).cpu()


@pytest.fixture(autouse=True)
def region_lists(hip):
    old = (hip.tile_cull, hip.binning, hip.depth_limit_on, hip._capacity_hint, hip._capacity_hint_limited)
    hip.tile_cull, hip.binning, hip.depth_limit_on = True, "region", False
    hip._cam_cache.clear()
    hip._region_off.clear()
    hip.drop_early_geometry()
    coop = hip.region_coop
    yield
    hip.drop_early_geometry()
    hip.region_coop = coop
    hip.tile_cull, hip.binning, hip.depth_limit_on, hip._capacity_hint, hip._capacity_hint_limited = old
    for k in ("TWO_PHASE", "TWO_PHASE_MIN_P", "EARLY_GEOMETRY"):
        if k in hip.__dict__:
            delattr(hip, k)
    hip._cam_cache.clear()
    hip._region_off.clear()


def walled(P, seed=4):
    """P rows with both kinds of blocks (rows in random order leave a reached row in every block): reached_scenes.wall first - its
    opaque shells cover the image from every orbit camera -, then a trained_like cloud pushed out to 10 - 20 times the shells' radius:
    behind the camera, off screen, or listed behind saturated pixels - never reached.  (Far away and not inside the ball: that
    many Gaussians in the image centre overfill a region's bucket.)"""
    wall = reached_scenes.wall()
    n = P - reached_scenes.P
    sc = synthetic.trained_like(n, seed=seed, sh_degree=3, knn=_knn)
    m = sc["means3D"]
    r = 20.0 + 16.0 * torch.rand((n, 1), generator=torch.Generator().manual_seed(seed))
    sc["means3D"] = m / m.norm(dim=1, keepdim=True).clamp_min(1e-6) * r
    sc["scales"] = sc["scales"] * 10.0
    return {k: (torch.cat([wall[k], v]).contiguous() if torch.is_tensor(v) else v) for k, v in sc.items()}


# ---------------------------------------------------------------------------------------------- 1. the two launches
def _args(sc, cam, bg):
    e = torch.empty(0)
    return (bg.to(DEV), sc["means3D"].to(DEV), e, sc["opacities"].to(DEV), sc["scales"].to(DEV), sc["rotations"].to(DEV), 1.0, e,
            cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV), cam.tanfovx, cam.tanfovy, cam.image_height,
            cam.image_width, sc["shs"].to(DEV), sc.get("sh_degree", 0), cam.camera_center.to(DEV), False, False, False)


def split_forward(hip, flags_scene, sc, cam0, cam1, bg):
    """A forward of `flags_scene` from cam0 leaves its reached flags in the buffers; then `sc` from cam1 as early launch (side
    stream) + late launch (gs_forward_geometry with the event), binning and blend in those buffers.
    -> (state of the cam1 forward, the flags [P] the launches split on, radii as the early launch alone left them)"""
    P = int(sc["means3D"].shape[0])
    hip._capacity_hint = max(64 * P, 1 << 20)   # (room for either camera's lists: the buffers are the first forward's)
    R0, _, _, geom, binning, img, _ = hip.rasterize_gaussians(*_args(flags_scene, cam0, bg))
    reached = hip.export_reached(P, geom).cpu()
    cap = hip._capacity_for(binning, P, W, H, R0)
    a = _args(sc, cam1, bg)
    keep = []
    view = hip._view(keep, DEV, a[0], a[8], a[9], a[16], cam1.tanfovx, cam1.tanfovy, H, W, 1.0, sc.get("sh_degree", 0), False, False,
                     False, tile_cull=2)
    g = hip._gauss(keep, DEV, a[1], a[14], None, a[3], a[4], a[5], None)
    radii = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    s = hip._scratch(geom, img, binning, cap)
    main = torch.cuda.current_stream(DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(main)
    hip.api.call("forward_geometry_early", C.byref(view), C.byref(g), C.byref(s), radii.data_ptr(), C.c_void_p(side.cuda_stream))
    done = torch.cuda.Event()
    done.record(side)
    side.synchronize()
    radii_early = radii.cpu()
    s.early_geometry_done = done.cuda_event
    stream = C.c_void_p(main.cuda_stream)
    hip.api.call("forward_geometry", C.byref(view), C.byref(g), C.byref(s), radii.data_ptr(), None, stream)
    assert not s.early_geometry_done, "the field is one-shot: a repeated forward runs in full"
    status = torch.zeros((16,), dtype=torch.int32).pin_memory()
    hip.api.call("forward_bin", C.byref(view), C.byref(g), C.byref(s), status.data_ptr(), stream)
    color = torch.empty((3, H, W), dtype=torch.float32, device=DEV)
    invd = torch.empty((1, H, W), dtype=torch.float32, device=DEV)
    hip.api.call("forward_render", C.byref(view), C.byref(g), C.byref(s), color.data_ptr(), invd.data_ptr(), stream)
    main.synchronize()
    R = int(status[0])
    assert int(status[1]) == 0, "region buckets overflowed: status %r" % (status[:4].tolist(),)
    st = {k: v.cpu() for k, v in hip.export_state(P, W, H, R, geom, binning, img).items()}
    st.update(num_rendered=R, color=color.cpu(), radii=radii.cpu(), invdepth=invd.cpu())
    return st, reached, radii_early


def assert_same_forward(a, b):
    assert a["num_rendered"] == b["num_rendered"]
    ra, rb = a["ranges"].long(), b["ranges"].long()
    assert torch.equal(ra[:, 1] - ra[:, 0], rb[:, 1] - rb[:, 0]), "ranges"
    ca, ka = canonical_lists(a)
    cb, kb = canonical_lists(b)
    assert np.array_equal(ca, cb) and np.array_equal(ka, kb), "a tile's list differs"
    for k in ("radii", "tiles_touched", "color", "invdepth", "n_contrib", "final_T"):
        assert torch.equal(a[k], b[k]), k
    listed = torch.unique(a["point_list"].long())
    for k in ("depths", "means2D", "cov3D", "conic_opacity", "rgb", "clamped"):
        assert torch.equal(a[k][listed], b[k][listed]), "record: " + k


def blocks_with(reached):
    P = reached.numel()
    pad = torch.zeros(((P + 255) // 256) * 256, dtype=torch.bool)
    pad[:P] = reached != 0
    return pad.view(-1, 256).any(dim=1)


def check_split(hip, flags_scene, sc, want_blocks):
    cams = reached_scenes.cameras()
    bg = torch.tensor([0.3, 0.1, 0.2])
    got, reached, radii_early = split_forward(hip, flags_scene, sc, cams[0], cams[1], bg)
    hip._capacity_hint = 0
    ref = forward_state(hip, sc, cams[1], DEV, bg, False)
    assert ref["num_rendered"] > 0
    has = blocks_with(reached)
    want_blocks(has)
    # the early launch alone: every row of a block without a reached row, no row of any other
    P = reached.numel()
    row_block_has = has.repeat_interleave(256)[:P]
    assert bool((radii_early[row_block_has] == -7).all()), "the early launch wrote into a block with a reached row"
    assert torch.equal(radii_early[~row_block_has], ref["radii"][~row_block_has])
    assert_same_forward(got, ref)


@pytest.mark.parametrize("P", [200, 256, 257, 2000, 60000])
def test_two_launches_leave_the_single_launch_forward(hip, P):
    """fewer rows than a block, exactly one, one row over, several blocks, and a size with reached and unreached blocks"""
    sc = walled(P) if P == 60000 else synthetic.trained_like(P, seed=4, sh_degree=3, knn=_knn)

    def want(has):
        if P == 60000:
            assert bool(has.any()) and not bool(has.all()), "the scene should hold both kinds of blocks"
    check_split(hip, sc, sc, want)


def test_block_zero_with_a_reached_row(hip):
    sc = reached_scenes.wall()   # rows: the opaque shells first, the hidden ball last

    def want(has):
        assert bool(has[0]) and not bool(has[-1])
    check_split(hip, sc, sc, want)


def test_block_zero_without_a_reached_row(hip):
    """the header words are the late launch's although its block 0 is filtered out"""
    sc = {k: (v.flip(0).contiguous() if torch.is_tensor(v) else v) for k, v in reached_scenes.wall().items()}

    def want(has):
        assert not bool(has[0]) and bool(has[-1])
    check_split(hip, sc, sc, want)


def test_every_block_reached_leaves_the_early_launch_empty(hip):
    sc = reached_scenes.haze()

    def want(has):
        assert bool(has.all())
    check_split(hip, sc, sc, want)


def test_no_block_reached_leaves_the_late_launch_empty(hip):
    sc = reached_scenes.haze()
    away = dict(sc, means3D=(sc["means3D"] + torch.tensor([0.0, 1.0e4, 0.0])).contiguous())   # nothing of it is on screen

    def want(has):
        assert not bool(has.any())
    check_split(hip, away, sc, want)


# ---------------------------------------------------------------------------------------------- 2. the train step
def make_trainer(hip, scene):
    import lgdwt_loss
    from gsplat_amd.trainer import GaussianModelLite, Trainer, camera_to, render
    sc = scene()
    cams = [camera_to(c, DEV) for c in reached_scenes.cameras()]
    g = torch.Generator().manual_seed(5)
    target = dict(sc, shs=sc["shs"] + 0.02 * torch.randn(sc["shs"].shape, generator=g))
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        tm = GaussianModelLite(target, DEV, api=hip.api)
        gts = [render(c, tm, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg)["render"].clone() for c in cams]
    model = GaussianModelLite(sc, DEV, api=hip.api)
    crit = lgdwt_loss.criterion(dwt_enable=True, patch_dwt_enable=True)
    tr = Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg, optimizer_step=True)
    tr.FUSED_STEP = True
    tr.depth_limit = "deferred"
    return tr


def trained_scene():
    return synthetic.trained_like(20000, seed=3, sh_degree=3, knn=_knn)


def walled_scene():
    return walled(20000, seed=3)   # (on the float4 grid: wall's own 2 503 rows are not, and the pass stays off there)


def run(hip, early, script, scene=walled_scene):
    """-> (what the run left: parameters, both moments, the three statistics, every loss; the pass's counters)"""
    hip.EARLY_GEOMETRY = early
    hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = True, 0
    hip._cam_cache.clear()
    hip._capacity_hint = hip._capacity_hint_limited = 0
    hip.drop_early_geometry()
    stats0 = dict(hip.early_geometry_stats)
    failed0 = hip.depth_limit_stats["failed"]
    tr = make_trainer(hip, scene)
    losses = [x.clone() for x in script(tr, hip)]
    tr.sync()
    torch.cuda.synchronize()
    m, o = tr.model, tr.model.optimizer
    out = dict(flat=m.flat.detach().clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
               max_radii2D=m.max_radii2D.clone(), xyz_gradient_accum=m.xyz_gradient_accum.clone(), denom=m.denom.clone(),
               losses=torch.stack([x.reshape(()) for x in losses]), t=o.t)
    stats = {k: hip.early_geometry_stats[k] - stats0[k] for k in stats0}
    stats["failed"] = hip.depth_limit_stats["failed"] - failed0
    has = blocks_with(hip.export_reached(m.P, hip._last.geom).cpu())   # (the last view's flags)
    stats["blocks"] = (int(has.sum()), int((~has).sum()))
    hip.drop_early_geometry()
    return out, stats


def assert_same_run(hip, script, scene=walled_scene, min_used=1, min_stale=0, min_failed=0, both_kinds=True):
    off, s_off = run(hip, False, script, scene)
    on, s_on = run(hip, True, script, scene)
    print("early geometry off", s_off, "on", s_on)
    if scene is walled_scene and both_kinds:   # (census of the LAST view's flags)
        assert min(s_on["blocks"]) > 0, "the scene should hold both kinds of blocks"
    assert s_off["issued"] == s_off["used"] == 0
    assert s_on["used"] >= min_used and s_on["stale"] >= min_stale and s_on["failed"] >= min_failed
    assert s_on["failed"] == s_off["failed"]
    assert on["t"] == off["t"]
    for k in off:
        if k != "t":
            assert on[k].shape == off[k].shape and torch.equal(on[k], off[k]), k


def plain(tr, hip):
    return [tr.step(k) for k in range(8)]   # cameras 0 1 2 0 1 2 0 1: limited from the second visit on


@pytest.mark.parametrize("scene", [walled_scene, trained_scene], ids=["walled", "trained_like"])
def test_trainer_with_the_early_pass_is_the_same_run(hip, scene):
    assert_same_run(hip, plain, scene, min_used=3)


def test_same_run_with_the_per_lane_kernel(hip):
    hip.region_coop = False
    assert_same_run(hip, plain, min_used=3)


def test_same_run_through_a_step_for_another_camera(hip):
    def script(tr, hip):
        out = [tr.step(k) for k in range(5)]        # step 4 starts camera 2's geometry ...
        out.append(tr.step(6))                      # ... and camera 0 comes
        return out + [tr.step(7), tr.step(8)]
    assert_same_run(hip, script, min_used=2, min_stale=1)


def test_same_run_through_limits_that_fail(hip):
    """camera 2's bounds cut everything: planted before the step that starts its geometry early, so the early and the late
    launch read the same table, the view fails its verdict and is stepped again with full lists; then planted once more behind
    an early pass that has read the old table (stale: the forward runs in full, fails, and is repeated)"""
    def script(tr, hip):
        out = [tr.step(k) for k in range(4)]
        tr.sync()
        hip.camera_entry(W, H, camera_key=("trainer", tr.uid, 2))["limit"].fill_(1e-3)
        out += [tr.step(4), tr.step(5), tr.step(6), tr.step(7)]
        tr.sync()
        hip.camera_entry(W, H, camera_key=("trainer", tr.uid, 2))["limit"].fill_(1e-3)
        return out + [tr.step(8), tr.step(9)]
    assert_same_run(hip, script, min_used=2, min_stale=1, min_failed=2)


def test_same_run_through_a_densification(hip):
    def script(tr, hip):
        out = [tr.step(k) for k in range(5)]
        tr.sync()
        n = tr.model.densify_and_prune(1e-7, 0.005, 2.0, None, generator=torch.Generator().manual_seed(9))
        assert n[0] + n[1] + n[2] > 0
        return out + [tr.step(k) for k in range(5, 8)]
    assert_same_run(hip, script, min_used=1, min_stale=1)


def test_same_run_through_an_opacity_reset(hip):
    def script(tr, hip):
        out = [tr.step(k) for k in range(5)]
        tr.sync()
        tr.model.reset_opacity()
        return out + [tr.step(k) for k in range(5, 8)]
    # (behind the reset nothing saturates: the shells are at 1 % opacity and every block of the last view holds a reached row)
    assert_same_run(hip, script, min_used=1, min_stale=1, both_kinds=False)
