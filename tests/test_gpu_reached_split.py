"""The reached split (GsStepState.reached_split): the forward blend leaves one byte per Gaussian saying whether the backward
blend will visit one of its list entries, and the fused step's tail - chain kernel, per-Gaussian kernel, side-stream Adam -
counts only those as "instanced".  Checked here: the flags against the exported lists (exact and tight), and the train step
with the split against the step without it, bit for bit, on constructed scenes (tests/reached_scenes.py).

Figures of one run on an MI355X (each test prints its own): wall, culled lists: 2 350 accepted and listed, 137-186 reached per
camera; depth-limited: 215-275 accepted, the same 137-186 reached; haze: 2 064-2 086 listed = reached; 4 of 10 dormant blocks
standing after the wall's steps in either form."""
import pytest
import torch

import diff_gaussian_rasterization as dgr
import lgdwt_loss
import reached_scenes as rs
from gsplat_amd.losses import LossOps
from gsplat_amd.trainer import GaussianModelLite, GraphedStep, NirCriterion, Trainer, TrainerNIR, camera_to
from test_gpu_raster_parity import forward_state

pytestmark = pytest.mark.gpu

SCENES = {"wall": rs.wall, "haze": rs.haze}


@pytest.fixture(autouse=True)
def pinned_backend(hip):
    """Region binning, culled lists, small scenes through the two-phase step; everything put back afterwards."""
    old = (hip.binning, hip._capacity_hint, hip._capacity_hint_limited, hip.tile_cull, hip.depth_limit_on)
    hip.binning, hip.tile_cull = "region", True
    hip._cam_cache.clear()
    yield
    hip.binning, hip._capacity_hint, hip._capacity_hint_limited, hip.tile_cull, hip.depth_limit_on = old
    for k in ("TWO_PHASE", "TWO_PHASE_MIN_P", "REACHED_SPLIT"):
        hip.__dict__.pop(k, None)     # (back to the class defaults)
    hip._cam_cache.clear()


# ---------------------------------------------------------------------------------------------------------------- the flags
@pytest.fixture(scope="module")
def scenes():
    return {k: f() for k, f in SCENES.items()}


def _forward_with_flags(hip, sc, cam):
    dev = torch.device("cuda")
    buf = {}
    st = forward_state(hip, sc, cam, dev, torch.zeros(3), False, buffers=buf)
    return st, hip.export_reached(rs.P, buf["geom"]).cpu().bool()


@pytest.mark.parametrize("lists", ["culled", "depth_limited"])
@pytest.mark.parametrize("scene", ["wall", "haze"])
def test_flags_are_exact_and_tight(hip, scenes, scene, lists):
    """Every Gaussian with a list entry in front of its tile's largest n_contrib is marked (no tolerance: its row can be
    non-zero), and none is marked without an entry at a position <= that bound in some tile."""
    sc = scenes[scene]
    hip.depth_limit_on = lists == "depth_limited"
    for ci, cam in enumerate(rs.cameras()):
        st, reached = _forward_with_flags(hip, sc, cam)
        if lists == "depth_limited":    # (the first visit measured the stop depths: the second one's lists are cut)
            full_R = st["num_rendered"]
            st, reached = _forward_with_flags(hip, sc, cam)
            assert st["num_rendered"] <= full_R
            if scene == "wall":
                assert st["num_rendered"] < full_R
        must, may, listed = rs.list_sets(st, rs.P)
        accepted = st["tiles_touched"] > 0
        print("%s %s camera %d: accepted %d listed %d reached %d (must %d, may %d)" % (
            scene, lists, ci, int(accepted.sum()), int(listed.sum()), int(reached.sum()), int(must.sum()), int(may.sum())))
        assert bool((reached | ~must).all()), "a Gaussian the backward blend visits is not marked: %d" % int((must & ~reached).sum())
        assert bool((may | ~reached).all()), "marked without an entry up to its tile's bound: %d" % int((reached & ~may).sum())
        assert bool((accepted | ~listed).all()) and int(must.sum()) > 0
        if scene == "haze":   # nothing saturates: every list is walked to its end, the split is a no-op
            assert float(st["final_T"].min()) > 0.05
            assert torch.equal(reached, listed)
        elif lists == "culled":
            # the ball behind the shells: accepted, listed, never reached - and with the shells' far side well over a quarter
            # of the accepted Gaussians
            back = torch.arange(rs.P) >= rs.N_SHELL
            assert bool(accepted[back].all()) and bool(listed[back].all()) and not bool(reached[back].any())
            assert int((accepted & ~reached).sum()) >= 0.25 * int(accepted.sum())


# ---------------------------------------------------------------------------------------------------------------- the steps
def _trainer(hip, sc, nir=False):
    dev = torch.device("cuda")
    cams = [camera_to(c, dev) for c in rs.cameras()]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, rs.H, rs.W), generator=g).to(dev) for _ in cams]
    bg = torch.zeros(3, device=dev)
    if nir:
        nirs = [torch.rand((1, rs.H, rs.W), generator=g).to(dev) for _ in cams]
        model = GaussianModelLite(sc, dev, api=hip.api, with_nir=True)
        return TrainerNIR(model, cams, gts, nirs, NirCriterion(LossOps(hip.api), fused=True), dgr.GaussianRasterizationSettings, bg)
    model = GaussianModelLite(sc, dev, api=hip.api)
    crit = lgdwt_loss.criterion(dwt_enable=True, patch_dwt_enable=True)
    tr = Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg, optimizer_step=True)
    tr.FUSED_STEP = True
    return tr


def _state(tr):
    m, o = tr.model, tr.model.optimizer
    s = dict(flat=m.flat.detach().clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
             accum=m.xyz_gradient_accum.clone(), denom=m.denom.clone(), max_radii=m.max_radii2D.clone())
    if m.nir_gain is not None:
        gs = m.nir_gain_optimizer.state[m.nir_gain]
        s.update(gain=m.nir_gain.detach().clone().reshape(1), gain_m=gs["exp_avg"].clone().reshape(1),
                 gain_v=gs["exp_avg_sq"].clone().reshape(1))
    return s


def _run(hip, sc, steps, split, two_phase, deferred, nir=False):
    hip._cam_cache.clear()
    hip.REACHED_SPLIT, hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = split, two_phase, 0
    tr = _trainer(hip, sc, nir)
    if deferred:
        tr.depth_limit = "deferred"
    n0 = hip.two_phase_launches
    losses = [tr.step(k) for k in range(steps)]
    tr.sync()
    torch.cuda.synchronize()
    assert (hip.two_phase_launches - n0 >= steps) == two_phase
    s = _state(tr)
    s["losses"] = torch.tensor([float(x) for x in losses])
    opt = tr.model.optimizer
    kept = opt.dormant_flags().clone()       # maintained by the kernels
    opt.invalidate_dormant()
    derived = opt.dormant_flags().clone()    # recomputed from the moments
    assert bool(((kept == 0) | (derived == 1)).all()), "a block is flagged dormant although one of its moments is not +0"
    return s, int(kept.sum())


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


# (scene, steps over the three cameras, depth limits): the wall on full lists; the haze; the wall again with the second and the
# third visit of every camera on depth-limited lists
CASES = {"wall": ("wall", 6, False), "haze": ("haze", 6, False), "wall_depth_limited": ("wall", 9, True)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_steps_with_the_split_leave_the_bits_of_the_steps_without(hip, scenes, case):
    """Parameters, both moments, the densification statistics and the losses of steps with the split (two-phase) against
    the same steps with GS_REACHED_SPLIT=0's definition (two-phase) and against the one-launch form: torch.equal."""
    scene, steps, deferred = CASES[case]
    sc = scenes[scene]
    on, dormant_on = _run(hip, sc, steps, True, True, deferred)
    off, dormant_off = _run(hip, sc, steps, False, True, deferred)
    one, _ = _run(hip, sc, steps, True, False, deferred)
    print("%s: dormant blocks standing %d (split) / %d (no split) of %d, denom max %.0f" % (
        case, dormant_on, dormant_off, (rs.P + 255) // 256, float(on["denom"].max())))
    _same(on, off, "split on / off")
    _same(on, one, "two-phase split / one launch")
    assert float(on["denom"].max()) == steps and float(on["exp_avg"].abs().max()) > 0
    if scene == "wall":   # the blocks that hold nothing but the ball never see a gradient: their flags stand in either form
        assert dormant_on >= 1 and dormant_off >= 1


def test_fourth_channel_step_with_the_split(hip, scenes):
    """The multispectral fused step (gs_backward_step_x: sixth row, gain from the chain kernel's partial sums) on the wall."""
    on, _ = _run(hip, scenes["wall"], 6, True, True, False, nir=True)
    off, _ = _run(hip, scenes["wall"], 6, False, True, False, nir=True)
    _same(on, off, "split on / off, four channels")
    assert float(on["gain"]) != 1.0 and float(on["denom"].max()) == 6.0


def test_a_failed_forward_changes_nothing_with_the_split(hip, scenes):
    """Binning capacity far too small (capture-safe form: fixed capacity, no re-run): the forward flags overflow, blends
    nothing and marks nothing, both phases are no-ops on the device - the trainer keeps its bits and trains on like a twin that
    never met the failure."""
    hip.REACHED_SPLIT, hip.TWO_PHASE, hip.TWO_PHASE_MIN_P = True, True, 0
    a, b = _trainer(hip, scenes["wall"]), _trainer(hip, scenes["wall"])
    a.step(0)
    b.step(0)
    a.sync(); b.sync()
    before = _state(a)
    opt = a.model.optimizer
    counters = (opt.t, dict(opt.seg_steps))
    rm0 = a.criterion.dwt_running_mean.clone()     # (the criterion's running mean sees the failed view's empty image)
    gs = GraphedStep(a, capacity=64)
    gs._shared_init(a.model.flat.device)
    gs.capacity = 64
    gs._coef_for_next()
    gs._one_step(1)
    torch.cuda.synchronize()
    status = hip.last_status()
    assert status[1] != 0, status     # overflow
    after = _state(a)
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    opt.t, opt.seg_steps = counters[0], dict(counters[1])   # (what GraphedStep puts back after such a step)
    a.criterion.dwt_running_mean.copy_(rm0)
    for k in (1, 2, 3):
        a.step(k)
        b.step(k)
    a.sync(); b.sync()
    torch.cuda.synchronize()
    _same(_state(a), _state(b), "after the failed step")
