"""TrainerDNG on the GPU: the compressed schedule of tests/test_dng_trainer_cpu.py with the real dng_neural.GridRenderer and
the HIP kernels for every piece.  The fused depth legs (gs_depth_backward_step) against the un-fused ones from the same state,
bit for bit; the un-fused HIP gradients of an iteration against the CPU restatement; render_dng against the rasterizer called
by hand; evaluate() and a checkpoint round trip."""
import copy

import pytest
import torch

import depth_pass_reference as dpr
import dgr_dng
import dng_train_reference as dtr
import test_dng_trainer_cpu as cpu
from gsplat_amd.trainer import GaussianModelLite, TrainerDNG, _settings_of, camera_to, render_dng
from helpers import TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def gpu_inputs():
    sc, cams, gts, mono = cpu.inputs()
    return sc, [camera_to(c, DEV) for c in cams], [g.to(DEV) for g in gts], [m.to(DEV) for m in mono]


def make_trainer(hip, neural=None, **kw):
    sc, cams, gts, mono = gpu_inputs()
    model = GaussianModelLite(sc, DEV, api=hip.api)
    model.active_sh_degree = 0
    return TrainerDNG(model, cams, gts, mono, neural=neural, near_centers=cpu.NEAR_CENTERS, near_range=0.0, **kw)


def state_of(tr):
    m, o = tr.model, tr.model.optimizer
    out = dict(flat=m.flat, exp_avg=o.exp_avg, exp_avg_sq=o.exp_avg_sq, accum=m.xyz_gradient_accum, denom=m.denom,
               max_radii2D=m.max_radii2D)
    out.update({"neural%d" % i: p for i, p in enumerate(tr.neural_parameters())})
    for i, p in enumerate(tr.neural_parameters()):
        st = tr.neural_optimizer.state.get(p, {})
        if "exp_avg" in st:
            out["neural%d_m" % i], out["neural%d_v" % i] = st["exp_avg"], st["exp_avg_sq"]
    return {k: v.detach().clone() for k, v in out.items()}


def assert_same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        n = int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum())
        assert n == 0, "%s: %s differs in %d of %d elements (max %.3e)" % (what, k, n, a[k].numel(),
                                                                            float((a[k] - b[k]).abs().max()))


def run_schedule(tr, opt, n):
    out = []
    for it in range(1, n + 1):
        tr.near_range = cpu.near_range(it)
        out.append(tr.train_iteration(it, opt))
    return out


def test_fused_depth_legs_are_the_unfused_ones_bit_for_bit(hip):
    """the whole compressed schedule twice from the same state: parameters, moments, neural parameters and their moments,
    statistics, P and the step counts after the run are the same bits, and `path` says which leg ran which way"""
    _, cams, _, _ = gpu_inputs()
    a = make_trainer(hip)
    b = make_trainer(hip, neural=copy.deepcopy(a.neural))
    assert a.fused_legs_available()
    assert_same_bits(state_of(a), state_of(b), "before the run")
    ra = run_schedule(a, cpu.options(cams, fused_depth_legs=True), cpu.N_ITERS)
    rb = run_schedule(b, cpu.options(cams, fused_depth_legs=False), cpu.N_ITERS)
    for it, (x, y) in enumerate(zip(ra, rb), 1):
        soft = x["loss_soft"] is not None
        last = it == cpu.N_ITERS    # no step on the last iteration: nothing to fuse
        assert x["path"] == dict(hard="unfused" if last else "fused", soft=("unfused" if last else "fused") if soft else None), (it, x["path"])
        assert y["path"] == dict(hard="unfused", soft="unfused" if soft else None), (it, y["path"])
        for k in ("camera", "patches", "xyz_lr", "stepped", "densified", "near_pruned", "cleaned", "P"):
            assert x[k] == y[k], (it, k, x[k], y[k])
        assert float(x["loss_hard"]) == float(y["loss_hard"]), it
    assert [it for it, r in enumerate(ra, 1) if r["densified"] is not None] == [20, 30]
    assert ra[16]["near_pruned"] == 0 and ra[32]["near_pruned"] > 0
    assert a.model.P == b.model.P != cpu.P0
    assert dict(a.model.optimizer.seg_steps) == dict(b.model.optimizer.seg_steps)
    assert a.model.optimizer.seg_steps["xyz"] > a.model.optimizer.seg_steps["scaling"] > 0
    assert_same_bits(state_of(a), state_of(b), "after %d iterations" % cpu.N_ITERS)


def test_the_unfused_hip_gradients_are_the_cpu_restatements(hip, oracle):
    """one iteration with all three legs on: the gradients behind each un-fused backward on the GPU (xyz after the hard leg,
    opacity after the soft leg, every tensor after the photometric leg) within helpers.TOL of the float32 CPU restatement, the
    stand-in grid on both sides"""
    sc, cams, gts, mono = cpu.inputs()
    opt = cpu.options(cams, fused_depth_legs=False, soft_depth_start=0)   # all three legs in the first iteration
    tr = make_trainer(hip, neural=dtr.stand_in_for(sc).to(DEV))
    got, want = {}, {}

    def keep(leg, trainer):
        got[leg] = {k: v.grad.detach().cpu().reshape(trainer.model.P, -1) for k, v in trainer.model.params.items() if v.grad is not None}
        got[leg].update({"neural%d" % i: p.grad.detach().cpu() for i, p in enumerate(trainer.neural_parameters()) if p.grad is not None})
    tr.after_backward = keep
    tr.train_iteration(1, opt)

    def keep_ref(leg, it, ref, neural):
        want[leg] = {k: v.grad.detach().clone().reshape(ref.P, -1) for k, v in ref.p.items() if v.grad is not None}
        want[leg].update({"neural%d" % i: p.grad.detach().clone() for i, p in enumerate(neural.parameters()) if p.grad is not None})
    # the checker in its exact-transmittance form, the arbiter of every GPU comparison of this rasterizer generation
    # (tests/depth_pass_reference.exact_T: the reference's `1 - alpha` read-back cancels in fp32 on saturated pixels)
    with dpr.exact_T(oracle):
        dtr.run(oracle, sc, cams, gts, mono, opt, 1, torch.float32, near_centers=cpu.NEAR_CENTERS, near_range=0.0,
                after_backward=keep_ref)
    assert set(got) == set(want) == {"hard", "soft", "photometric"}
    assert set(want["hard"]) == {"xyz"} and set(want["soft"]) == {"opacity"}
    for leg in ("hard", "soft", "photometric"):
        assert set(got[leg]) == set(want[leg]), (leg, set(got[leg]) ^ set(want[leg]))
        for k, w in want[leg].items():
            e = rel_err(got[leg][k], w)
            print("%-11s dL/d%-9s rel err %.2e" % (leg, k, e))
            assert float(w.abs().max()) > 0 and e <= TOL, (leg, k, e)


def test_render_dng_is_the_rasterizer_called_by_hand(hip):
    tr = make_trainer(hip)
    m, cam = tr.model, tr.cameras[2]
    with torch.no_grad():
        pkg = render_dng(cam, m, tr.neural, dgr_dng.GaussianRasterizer, dgr_dng.GaussianRasterizationSettings, tr.bg)
        assert set(pkg) == {"render", "depth", "alpha", "viewspace_points", "visibility_filter", "radii", "opacity", "color"}
        rs = _settings_of(dgr_dng.GaussianRasterizationSettings, cam, tr.bg, 0, m.P)
        image, radii, depth, alpha = dgr_dng.GaussianRasterizer(raster_settings=rs)(
            means3D=m.get_xyz, means2D=torch.zeros_like(m.get_xyz), shs=None, colors_precomp=pkg["color"], opacities=m.get_opacity,
            scales=m.get_scaling, rotations=m.get_rotation, cov3D_precomp=None)
    assert pkg["render"].shape == (3, cpu.H, cpu.W)
    for k, t in (("render", image), ("depth", depth), ("alpha", alpha), ("radii", radii)):
        assert torch.equal(pkg[k], t), k
    assert torch.equal(pkg["visibility_filter"], radii > 0) and torch.equal(pkg["opacity"], m.get_opacity)
    assert float(pkg["render"].max()) > 0 and int((radii > 0).sum()) > 0
    # sigma is never used (combine_opacity returns the model's own opacity): no gradient reaches its column
    m.zero_grad()
    pkg = render_dng(cam, m, tr.neural, dgr_dng.GaussianRasterizer, dgr_dng.GaussianRasterizationSettings, tr.bg)
    pkg["render"].sum().backward()
    last = tr.neural.sigma_net.net[-1].weight.grad
    assert float(last[0].abs().max()) == 0 and float(last[1:].abs().max()) > 0
    assert float(m.params["opacity"].grad.abs().max()) > 0 and m.params["features"].grad is None


def test_evaluate_and_a_checkpoint_round_trip(hip):
    """five iterations, a checkpoint, an evaluation, iteration 6; a second trainer restored from the checkpoint runs iteration 6
    to the same bits - evaluate() touched nothing the loop reads"""
    _, cams, _, _ = gpu_inputs()
    opt = cpu.options(cams, soft_depth_start=2)
    a = make_trainer(hip)
    run_schedule(a, opt, 5)
    ck = a.checkpoint()
    before = state_of(a)
    res = a.evaluate()
    assert set(res) >= {"PSNR", "SSIM", "L1"} and res["PSNR"] > 0
    assert_same_bits(before, state_of(a), "evaluate()")
    ra = a.train_iteration(6, opt)
    b = make_trainer(hip, neural=copy.deepcopy(a.neural))
    b.restore(ck)
    rb = b.train_iteration(6, opt)
    for k in ("camera", "patches", "xyz_lr", "stepped", "P", "path"):
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert dict(a.model.optimizer.seg_steps) == dict(b.model.optimizer.seg_steps)
    assert_same_bits(state_of(a), state_of(b), "iteration 6 after the round trip")
