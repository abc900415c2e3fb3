"""TrainerFSGS without a GPU: the loop of gsplat_amd.trainer on the CPU checker (un-fused path) against the literal
restatement of FSGS/train.py:81-176 (tests/fsgs_train_reference.py), on a compressed schedule that passes two densifications,
an opacity reset, SH increases, the depth_weight switch and several pseudo iterations inside 48 iterations."""
import pytest
import torch

import fsgs_loss_reference as flr
import fsgs_train_reference as ftr
from gsplat_amd import synthetic
from gsplat_amd.fsgs_criterion import FsgsCriterion
from gsplat_amd.losses import LossOps
from gsplat_amd.trainer import FsgsOptions, GaussianModelLite, TrainerFSGS, camera_to, cameras_extent
from helpers import TOL, rel_err

P0, W, H, N_ITERS, SEED = 240, 64, 48, 48, 2


def estimator(image):
    """stands for estimate_depth(render, mode='train'): any differentiable map image [3,H,W] -> depth [H,W]"""
    return 40.0 * image[0] - 25.0 * image[1] + 10.0 * image[2] * image[2] + 3.0


def inputs():
    dev = torch.device("cpu")
    sc = synthetic.trained_like(P0, seed=SEED, scale_mult=1.5)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:4]]
    pseudo = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[4:7]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g) for _ in cams]
    midas = [(1000.0 - 100.0 * (2.0 + 6.0 * torch.rand((H, W), generator=g))) for _ in cams]
    return sc, cams, pseudo, gts, midas


def options(cams, **kw):
    o = dict(iterations=60, position_lr_max_steps=60, densify_from_iter=10, densification_interval=12, densify_until_iter=30,
             prune_from_iter=15, proximity_until_iter=20, opacity_reset_interval=100, start_sample_pseudo=16, end_sample_pseudo=40,
             sample_pseudo_interval=4, sh_increase_interval=15, densify_grad_threshold=5.05e-6, seed=3,
             cameras_extent=cameras_extent([c.camera_center for c in cams]))
    o.update(kw)
    return FsgsOptions(**o)


def make_trainer(oracle, with_pseudo=True, **kw):
    sc, cams, pseudo, gts, midas = inputs()
    model = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    model.active_sh_degree = 0
    crit = FsgsCriterion(LossOps(oracle.api))
    assert not crit.fused   # (the checker has neither the partial-sum kernels nor the Pearson kernels: the un-fused path)
    return TrainerFSGS(model, cams, gts, midas, crit, torch.zeros(3), Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings,
                       pseudo_cameras=pseudo if with_pseudo else None, depth_estimator=estimator if with_pseudo else None,
                       pearson=flr.depth_pearson_loss, pseudo_pearson=flr.pseudo_depth_pearson_loss, **kw)


EVENT_KEYS = ("camera", "sh_degree", "xyz_lr", "depth_weight", "stepped", "densified", "reset", "pseudo")


def event(r):
    return dict(camera=r["camera"], sh_degree=r["sh_degree"], xyz_lr=r["xyz_lr"], depth_weight=r["depth_weight"],
                stepped=r["stepped"], densified=r["densified"] is not None, reset=r["reset"], pseudo=r["pseudo"])


@pytest.fixture(scope="module")
def runs(oracle):
    """the trainer, the float32 restatement and its float64 twin over the compressed schedule - computed once"""
    sc, cams, pseudo, gts, midas = inputs()
    opt = options(cams)
    tr = make_trainer(oracle)
    first = {}
    out = []
    for it in range(1, N_ITERS + 1):
        out.append(tr.train_iteration(it, opt))
        if it == 1:
            first["trainer"] = {k: v.grad.detach().clone().reshape(tr.model.P, -1) for k, v in tr.model.params.items()}

    def keep(it, model):
        if it == 1:
            first["reference"] = {k: v.detach().clone().reshape(model.P, -1) for k, v in model.grads().items()}
    ref32 = ftr.run(oracle, sc, cams, gts, midas, opt, N_ITERS, torch.float32, pseudo, estimator, after_backward=keep)
    ref64 = ftr.run(oracle, sc, cams, gts, midas, opt, N_ITERS, torch.float64, pseudo, estimator)
    return dict(trainer=tr, out=out, ref32=ref32, ref64=ref64, first=first, opt=opt)


def test_the_schedule_passes_every_event(runs):
    ev = [event(r) for r in runs["out"]]
    assert sum(e["densified"] for e in ev) == 2 and sum(e["reset"] for e in ev) == 1
    assert ev[-1]["sh_degree"] == 3 and ev[0]["sh_degree"] == 0
    assert sum(e["pseudo"] for e in ev) >= 4
    assert {e["depth_weight"] for e in ev} == {0.05, 0.001}
    # depth_weight falls AFTER the loss of the first iteration beyond end_sample_pseudo: that iteration still used 0.05
    assert ev[40]["depth_weight"] == 0.05 and ev[41]["depth_weight"] == 0.001
    assert ev[0]["xyz_lr"] == 0.00016 and ev[1]["xyz_lr"] < ev[0]["xyz_lr"]      # the step of iteration k uses the rate of k - 1
    assert not any(e["stepped"] and e["densified"] for e in ev)
    assert all(r["path"] == "unfused" for r in runs["out"])
    counts = [r["densified"] for r in runs["out"] if r["densified"] is not None]
    print("densifications (clone, split, proximity, pruned):", counts)
    assert counts[0][3] == 0 and counts[1][2] == 0     # first: no prune yet; second: proximity is over
    assert sum(c[0] + c[1] for c in counts) > 0


def test_the_event_trace_is_the_restatements(runs):
    got = [event(r) for r in runs["out"]]
    for name in ("ref32", "ref64"):
        want = [{k: e[k] for k in EVENT_KEYS} for e in runs[name]["trace"]]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]


def test_P_after_each_densification_is_the_restatements(runs):
    # the margin condition of tests/test_densify_device_cpu.py, asserted on the float64 twin: no decision value of any
    # densification lies within 1e-5 relative of its threshold, so no row is exempt (count of exempted rows: 0)
    assert len(runs["ref64"]["margins"]) == 2 and min(runs["ref64"]["margins"]) > 1e-5, runs["ref64"]["margins"]
    got = [r["P"] for r in runs["out"] if r["densified"] is not None]
    assert got == runs["ref32"]["P_after_densify"] == runs["ref64"]["P_after_densify"]
    assert got[0] != P0


def test_the_gradients_of_one_iteration_are_the_restatements(runs):
    got, want = runs["first"]["trainer"], runs["first"]["reference"]
    for k in want:
        e = rel_err(got[k], want[k])
        print("dL/d%-9s rel err %.2e" % (k, e))
        assert float(want[k].abs().max()) > 0 and e <= TOL, (k, e)


def test_the_parameters_after_the_run_lie_within_the_restatements_own_rounding(runs):
    tr = runs["trainer"]
    f32, f64 = runs["ref32"]["model"].flat().double(), runs["ref64"]["model"].flat()
    got = tr.model.flat.detach().double()
    assert got.shape == f32.shape == f64.shape
    own = float((f32 - f64).pow(2).mean().sqrt())
    dist = float((got - f32).pow(2).mean().sqrt())
    print("rms(float32 restatement - float64 twin) = %.3e, rms(trainer - float32 restatement) = %.3e" % (own, dist))
    assert own > 0 and dist <= 4.0 * own, (dist, own)


@pytest.mark.parametrize("kind", ["A", "B"])
def test_the_unfused_criterion_is_the_restatements_loss(oracle, kind):
    g = torch.Generator().manual_seed(11)
    gt = torch.rand((3, H, W), generator=g)
    img = (gt + 0.2 * torch.randn((3, H, W), generator=g)).requires_grad_(True)   # (leaves [0, 1]: nothing clamps)
    x, m = flr.scene(H, W, kind, 3, dtype=torch.float32)
    depth = x.reshape(1, H, W).clone().requires_grad_(True)
    crit = FsgsCriterion(LossOps(oracle.api), pearson=flr.depth_pearson_loss)
    loss, parts = crit(img, depth, gt, m, 0.05)
    loss.backward()
    i64, d64 = img.detach().double().requires_grad_(True), depth.detach().double().requires_grad_(True)
    want, branch = ftr.train_loss(i64, d64[0], gt.double(), m.double(), 0.05)
    want.backward()
    assert branch == (0 if kind == "A" else 1)
    assert abs(float(loss.detach()) - float(want.detach())) <= TOL * abs(float(want.detach()))
    assert rel_err(img.grad, i64.grad) <= TOL and rel_err(depth.grad, d64.grad) <= TOL
    assert float(d64.grad.abs().max()) > 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        FsgsCriterion(LossOps(oracle.api))(img, depth, gt, m, 0.05)
    with pytest.raises(RuntimeError, match="no fallback"):
        crit.fused_call(img, depth, gt, m, 0.05)


def test_what_is_closed_to_this_trainer_raises_at_construction(oracle):
    with pytest.raises(RuntimeError, match="world_size"):
        make_trainer(oracle, world_size=2)
    with pytest.raises(RuntimeError, match="alpha masks"):
        make_trainer(oracle, alpha_masks=[None] * 4)
    with pytest.raises(RuntimeError, match="depth_limit"):
        make_trainer(oracle, depth_limit="deferred")
    with pytest.raises(RuntimeError, match="sparse_adam"):
        make_trainer(oracle, optimizer_type="sparse_adam")
    sc, cams, pseudo, gts, midas = inputs()
    crit = FsgsCriterion(LossOps(oracle.api))
    nir = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api, with_nir=True)
    with pytest.raises(RuntimeError, match="with_nir"):
        TrainerFSGS(nir, cams, gts, midas, crit, torch.zeros(3), Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings)
    exp = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    exp.enable_exposure(len(cams))
    with pytest.raises(RuntimeError, match="exposure"):
        TrainerFSGS(exp, cams, gts, midas, crit, torch.zeros(3), Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings)
    tr = make_trainer(oracle)
    with pytest.raises(RuntimeError, match="depth_limit"):
        tr.depth_limit = "deferred"
    from gsplat_amd.trainer import GraphedStep
    with pytest.raises(RuntimeError, match="GraphedStep"):
        GraphedStep(tr)
    with pytest.raises(ValueError):
        TrainerFSGS(GaussianModelLite(sc, torch.device("cpu"), api=oracle.api), cams, gts, midas[:2], crit, torch.zeros(3),
                    Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings)


def test_without_an_estimator_the_pseudo_leg_is_off(oracle):
    tr = make_trainer(oracle, with_pseudo=False)
    _, cams, _, _, _ = inputs()
    opt = options(cams)
    assert not tr.pseudo_on()
    out = [tr.train_iteration(it, opt) for it in range(1, 22)]
    assert not any(r["pseudo"] for r in out) and out[19]["stepped"]


def test_the_options_carry_the_references_defaults():
    o = FsgsOptions()
    assert (o.iterations, o.position_lr_max_steps, o.densify_until_iter, o.densify_grad_threshold, o.min_opacity, o.prune_from_iter,
            o.dist_thres, o.start_sample_pseudo, o.end_sample_pseudo, o.sample_pseudo_interval, o.depth_weight,
            o.depth_pseudo_weight, o.sh_increase_interval, o.densify_rule) == \
        (10_000, 10_000, 10_000, 5e-4, 0.005, 500, 10.0, 2000, 9500, 10, 0.05, 0.5, 500, "fsgs")
    assert (o.densification_interval, o.opacity_reset_interval, o.densify_from_iter, o.proximity_until_iter) == (100, 3000, 500, 2000)
    with pytest.raises(TypeError):
        FsgsOptions(depth_weights=1.0)


def test_the_new_entry_point_is_declared_everywhere():
    import os
    import re
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gsplat.h")).read(), flags=re.S)
    assert "backward_step_fsgs" in PROTOTYPES and "backward_step_fsgs" in DEVICE_ONLY
    decl = re.search(r"\bgs_backward_step_fsgs\s*\(([^;]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == len(PROTOTYPES["backward_step_fsgs"][1])
