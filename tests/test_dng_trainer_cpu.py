"""TrainerDNG without a GPU: the loop of gsplat_amd.trainer on the CPU checker (un-fused legs through the given rasterizer)
against the literal restatement of DNGaussian/train_llff.py:68-228 (tests/dng_train_reference.py) and its float64 twin, on a
schedule compressed into 48 iterations: hard-leg-only iterations, the soft leg's start, the smoothness term's start, two
densifications, a near-camera prune with an empty mask and one that removes rows, the clean at iteration 1, and the last
iteration, which steps nothing."""
import pytest
import torch

import dng_depth_reference as depr
import dng_reg_reference as rgr
import dng_train_reference as dtr
from gsplat_amd import synthetic
from gsplat_amd.trainer import DngOptions, GaussianModelLite, TrainerDNG, camera_to, cameras_extent
from helpers import TOL, rel_err

P0, W, H, N_ITERS, SEED = 240, 64, 48, 48, 2
NEAR_CENTERS = torch.tensor([[0.9, 0.9, 0.9], [-1.0, 0.5, 0.0]])
EVENT_KEYS = ("camera", "patches", "xyz_lr", "stepped", "densified", "near_pruned", "cleaned", "P")


def near_range(iteration):
    """the first near-camera prune of the schedule (iteration 17) meets an empty mask, the second (33) removes rows"""
    return 0.0 if iteration < 20 else 0.45


def inputs():
    dev = torch.device("cpu")
    sc = synthetic.trained_like(P0, seed=SEED, scale_mult=1.5)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:4]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g) for _ in cams]
    mono = [depr.scene(H, W, 20 + i, dtype=torch.float32)[1].reshape(H, W).clamp(0, 255) for i in range(len(cams))]
    mono = [255.0 - m for m in mono]   # as stored: the loop forms 255 - depth_mono
    return sc, cams, gts, mono


def options(cams, **kw):
    o = dict(iterations=48, position_lr_max_steps=48, hard_depth_start=0, soft_depth_start=6, smooth_start=10,
             densify_from_iter=12, densification_interval=10, densify_until_iter=35, near_prune_interval=16, near_prune_start=15,
             clean_iterations=[6000, 1], densify_grad_threshold=GRAD_THRESHOLD, seed=3,
             cameras_extent=cameras_extent([c.camera_center for c in cams]))
    o.update(kw)
    return DngOptions(**o)


# in a gap of the float64 twin's statistic at both densifications (test_P_after_each_densification prints the neighbours)
GRAD_THRESHOLD = 1.02e-6


def regulariser(scaling, opacity, shape_pena, scale_pena, opa_pena):
    t = rgr.terms(scaling, opacity)
    return shape_pena * t[0] + scale_pena * t[1] + opa_pena * t[2]


def make_trainer(oracle, **kw):
    sc, cams, gts, mono = inputs()
    model = kw.pop("model", None) or GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    model.active_sh_degree = 0
    return TrainerDNG(model, cams, gts, mono, neural=dtr.stand_in_for(sc), near_centers=NEAR_CENTERS, near_range=0.0,
                      bg=torch.zeros(3), Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings,
                      depth_loss=depr.depth_regulariser, regulariser=regulariser, view_dirs=rgr.view_dirs, **kw)


def event(r):
    return dict(camera=r["camera"], patches=tuple(r["patches"]), xyz_lr=r["xyz_lr"], stepped=dict(r["stepped"]),
                densified=r["densified"] is not None, near_pruned=r["near_pruned"] is not None, cleaned=r["cleaned"] is not None,
                P=r["P"])


def rows(model):
    o = model.optimizer
    return [t.detach().clone() for t in (model.flat, o.exp_avg, o.exp_avg_sq)]


@pytest.fixture(scope="module")
def runs(oracle):
    """the trainer, the float32 restatement and its float64 twin over the compressed schedule - computed once"""
    sc, cams, gts, mono = inputs()
    opt = options(cams)
    tr = make_trainer(oracle)
    first, out, relayout = {"trainer": {}, "reference": {}}, [], []
    it_now = [0]

    def keep_trainer(leg, trainer):
        if it_now[0] == 1:
            first["trainer"][leg] = {k: (v.grad.detach().clone().reshape(trainer.model.P, -1) if v.grad is not None else None)
                                     for k, v in trainer.model.params.items()}
            first["trainer"][leg].update({"neural%d" % i: (p.grad.detach().clone() if p.grad is not None else None)
                                          for i, p in enumerate(trainer.neural_parameters())})
    tr.after_backward = keep_trainer
    for it in range(1, N_ITERS + 1):
        it_now[0] = it
        tr.near_range = near_range(it)
        before, neural_before, P_before = rows(tr.model), [p.detach().clone() for p in tr.neural_parameters()], tr.model.P
        r = tr.train_iteration(it, opt)
        out.append(r)
        if (r["densified"] is not None or r["near_pruned"] is not None or r["cleaned"] is not None) and r["P"] == P_before \
                and it < opt.iterations:
            # a re-layout that left the rows where they were: the Gaussian rows must come through the step untouched
            relayout.append((it, before, rows(tr.model), neural_before, [p.detach().clone() for p in tr.neural_parameters()]))

    def keep_reference(leg, it, ref, neural):
        if it == 1:
            first["reference"][leg] = {k: (v.grad.detach().clone().reshape(ref.P, -1) if v.grad is not None else None)
                                       for k, v in ref.p.items()}
            first["reference"][leg].update({"neural%d" % i: (p.grad.detach().clone() if p.grad is not None else None)
                                            for i, p in enumerate(neural.parameters())})
    common = dict(near_centers=NEAR_CENTERS, near_range=near_range)
    ref32 = dtr.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float32, after_backward=keep_reference, **common)
    ref64 = dtr.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float64, **common)
    return dict(trainer=tr, out=out, ref32=ref32, ref64=ref64, first=first, opt=opt, relayout=relayout)


def test_the_schedule_passes_every_event(runs):
    out = runs["out"]
    ev = [event(r) for r in out]
    assert all(r["loss_soft"] is None and r["patches"][2:] == (None, None) for r in out[:6]) and out[6]["loss_soft"] is not None
    assert all(r["loss_hard"] is not None for r in out)
    assert [i + 1 for i, e in enumerate(ev) if e["densified"]] == [20, 30]
    assert [i + 1 for i, e in enumerate(ev) if e["near_pruned"]] == [17, 33]
    assert out[16]["near_pruned"] == 0 and out[32]["near_pruned"] > 0, (out[16]["near_pruned"], out[32]["near_pruned"])
    assert [i + 1 for i, e in enumerate(ev) if e["cleaned"]] == [1]
    for it in (1, 17, 20, 30, 33):   # a re-layout - the empty prune too - cancels the Gaussian groups' step, not the neural one
        s = ev[it - 1]["stepped"]
        assert s["hard"] and not s["gaussians"] and s["neural"], (it, s)
    assert ev[1]["stepped"] == dict(hard=True, soft=False, gaussians=True, neural=True)
    assert ev[7]["stepped"] == dict(hard=True, soft=True, gaussians=True, neural=True)
    assert ev[-1]["stepped"] == dict(hard=False, soft=False, gaussians=False, neural=False)   # the last iteration: no step at all
    assert ev[0]["xyz_lr"] < 0.00016 and ev[0]["xyz_lr"] > ev[1]["xyz_lr"]   # the rate of iteration k, set BEFORE its steps
    assert all(p is None or 5 <= p <= 17 for e in ev for p in e["patches"])
    assert all(r["path"] == dict(hard="unfused", soft="unfused" if r["loss_soft"] is not None else None) for r in out)
    counts = [r["densified"] for r in out if r["densified"] is not None]
    print("densifications (outliers, clone, split, pruned):", counts)
    assert sum(c[1] + c[2] for c in counts) > 0


def test_the_event_trace_is_the_restatements(runs):
    got = [event(r) for r in runs["out"]]
    for name in ("ref32", "ref64"):
        want = [{k: e[k] for k in EVENT_KEYS} for e in runs[name]["trace"]]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]


def test_the_step_counts_are_the_restatements(runs):
    tr = runs["trainer"]
    got = {k: tr.model.optimizer.seg_steps[k] for k in ("xyz", "opacity", "scaling", "rotation", "features")}
    neural = [int(tr.neural_optimizer.state[p]["step"]) for p in tr.neural_parameters()]
    print("Adam step counts:", got, "neural:", neural)
    for name in ("ref32", "ref64"):
        assert got == {k: runs[name]["steps"][k] for k in got}, (name, got, runs[name]["steps"])
        assert neural == runs[name]["neural_steps"]
    assert got["features"] == 0
    assert got["xyz"] == 47 + 42 and got["opacity"] == 41 + 42 and got["scaling"] == got["rotation"] == 42
    assert neural == [47] * 6   # ahead of scaling / rotation by the five re-layouts


def test_P_after_each_densification_is_the_restatements(runs):
    """the margin condition, asserted on the float64 twin: no decision value of either densification lies within 1e-5
    relative of its threshold, no row exempt"""
    r64 = runs["ref64"]
    for g in r64["statistic"]:
        thr = runs["opt"].densify_grad_threshold
        below, above = g[g < thr], g[g >= thr]
        print("statistic: %d rows, nearest below %.6e, threshold %.6e, nearest above %.6e"
              % (g.numel(), float(below.max()) if below.numel() else float("nan"), thr, float(above.min()) if above.numel() else float("nan")))
    assert len(r64["margins"]) == 2 and min(r64["margins"]) > 1e-5, r64["margins"]
    got = [r["P"] for r in runs["out"] if r["densified"] is not None]
    assert got == runs["ref32"]["P_after_densify"] == r64["P_after_densify"]
    assert [r["P"] for r in runs["out"]] == [e["P"] for e in runs["ref32"]["trace"]]
    assert got[0] != runs["out"][18]["P"]


def test_a_relayout_iteration_keeps_the_gaussian_rows_bits(runs):
    """the empty near-camera prune (iteration 17): parameters and both moments of xyz / opacity rows move only by the depth
    legs, scaling / rotation / SH rows keep every bit; the neural parameters change"""
    its = [it for it, *_ in runs["relayout"]]
    assert 17 in its, its
    P = None
    for it, before, after, neural_before, neural_after in runs["relayout"]:
        tr = runs["trainer"]
        for b, a in zip(before, after):
            P = b.numel() // 59
            off = {"xyz": (0, 3 * P), "features": (3 * P, 51 * P), "opacity": (51 * P, 52 * P), "scaling": (52 * P, 55 * P),
                   "rotation": (55 * P, 59 * P)}
            for k in ("features", "scaling", "rotation"):
                lo, hi = off[k]
                assert torch.equal(b[lo:hi].view(torch.int32), a[lo:hi].view(torch.int32)), (it, k)
        assert any(not torch.equal(x, y) for x, y in zip(neural_before, neural_after)), it
        assert tr is not None


def test_the_photometric_step_alone_is_cancelled_by_a_relayout(oracle):
    """one iteration with both depth legs off and an empty near-camera prune: EVERY Gaussian row keeps its bits, parameters and
    moments, and no step count advances, while the neural parameters change"""
    _, cams, _, _ = inputs()
    opt = options(cams, hard_depth_start=100, soft_depth_start=100, near_prune_interval=1, near_prune_start=0, clean_iterations=[])
    tr = make_trainer(oracle)
    tr.train_iteration(1, options(cams, hard_depth_start=100, soft_depth_start=100, clean_iterations=[]))   # a plain step first
    before, nb = rows(tr.model), [p.detach().clone() for p in tr.neural_parameters()]
    steps = dict(tr.model.optimizer.seg_steps)
    r = tr.train_iteration(2, opt)
    assert r["near_pruned"] == 0 and r["stepped"] == dict(hard=False, soft=False, gaussians=False, neural=True)
    for b, a in zip(before, rows(tr.model)):
        assert torch.equal(b.view(torch.int32), a.view(torch.int32))
    assert dict(tr.model.optimizer.seg_steps) == steps and steps["scaling"] == 1 and steps["features"] == 0
    assert all(not torch.equal(x, y) for x, y in zip(nb, tr.neural_parameters()) if float(x.abs().max()) > 0)


def test_the_gradients_of_the_first_iteration_are_the_restatements(runs):
    got, want = runs["first"]["trainer"], runs["first"]["reference"]
    assert set(got) == set(want) == {"hard", "photometric"}
    # the hard leg reaches xyz and nothing else
    assert all(v is None for k, v in want["hard"].items() if k != "xyz") and all(v is None for k, v in got["hard"].items() if k != "xyz")
    e = rel_err(got["hard"]["xyz"], want["hard"]["xyz"])
    print("hard leg   dL/dxyz       rel err %.2e" % e)
    assert float(want["hard"]["xyz"].abs().max()) > 0 and e <= TOL, e
    # the photometric leg: xyz, opacity, scaling, rotation, the embeddings and the five weight matrices - never the SH rows
    assert want["photometric"]["features"] is None and got["photometric"]["features"] is None
    for k, w in want["photometric"].items():
        if k == "features":
            continue
        e = rel_err(got["photometric"][k], w)
        print("photometric dL/d%-9s rel err %.2e" % (k, e))
        assert float(w.abs().max()) > 0 and e <= TOL, (k, e)


def test_the_parameters_after_the_run_lie_within_the_restatements_own_rounding(runs):
    tr = runs["trainer"]
    f32, f64 = dtr.flat_of(runs["ref32"]["model"]).double(), dtr.flat_of(runs["ref64"]["model"])
    got = tr.model.flat.detach().double()
    assert got.shape == f32.shape == f64.shape
    own = float((f32 - f64).pow(2).mean().sqrt())
    dist = float((got - f32).pow(2).mean().sqrt())
    print("rms(float32 restatement - float64 twin) = %.3e, rms(trainer - float32 restatement) = %.3e" % (own, dist))
    assert own > 0 and dist <= 4.0 * own, (dist, own)
    n32 = torch.cat([p.detach().double().reshape(-1) for p in runs["ref32"]["neural"].parameters()])
    n64 = torch.cat([p.detach().double().reshape(-1) for p in runs["ref64"]["neural"].parameters()])
    ngot = torch.cat([p.detach().double().reshape(-1) for p in tr.neural_parameters()])
    own_n, dist_n = float((n32 - n64).pow(2).mean().sqrt()), float((ngot - n32).pow(2).mean().sqrt())
    print("neural: rms(float32 - float64) = %.3e, rms(trainer - float32) = %.3e" % (own_n, dist_n))
    assert own_n > 0 and dist_n <= 4.0 * own_n, (dist_n, own_n)


def test_what_is_closed_to_this_trainer_raises_its_message(oracle):
    with pytest.raises(RuntimeError, match="world_size"):
        make_trainer(oracle, world_size=2)
    with pytest.raises(RuntimeError, match="alpha masks"):
        make_trainer(oracle, alpha_masks=[None] * 4)
    with pytest.raises(RuntimeError, match="depth_limit"):
        make_trainer(oracle, depth_limit="deferred")
    with pytest.raises(RuntimeError, match="sparse_adam"):
        make_trainer(oracle, optimizer_type="sparse_adam")
    with pytest.raises(RuntimeError, match="side launch"):
        make_trainer(oracle, side_launch=True)
    with pytest.raises(RuntimeError, match="fused photometric step"):
        make_trainer(oracle, fused_step=True)
    sc, cams, gts, mono = inputs()
    with pytest.raises(RuntimeError, match="with_nir"):
        make_trainer(oracle, model=GaussianModelLite(sc, torch.device("cpu"), api=oracle.api, with_nir=True))
    exp = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    exp.enable_exposure(len(cams))
    with pytest.raises(RuntimeError, match="exposure"):
        make_trainer(oracle, model=exp)
    tr = make_trainer(oracle)
    with pytest.raises(RuntimeError, match="depth_limit"):
        tr.depth_limit = "deferred"
    from gsplat_amd.trainer import GraphedStep
    with pytest.raises(RuntimeError, match="GraphedStep"):
        GraphedStep(tr)
    with pytest.raises(ValueError, match="one mono depth map"):
        TrainerDNG(GaussianModelLite(sc, torch.device("cpu"), api=oracle.api), cams, gts, mono[:2], neural=dtr.stand_in_for(sc),
                   Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings)
    assert not tr.fused_legs_available()   # (a CPU model: the legs are un-fused whatever fused_depth_legs says)


def test_the_options_carry_the_references_defaults():
    o = DngOptions()
    assert (o.iterations, o.position_lr_start, o.neural_grid, o.neural_net, o.error_tolerance, o.split_opacity_thresh,
            o.soft_depth_start, o.hard_depth_start, o.shape_pena, o.scale_pena, o.opa_pena, o.lambda_dssim, o.densify_from_iter,
            o.densify_until_iter, o.densify_grad_threshold, o.min_opacity, o.densify_rule) == \
        (30_000, 0, 5e-3, 5e-4, 0.2, 0.1, 1000, 0, 0.001, 0.001, 0.01, 0.2, 500, 15_000, 1e-4, 0.01, "dng")
    assert (o.patch_range, o.smooth_start, o.near_prune_interval, o.near_prune_start, o.clean_iterations) == \
        ((5, 17), 3000, 25, 2000, [6000, 1])
    assert (o.opacity_lr, o.position_lr_final, o.position_lr_max_steps, o.densification_interval) == (0.05, 0.0000016, 30_000, 100)
    assert o.fused_depth_legs is False   # opt-in: DESIGN.md section 4.12 has the measurement that decided it
    with pytest.raises(TypeError):
        DngOptions(patch_ranges=(5, 17))


def test_the_entry_point_is_declared_everywhere():
    import os
    import re
    from gsplat_amd.capi import DEVICE_ONLY, PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "gsplat.h")).read(), flags=re.S)
    assert "depth_backward_step" in PROTOTYPES and "depth_backward_step" in DEVICE_ONLY
    decl = re.search(r"\bgs_depth_backward_step\s*\(([^;]*)\)\s*;", header)
    assert decl and len(decl.group(1).split(",")) == len(PROTOTYPES["depth_backward_step"][1]) == 20
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)   # additive: the ABI number stays
