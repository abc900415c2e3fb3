"""TrainerDNGBlender and TrainerDNGBlenderSH without a GPU: the loops of gsplat_amd.trainer on the CPU checker (un-fused legs
through the given rasterizer, the Blender pieces as tests/blender_reference.py's callables).

The neural loop is held to the literal restatement of DNGaussian/train_blender.py:66-228 (tests/blender_train_reference.py) and
its float64 twin on a schedule compressed into 48 iterations - the method and the bars of tests/test_dng_trainer_cpu.py: 257
Gaussians, 64 x 48, 4 cameras of which the last has no white pixel, depth legs every 2nd iteration, densification every 10 from
10, a height prune that removes some rows, the regulariser's decay past densify_until_iter, the clean at iteration 1.
The SH loop is held the same way to the literal restatement of train_blender.py:265-388 (blender_train_reference.run_sh) and
its float64 twin - trace, step counts, patch draws, rule counts, P, the gradients of the hard and photometric legs, final
parameters - and to the script's conditions: which iteration runs which leg, the SH ramp, the reset at densify_from_iter
without a densification and its cancelled opacity step, the white rule on the re-laid-out model.
Both loops: a re-layout that removes nothing keeps every Gaussian row's bits, parameters and moments."""
import pytest
import torch

import blender_reference as br
import blender_train_reference as btr
import dng_depth_reference as depr
import dng_reg_reference as rgr
import dng_train_reference as dtr
import test_dng_trainer_cpu as llff
from gsplat_amd.trainer import (DngBlenderOptions, DngOptions, GaussianModelLite, TrainerDNG, TrainerDNGBlender,
                                TrainerDNGBlenderSH, cameras_extent)
from helpers import TOL, rel_err

P0, W, H, N_ITERS = 257, 64, 48, 48
EVENT_KEYS = ("camera", "patches", "xyz_lr", "stepped", "densified", "cleaned", "P", "height_pruned")

# chosen in gaps of the float64 twin's traces (the tests print the nearest neighbours):
GRAD_THRESHOLD = 1.0e-6       # of the densification statistic at both densifications
WHITE_RULE = (0.50436, 0.1)   # of min_c of the per-Gaussian colours at both densifications: the stand-in renderer's lie around 0.5
HEIGHT = -1.15                # of the last coordinate after both densifications


def inputs():
    """tests/test_dng_trainer_cpu.py's cameras and mono depths, a 257-Gaussian scene, and ground truth with a white (1.0) band
    down from the top of each column, 0 .. 30 rows deep; the last camera's image has no white pixel"""
    from gsplat_amd import synthetic
    _, cams, gts, mono = llff.inputs()
    sc = synthetic.trained_like(P0, seed=llff.SEED, scale_mult=1.5)
    g = torch.Generator().manual_seed(12)
    out = []
    for i, gt in enumerate(gts):
        gt = 0.1 + 0.8 * gt
        if i < len(gts) - 1:
            depth = torch.randint(0, 31, (W,), generator=g)
            white = torch.arange(H)[:, None] < depth[None, :]
            gt = torch.where(white[None], torch.ones_like(gt), gt)
            gt[1, 40, 5] = 1.0      # one white channel beside two others: not masked
        out.append(gt.contiguous())
    return sc, cams, out, mono


def options(cams, **kw):
    o = dict(iterations=48, position_lr_max_steps=48, hard_depth_start=0, soft_depth_start=6, densify_from_iter=10,
             densification_interval=10, densify_until_iter=35, clean_iterations=[6000, 1], densify_grad_threshold=GRAD_THRESHOLD,
             seed=3, cameras_extent=cameras_extent([c.camera_center for c in cams]), patch_range=(5, 17), depth_leg_interval=2,
             white_rule=WHITE_RULE, height_prune=HEIGHT, shape_pena=0.001, scale_pena=0.001, opa_pena=0.01,
             # the rule leaves opacities at 0.1 sigmoid(o) and the reference splits on `opacity > 0.1`: the threshold is moved
             # off the value the DTU schedule moves it off, for the same reason
             split_opacity_thresh=0.15)
    o.update(kw)
    return DngBlenderOptions(**o)


def background_mask(gt, threshold, mono=None):
    mask = br.background_mask(gt, threshold)
    return mask if mono is None else (mask, br.depth_target(mono, mask))


def white_rule(colour, stat, opacity_raw, threshold, factor=0.1):
    return br.white_rule(colour, stat, opacity_raw, threshold, factor)


def white_rule_sh(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor=0.1, return_colour=False):
    n, colour = br.white_rule_sh(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor)
    return (n, colour) if return_colour else n


def make_trainer(oracle, opt=None, **kw):
    sc, cams, gts, mono = inputs()
    model = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    model.active_sh_degree = 0
    return TrainerDNGBlender(model, cams, gts, mono, opt=opt, neural=dtr.stand_in_for(sc), Rasterizer=oracle.FsgsRasterizer,
                             Settings=oracle.FsgsSettings, depth_loss=depr.depth_regulariser, regulariser=llff.regulariser,
                             view_dirs=rgr.view_dirs, background_mask=background_mask, white_rule=white_rule, **kw)


def make_sh_trainer(oracle, opt=None, **kw):
    sc, cams, gts, mono = inputs()
    model = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    model.active_sh_degree = 0
    return TrainerDNGBlenderSH(model, cams, gts, mono, opt=opt, Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings,
                               depth_loss=depr.depth_regulariser, background_mask=background_mask, white_rule_sh=white_rule_sh, **kw)


def event(r):
    return dict(camera=r["camera"], patches=tuple(r["patches"]), xyz_lr=r["xyz_lr"], stepped=dict(r["stepped"]),
                densified=r["densified"] is not None, cleaned=r["cleaned"] is not None, P=r["P"], height_pruned=r["height_pruned"])


def grads_of(params, P, neural_parameters):
    out = {k: (v.grad.detach().clone().reshape(P, -1) if v.grad is not None else None) for k, v in params.items()}
    out.update({"neural%d" % i: (p.grad.detach().clone() if p.grad is not None else None) for i, p in enumerate(neural_parameters)})
    return out


@pytest.fixture(scope="module")
def runs(oracle):
    """the trainer, the float32 restatement and its float64 twin over the compressed schedule - computed once"""
    sc, cams, gts, mono = inputs()
    opt = options(cams)
    tr = make_trainer(oracle, opt=opt)
    out = []
    for it in range(1, N_ITERS + 1):
        out.append(tr.train_iteration(it, opt))
    ref32 = btr.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float32)
    ref64 = btr.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float64)
    return dict(trainer=tr, out=out, ref32=ref32, ref64=ref64, opt=opt, gts=gts)


def _gap(name, v, thr):
    lo, hi = v[v < thr], v[v > thr]
    print("%s: %d rows, nearest below %.6e, threshold %.6e, nearest above %.6e"
          % (name, v.numel(), float(lo.max()) if lo.numel() else float("nan"), thr, float(hi.min()) if hi.numel() else float("nan")))
    return lo, hi


def test_the_inputs_alone_satisfy_the_margin_conditions(runs):
    """a condition on the INPUTS, asserted on the restatement's float64 twin before anything is compared against it: the
    densification threshold, the white threshold and the height lie in gaps of its traces"""
    r64, opt = runs["ref64"], runs["opt"]
    for g in r64["statistic"]:
        _gap("statistic", g, opt.densify_grad_threshold)
    assert len(r64["margins"]) == 2 and min(r64["margins"]) > 1e-5, r64["margins"]
    assert len(r64["colours"]) == 2 and len(r64["heights"]) == 2
    for mn in r64["colours"]:
        lo, hi = _gap("min_c", mn, opt.white_rule[0])
        assert lo.numel() and hi.numel() and min(opt.white_rule[0] - float(lo.max()), float(hi.min()) - opt.white_rule[0]) > 1e-5
    for z in r64["heights"]:
        lo, hi = _gap("height", z, opt.height_prune)
        assert lo.numel() and hi.numel() and min(opt.height_prune - float(lo.max()), float(hi.min()) - opt.height_prune) > 1e-4
    a, b = runs["ref32"]["trace"], r64["trace"]
    for k in EVENT_KEYS + ("rule_count", "masked"):
        assert [e[k] for e in a] == [e[k] for e in b], k


def test_the_schedule_passes_every_event(runs):
    out, opt = runs["out"], runs["opt"]
    for i, r in enumerate(out, 1):
        due = i % 2 == 0 and i < opt.densify_until_iter
        assert (r["loss_hard"] is not None) == due, i
        assert (r["loss_soft"] is not None) == (due and i > opt.soft_depth_start), i
        assert (r["patches"][:2] != (None, None)) == due and (r["patches"][2:] != (None, None)) == (due and i > 6)
        assert r["near_pruned"] is None
    assert [i + 1 for i, r in enumerate(out) if r["densified"] is not None] == [20, 30]
    counts = {i + 1: int(r["rule_count"]) for i, r in enumerate(out) if r["rule_count"] is not None}
    pruned = {i + 1: r["height_pruned"] for i, r in enumerate(out) if r["height_pruned"] is not None}
    print("white rule counts:", counts, "height prunes:", pruned, "densifications:", [r["densified"] for r in out if r["densified"] is not None])
    assert sorted(counts) == [20, 30] and min(counts.values()) > 0
    assert sorted(pruned) == [20, 30] and max(pruned.values()) > 0                  # the height prune removes some rows
    assert [i + 1 for i, r in enumerate(out) if r["cleaned"] is not None] == [1]
    assert out[0]["stepped"] == dict(hard=False, soft=False, gaussians=False, neural=True)
    assert out[1]["stepped"] == dict(hard=True, soft=False, gaussians=True, neural=True)
    assert out[7]["stepped"] == dict(hard=True, soft=True, gaussians=True, neural=True)
    assert out[19]["stepped"] == dict(hard=True, soft=True, gaussians=False, neural=True)
    assert out[-1]["stepped"] == dict(hard=False, soft=False, gaussians=False, neural=False)   # the last iteration steps nothing
    assert all(p is None or 5 <= p <= 17 for r in out for p in r["patches"])
    masked = [int(m.sum()) for m in runs["trainer"].bg_masks]
    assert masked[3] == 0 and min(masked[:3]) > 0, masked


def test_the_masks_and_the_zeroed_targets_are_the_restatements(runs):
    tr = runs["trainer"]
    _, _, gts, mono = inputs()
    for ci, gt in enumerate(gts):
        mask = gt.min(0, keepdim=True).values > 254 / 255
        assert torch.equal(tr.bg_masks[ci], mask) and torch.equal(tr.gts[ci], gt)       # the ground truth is not edited
        want = 255.0 - mono[ci]
        want[mask.reshape(want.shape)] = 0
        assert torch.equal(tr.mono[ci].reshape(want.shape), want) and tr.mono[ci].shape == (1, 1, H, W)
        assert not bool(mask[0, 40, 5]) or ci == 3


def test_the_event_trace_is_the_restatements(runs):
    got = [event(r) for r in runs["out"]]
    for name in ("ref32", "ref64"):
        want = [{k: e[k] for k in EVENT_KEYS} for e in runs[name]["trace"]]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]
        counts = [int(r["rule_count"]) if r["rule_count"] is not None else None for r in runs["out"]]
        assert counts == [e["rule_count"] for e in runs[name]["trace"]]


def test_the_step_counts_are_the_restatements(runs):
    tr = runs["trainer"]
    got = {k: tr.model.optimizer.seg_steps[k] for k in ("xyz", "opacity", "scaling", "rotation", "features")}
    neural = [int(tr.neural_optimizer.state[p]["step"]) for p in tr.neural_parameters()]
    print("Adam step counts:", got, "neural:", neural)
    for name in ("ref32", "ref64"):
        assert got == {k: runs[name]["steps"][k] for k in got}, (name, got, runs[name]["steps"])
        assert neural == runs[name]["neural_steps"]
    n_hard = sum(1 for r in runs["out"] if r["stepped"]["hard"])
    n_soft = sum(1 for r in runs["out"] if r["stepped"]["soft"])
    n_photo = sum(1 for r in runs["out"] if r["stepped"]["gaussians"])
    assert (n_hard, n_soft, n_photo) == (17, 14, 44) and got["features"] == 0
    assert got["xyz"] == n_hard + n_photo and got["opacity"] == n_soft + n_photo and got["scaling"] == got["rotation"] == n_photo
    assert neural == [47] * 6


def test_P_after_each_relayout_is_the_restatements(runs):
    got = [r["P"] for r in runs["out"] if r["densified"] is not None]
    assert got == runs["ref32"]["P_after_densify"] == runs["ref64"]["P_after_densify"]
    assert [r["P"] for r in runs["out"]] == [e["P"] for e in runs["ref32"]["trace"]]
    assert got[0] != runs["out"][18]["P"]


def test_the_gradients_of_an_iteration_with_every_leg_are_the_restatements(oracle):
    """iterations 1 and 2 from the same state with the soft leg's start at 0: iteration 2 runs hard, soft and photometric"""
    sc, cams, gts, mono = inputs()
    opt = options(cams, soft_depth_start=0)
    got, want = {}, {}
    tr = make_trainer(oracle, opt=opt)
    tr.train_iteration(1, opt)
    tr.after_backward = lambda leg, trainer: got.__setitem__(leg, grads_of(trainer.model.params, trainer.model.P, trainer.neural_parameters()))
    r = tr.train_iteration(2, opt)
    assert r["stepped"]["hard"] and r["stepped"]["soft"]
    btr.run(oracle, sc, cams, gts, mono, opt, 2, torch.float32,
            after_backward=lambda leg, it, ref, neural: want.__setitem__(leg, grads_of(ref.p, ref.P, list(neural.parameters()))) if it == 2 else None)
    assert set(got) == set(want) == {"hard", "soft", "photometric"}
    for leg, field in (("hard", "xyz"), ("soft", "opacity")):
        assert all(v is None for k, v in want[leg].items() if k != field) and all(v is None for k, v in got[leg].items() if k != field), leg
        e = rel_err(got[leg][field], want[leg][field])
        print("%-5s leg  dL/d%-9s rel err %.2e" % (leg, field, e))
        assert float(want[leg][field].abs().max()) > 0 and e <= TOL, (leg, e)
    for k, w in want["photometric"].items():
        if k == "features":
            assert w is None and got["photometric"][k] is None
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


def test_the_regulariser_decays_past_densify_until_iter(oracle):
    """one photometric leg from the same state, before and past densify_until_iter: the losses differ by 0.9 regulariser"""
    _, cams, _, _ = inputs()
    a, b, fresh = make_trainer(oracle), make_trainer(oracle), make_trainer(oracle)
    oa, ob = options(cams, densify_until_iter=35, clean_iterations=[]), options(cams, densify_until_iter=0, clean_iterations=[])
    ra, rb = a.train_iteration(1, oa), b.train_iteration(1, ob)
    reg = float(llff.regulariser(fresh.model.get_scaling.detach(), fresh.model.get_opacity.detach(), 0.001, 0.001, 0.01))
    assert ra["camera"] == rb["camera"] and reg > 0
    assert abs((float(ra["loss"]) - float(rb["loss"])) - 0.9 * reg) <= 1e-5 * abs(float(ra["loss"]))


# ---------------------------------------------------------------------------------------------------------------- the SH loop
def sh_options(cams, **kw):
    o = dict(use_sh=True, sh_increase_interval=15, opacity_reset_interval=30, white_rule=(0.6, 0.1), height_prune=HEIGHT)
    o.update(kw)
    return options(cams, **o)


SH_EVENT_KEYS = ("camera", "patches", "xyz_lr", "sh_degree", "stepped", "densified", "cleaned", "reset", "P", "height_pruned")


def rows(model):
    o = model.optimizer
    return model.flat.detach().clone(), o.exp_avg.detach().clone(), o.exp_avg_sq.detach().clone()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def sh_grads_of(params, P):
    out = {k: (v.grad.detach().clone().reshape(P, -1) if v.grad is not None else None) for k, v in params.items()}
    if "f_dc" in out:      # the restatement's two groups in the model's row layout [P,16,3]
        dc, rest = out.pop("f_dc"), out.pop("f_rest")
        out["features"] = None if dc is None else torch.cat((dc.reshape(P, 1, 3), rest.reshape(P, 15, 3)), dim=1).reshape(P, -1)
    return out


@pytest.fixture(scope="module")
def sh_run(oracle):
    """the SH trainer, the float32 restatement and its float64 twin over the compressed schedule - computed once"""
    sc, cams, gts, mono = inputs()
    opt = sh_options(cams)
    tr = make_sh_trainer(oracle, opt=opt)
    out, opacity_at_reset = [], {}
    for it in range(1, N_ITERS + 1):
        out.append(tr.train_iteration(it, opt))
        if out[-1]["reset"]:
            opacity_at_reset[it] = tr.model.get_opacity.detach().clone()
    ref32 = btr.run_sh(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float32)
    ref64 = btr.run_sh(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float64)
    return dict(trainer=tr, out=out, opt=opt, opacity_at_reset=opacity_at_reset, ref32=ref32, ref64=ref64)


def sh_event(r):
    return dict(camera=r["camera"], patches=tuple(r["patches"]), xyz_lr=r["xyz_lr"], sh_degree=r["sh_degree"],
                stepped=dict(r["stepped"]), densified=r["densified"] is not None, cleaned=r["cleaned"] is not None,
                reset=r["reset"], P=r["P"], height_pruned=r["height_pruned"])


def test_the_sh_inputs_alone_satisfy_the_margin_conditions(sh_run):
    """asserted on the restatement's float64 twin before anything is compared against it: the densification threshold, the
    white threshold and the height lie in gaps of its traces, and the float32 restatement took every decision as its twin did"""
    r64, opt = sh_run["ref64"], sh_run["opt"]
    assert len(r64["statistic"]) == len(r64["colours"]) == len(r64["heights"]) == 2
    for g in r64["statistic"]:
        lo, hi = _gap("statistic", g, opt.densify_grad_threshold)
        assert hi.numel() and float(hi.min()) - opt.densify_grad_threshold > 1e-3 * opt.densify_grad_threshold
        assert not lo.numel() or opt.densify_grad_threshold - float(lo.max()) > 1e-3 * opt.densify_grad_threshold
    for mn in r64["colours"]:
        lo, hi = _gap("min_c", mn, opt.white_rule[0])
        assert lo.numel() and hi.numel() and min(opt.white_rule[0] - float(lo.max()), float(hi.min()) - opt.white_rule[0]) > 1e-5
    for z in r64["heights"]:
        lo, hi = _gap("height", z, opt.height_prune)
        assert lo.numel() and hi.numel() and min(opt.height_prune - float(lo.max()), float(hi.min()) - opt.height_prune) > 1e-4
    a, b = sh_run["ref32"]["trace"], r64["trace"]
    for k in SH_EVENT_KEYS + ("rule_count", "masked"):
        assert [e[k] for e in a] == [e[k] for e in b], k


def test_the_sh_event_trace_step_counts_and_P_are_the_restatements(sh_run):
    got = [sh_event(r) for r in sh_run["out"]]
    tr = sh_run["trainer"]
    steps = {k: tr.model.optimizer.seg_steps[k] for k in ("xyz", "opacity", "scaling", "rotation", "features")}
    print("SH loop Adam step counts:", steps)
    for name in ("ref32", "ref64"):
        ref = sh_run[name]
        want = [{k: e[k] for k in SH_EVENT_KEYS} for e in ref["trace"]]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]
        counts = [int(r["rule_count"]) if r["rule_count"] is not None else None for r in sh_run["out"]]
        assert counts == [e["rule_count"] for e in ref["trace"]]
        rs = ref["steps"]
        assert rs["f_dc"] == rs["f_rest"] == steps["features"]
        assert {k: rs[k] for k in ("xyz", "opacity", "scaling", "rotation")} == {k: steps[k] for k in ("xyz", "opacity", "scaling", "rotation")}
        assert [r["P"] for r in sh_run["out"] if r["densified"] is not None] == ref["P_after_densify"]
    dens = [r["P"] for r in sh_run["out"] if r["densified"] is not None]
    assert dens[0] != sh_run["out"][18]["P"]


def test_the_sh_gradients_of_an_iteration_with_both_legs_are_the_restatements(oracle):
    """iterations 1 and 2 from the same state: iteration 2 runs the hard leg and the photometric leg through the SH rows"""
    sc, cams, gts, mono = inputs()
    opt = sh_options(cams)
    got, want = {}, {}
    tr = make_sh_trainer(oracle, opt=opt)
    tr.model.active_sh_degree = 3
    tr.train_iteration(1, opt)
    tr.after_backward = lambda leg, trainer: got.__setitem__(leg, sh_grads_of(trainer.model.params, trainer.model.P))
    r = tr.train_iteration(2, opt)
    assert r["stepped"] == dict(hard=True, gaussians=True, opacity=True) and r["sh_degree"] == 3
    btr.run_sh(oracle, sc, cams, gts, mono, opt, 2, torch.float32, sh_degree=3,
               after_backward=lambda leg, it, ref: want.__setitem__(leg, sh_grads_of(ref.p, ref.P)) if it == 2 else None)
    assert set(got) == set(want) == {"hard", "photometric"}
    assert all(v is None for k, v in want["hard"].items() if k != "xyz") and all(v is None for k, v in got["hard"].items() if k != "xyz")
    e = rel_err(got["hard"]["xyz"], want["hard"]["xyz"])
    print("SH hard leg  dL/dxyz rel err %.2e" % e)
    assert float(want["hard"]["xyz"].abs().max()) > 0 and e <= TOL
    assert set(want["photometric"]) == {"xyz", "features", "opacity", "scaling", "rotation"}
    for k, w in want["photometric"].items():
        e = rel_err(got["photometric"][k], w)
        print("SH photometric dL/d%-9s rel err %.2e" % (k, e))
        assert float(w.abs().max()) > 0 and e <= TOL, (k, e)
    assert float(want["photometric"]["features"][:, 3:].abs().max()) > 0          # the higher SH rows get a gradient at degree 3


def test_the_sh_parameters_after_the_run_lie_within_the_restatements_own_rounding(sh_run):
    tr = sh_run["trainer"]
    f32, f64 = btr.flat_of_sh(sh_run["ref32"]["model"]).double(), btr.flat_of_sh(sh_run["ref64"]["model"])
    got = tr.model.flat.detach().double()
    assert got.shape == f32.shape == f64.shape
    own = float((f32 - f64).pow(2).mean().sqrt())
    dist = float((got - f32).pow(2).mean().sqrt())
    print("SH loop: rms(float32 restatement - float64 twin) = %.3e, rms(trainer - float32 restatement) = %.3e" % (own, dist))
    assert own > 0 and dist <= 4.0 * own, (dist, own)


# ---------------------------------------------------------------------------------------------------------------- bits kept
def test_a_relayout_that_removes_nothing_keeps_every_gaussian_rows_bits(oracle):
    """both loops, one plain step and then an iteration whose clean sees every Gaussian (a re-layout in the reference all the
    same): no depth leg, the photometric step of the Gaussian groups cancelled - parameters, both moments and every step count
    keep their bits, while the neural tensors step"""
    _, cams, _, _ = inputs()
    for make, opts in ((make_trainer, options), (make_sh_trainer, sh_options)):
        tr = make(oracle)
        tr.train_iteration(1, opts(cams, hard_depth_start=100, soft_depth_start=100, clean_iterations=[]))
        keep = tr.prune_unseen(opt=opts(cams))
        assert keep == 0                                              # every Gaussian is seen: the clean below removes nothing
        before, steps = rows(tr.model), dict(tr.model.optimizer.seg_steps)
        nb = [p.detach().clone() for p in tr.neural_parameters()]
        r = tr.train_iteration(2, opts(cams, hard_depth_start=100, soft_depth_start=100, clean_iterations=[2]))
        assert r["cleaned"] == 0 and r["stepped"]["gaussians"] is False and r["stepped"]["hard"] is False
        for b, a in zip(before, rows(tr.model)):
            assert same_bits(b, a)
        assert dict(tr.model.optimizer.seg_steps) == steps and steps["scaling"] == 1
        if nb:
            assert r["stepped"]["neural"] and any(not torch.equal(x, y) for x, y in zip(nb, tr.neural_parameters()))


def test_the_sh_reset_without_a_densification_cancels_the_opacity_group_alone(oracle):
    """iteration 10 = densify_from_iter: the opacity rows are inverse_sigmoid(min(sigmoid(rows), 0.01)) of the rows the
    iteration started with (the hard leg steps xyz alone), their moments zero and their step count where it was; every other
    group steps"""
    _, cams, _, _ = inputs()
    opt = sh_options(cams)
    tr = make_sh_trainer(oracle, opt=opt)
    for it in range(1, 10):
        tr.train_iteration(it, opt)
    m, o = tr.model, tr.model.optimizer
    P = m.P
    off = {"xyz": (0, 3 * P), "features": (3 * P, 51 * P), "opacity": (51 * P, 52 * P), "scaling": (52 * P, 55 * P),
           "rotation": (55 * P, 59 * P)}
    before, steps = rows(m), dict(o.seg_steps)
    r = tr.train_iteration(10, opt)
    assert r["reset"] and r["densified"] is None and r["P"] == P and r["stepped"] == dict(hard=True, gaussians=True, opacity=False)
    after = rows(m)
    lo, hi = off["opacity"]
    op = torch.sigmoid(before[0][lo:hi])
    new = torch.min(op, torch.ones_like(op) * 0.01)
    assert same_bits(after[0][lo:hi], torch.log(new / (1 - new)))
    assert int((after[1][lo:hi].view(torch.int32) != 0).sum()) == 0 and int((after[2][lo:hi].view(torch.int32) != 0).sum()) == 0
    assert float(before[1][lo:hi].abs().max()) > 0                    # (they held something)
    for k in ("xyz", "features", "scaling", "rotation"):
        lo, hi = off[k]
        assert not same_bits(before[0][lo:hi], after[0][lo:hi]), k
    want = {k: v + 1 for k, v in steps.items()}
    want["xyz"] += 1
    want["opacity"] -= 1
    assert dict(o.seg_steps) == want


def test_the_sh_loop_follows_the_scripts_conditions(sh_run):
    out, opt, tr = sh_run["out"], sh_run["opt"], sh_run["trainer"]
    for i, r in enumerate(out, 1):
        due = i % 2 == 0 and i < opt.densify_until_iter
        assert (r["loss_hard"] is not None) == due and (r["patches"] != (None, None)) == due, i
        assert r["sh_degree"] == min(i // 15, 3), i                                 # the ramp: every sh_increase_interval
    assert [i + 1 for i, r in enumerate(out) if r["densified"] is not None] == [20, 30]
    # the reset: at densify_from_iter (10) WITHOUT a densification, and at opacity_reset_interval (30) behind one
    assert [i + 1 for i, r in enumerate(out) if r["reset"]] == [10, 30]
    assert out[9]["densified"] is None and out[9]["stepped"] == dict(hard=True, gaussians=True, opacity=False)
    assert out[29]["densified"] is not None and out[29]["stepped"] == dict(hard=True, gaussians=False, opacity=False)
    assert out[19]["stepped"] == dict(hard=True, gaussians=False, opacity=False)   # a re-layout cancels every group's step
    assert out[0]["cleaned"] is not None and out[0]["stepped"]["gaussians"] is False
    assert out[-1]["stepped"] == dict(hard=False, gaussians=False, opacity=False)  # the last iteration steps nothing
    for it, op in sh_run["opacity_at_reset"].items():
        assert float(op.max()) <= 0.01 + 1e-6, it
    counts = {i + 1: int(r["rule_count"]) for i, r in enumerate(out) if r["rule_count"] is not None}
    pruned = {i + 1: r["height_pruned"] for i, r in enumerate(out) if r["height_pruned"] is not None}
    print("SH loop: white rule counts", counts, "height prunes", pruned, "densifications", [r["densified"] for r in out if r["densified"] is not None])
    assert sorted(counts) == [20, 30] and sorted(pruned) == [20, 30]
    # per-tensor step counts, from the conditions alone
    s = tr.model.optimizer.seg_steps
    n_hard = sum(1 for i in range(1, 48) if i % 2 == 0 and i < 35)
    n_photo = 47 - 3                                                               # iterations 1 (clean), 20 and 30 re-lay out
    assert n_hard == sum(1 for r in out if r["stepped"]["hard"]) and n_photo == sum(1 for r in out if r["stepped"]["gaussians"])
    assert s["xyz"] == n_hard + n_photo and s["scaling"] == s["rotation"] == s["features"] == n_photo
    assert s["opacity"] == n_photo - 1                                             # iteration 10: the reset cancels its step


def test_the_sh_white_rule_runs_on_the_relaid_out_model(oracle):
    """up to the first densification, then the rule's own statements on a copy of the model the densification left"""
    _, cams, _, _ = inputs()
    opt = sh_options(cams)
    tr = make_sh_trainer(oracle, opt=opt)
    seen = {}

    def spy(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor=0.1, return_colour=False):
        seen.update(P=xyz.shape[0], degree=degree, campos=campos.clone(), stat=stat.clone(), opacity=opacity_raw.clone(),
                    xyz=xyz.clone(), shs=shs.clone())
        return white_rule_sh(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor, return_colour)
    tr._white_rule_sh = spy
    for it in range(1, 21):
        r = tr.train_iteration(it, opt)
    m = tr.model
    assert r["densified"] is not None and seen["P"] + (-r["height_pruned"] if r["height_pruned"] else 0) == m.P
    assert seen["degree"] == 1 and torch.equal(seen["campos"], tr.cameras[r["camera"]].camera_center)
    assert float(seen["stat"].abs().max()) == 0.0                                  # the re-layout had zeroed it already
    colour = br.sh_colour(seen["xyz"], seen["shs"], 1, seen["campos"])
    fires = colour.min(-1).values > opt.white_rule[0]
    assert int(r["rule_count"]) == int(fires.sum()) > 0
    assert torch.equal(tr.last_colour, colour)


def test_the_sh_loop_refuses_a_neural_checkpoint(oracle):
    with pytest.raises(RuntimeError, match="load_shape"):
        make_sh_trainer(oracle, start_checkpoint="chkpnt_latest.pth")
    _, cams, _, _ = inputs()
    opt = options(cams)
    neural = make_trainer(oracle, opt=opt)
    neural.train_iteration(1, opt)
    with pytest.raises(RuntimeError, match="load_shape"):
        make_sh_trainer(oracle).restore(neural.checkpoint())
    a, b = make_sh_trainer(oracle), make_sh_trainer(oracle)
    so = sh_options(cams)
    for it in (1, 2, 3):
        a.train_iteration(it, so)
    b.restore(a.checkpoint())
    ra, rb = a.train_iteration(4, so), b.train_iteration(4, so)
    assert ra["camera"] == rb["camera"] and ra["patches"] == rb["patches"] and torch.equal(a.model.flat, b.model.flat)


# ---------------------------------------------------------------------------------------------------------------- options
RUN_BLENDER_SH = {   # scripts/run_blender.sh, flag by flag: (lines 13-21, 34-43, 58-67)
    1: {"--iterations": 6000, "--lambda_dssim": 0.2, "--densify_grad_threshold": 0.0005, "--prune_threshold": 0.01,
        "--densify_until_iter": 6000, "--densify_from_iter": 500, "--position_lr_final": 0.0000016, "--position_lr_max_steps": 1000,
        "--position_lr_start": 5000, "--hard_depth_start": 0, "--soft_depth_start": 9999999, "--split_opacity_thresh": 0.1,
        "--error_tolerance": 0.001, "--shape_pena": 0.0, "--opa_pena": 0.0, "--scale_pena": 0.0, "--use_SH": False,
        "--test_iterations": [1000, 2000, 3000, 4500, 6000]},
    2: {"--iterations": 6000, "--lambda_dssim": 0.2, "--densify_grad_threshold": 0.0005, "--prune_threshold": 0.005,
        "--densify_until_iter": 6000, "--densify_from_iter": 500, "--position_lr_final": 0.0000016, "--position_lr_max_steps": 1000,
        "--position_lr_start": 5000, "--hard_depth_start": 0, "--error_tolerance": 0.01, "--shape_pena": 0.0, "--opa_pena": 0.0,
        "--scale_pena": 0.0, "--use_SH": True, "--test_iterations": [1000, 2000, 3000, 4500, 6000]},
    3: {"--iterations": 30000, "--lambda_dssim": 0.2, "--densify_grad_threshold": 0.0002, "--prune_threshold": 0.005,
        "--densify_until_iter": 15000, "--densify_from_iter": 500, "--position_lr_final": 0.0000016, "--position_lr_max_steps": 30000,
        "--position_lr_start": 0, "--hard_depth_start": 99999, "--error_tolerance": 0.2, "--shape_pena": 0.0, "--opa_pena": 0.0,
        "--scale_pena": 0.0, "--use_SH": True, "--test_iterations": [1000, 2000, 3000, 4500, 6000]},
}
FLAG_TO_OPTION = {"--prune_threshold": "min_opacity", "--use_SH": "use_sh"}


@pytest.mark.parametrize("scene,setting", (("drums", 1), ("materials", 1), ("ship", 2), ("lego", 2), ("ficus", 2), ("hotdog", 2),
                                           ("chair", 3), ("mic", 3)))
def test_for_scene_is_run_blender_sh_line_by_line(scene, setting):
    o = DngBlenderOptions.for_scene("data/nerf_synthetic/%s" % scene)
    for flag, value in RUN_BLENDER_SH[setting].items():
        if flag == "--test_iterations":
            assert o.clean_iterations == value + [1]                                # testing_iterations + [first_iter]
            continue
        assert getattr(o, FLAG_TO_OPTION.get(flag, flag[2:])) == value, flag
    if "--soft_depth_start" not in RUN_BLENDER_SH[setting]:
        assert o.soft_depth_start == DngOptions().soft_depth_start
    assert o.white_background is True and o.patch_range == (5, 17) and o.depth_leg_interval == 10 and o.bg_threshold == 254 / 255
    assert o.height_prune == dict(ship=-0.5, hotdog=-0.2).get(scene)
    assert o.white_rule == (None if scene == "chair" else (253 / 255, 0.1))
    assert (o.prune_opacity, o.size_threshold, o.reset_at_densify_from, o.reg_decay) == (0.005, 20, True, 0.1)


def test_the_options_refuse_what_they_do_not_know():
    with pytest.raises(TypeError):
        DngBlenderOptions(bg_thresholds=0.1)
    with pytest.raises(TypeError):
        DngBlenderOptions.for_scene("lego", height=1.0)
    with pytest.raises(ValueError):
        DngBlenderOptions.for_scene("bicycle")
    assert DngBlenderOptions.for_scene("lego", iterations=100).iterations == 100
    assert isinstance(DngBlenderOptions(), DngOptions) and issubclass(TrainerDNGBlender, TrainerDNG)
    assert not hasattr(DngOptions(), "bg_threshold") and DngOptions().fused_depth_legs is False


def test_what_is_closed_to_the_llff_trainer_is_closed_here(oracle):
    for make in (make_trainer, make_sh_trainer):
        with pytest.raises(RuntimeError, match="world_size"):
            make(oracle, world_size=2)
        with pytest.raises(RuntimeError, match="fused photometric step"):
            make(oracle, fused_step=True)
        with pytest.raises(RuntimeError, match="depth_limit"):
            make(oracle, depth_limit=1.0)
        with pytest.raises(RuntimeError, match="sparse_adam"):
            make(oracle, optimizer_type="sparse_adam")
        tr = make(oracle)
        assert not tr.fused_legs_available()
        from gsplat_amd.trainer import GraphedStep
        with pytest.raises(RuntimeError, match="GraphedStep"):
            GraphedStep(tr)
