"""TrainerDNGDTU without a GPU: the loop of gsplat_amd.trainer on the CPU checker (un-fused legs through the given rasterizer,
the DTU pieces as tests/dtu_reference.py's callables) against the literal restatement of DNGaussian/train_dtu.py:64-247
(tests/dtu_train_reference.py) and its float64 twin, on a schedule compressed into 48 iterations - the method and the bars of
tests/test_dng_trainer_cpu.py.  The schedule shows: the soft leg's gate open and closed, iterations past the soft leg's start
with the gate shut (no patch draws for it), both colour rules with non-zero counts, the white rule's reset iteration, a camera
with an empty mask (a NaN alpha loss, a zero gradient, a step all the same), the clean at iteration 1, and the last iteration,
where the alpha leg's step is the only one."""
import pytest
import torch

import dng_depth_reference as depr
import dng_reg_reference as rgr
import dng_train_reference as dtr
import dtu_reference as dr
import dtu_train_reference as dtu
import test_dng_trainer_cpu as llff
from gsplat_amd.trainer import DngDtuOptions, DngOptions, GaussianModelLite, TrainerDNG, TrainerDNGDTU, cameras_extent
from helpers import TOL, rel_err

P0, W, H, N_ITERS = 257, 64, 48, 48
EVENT_KEYS = ("camera", "patches", "xyz_lr", "stepped", "densified", "cleaned", "P", "soft_gate_open")
BG_THRESHOLD = 30 / 255

# chosen in gaps of the float64 twin's traces (the tests print the nearest neighbours):
GRAD_THRESHOLD = 1.0e-6   # of the densification statistic at both densifications
SOFT_GATE = 1.0           # of ema_loss_hard over the iterations past the soft leg's start
BLACK_RULE = (0.496998, 10, True)   # of max_c / min_c of the per-Gaussian colours at both densifications: the stand-in renderer's
WHITE_RULE = (0.492025, 2, 15)      # colours lie around 0.5; the white rule resets at iteration 30 (30 % 15 == 0), not at 20


def inputs():
    """tests/test_dng_trainer_cpu.py's cameras and mono depths, a 257-Gaussian scene, and ground truth whose columns are dark
    from the top for 0 .. 30 rows (48 rows < run = 50: masked = dark all the way up); the last camera's image has no dark pixel"""
    from gsplat_amd import synthetic
    _, cams, gts, mono = llff.inputs()
    sc = synthetic.trained_like(P0, seed=llff.SEED, scale_mult=1.5)
    g = torch.Generator().manual_seed(11)
    out = []
    for i, gt in enumerate(gts):
        gt = 0.2 + 0.8 * gt
        if i < len(gts) - 1:
            depth = torch.randint(0, 31, (W,), generator=g)
            dark = torch.arange(H)[:, None] < depth[None, :]
            gt = torch.where(dark[None], gt * 0.1, gt)
            gt[:, 40, 5] *= 0.1     # a dark pixel with bright ones above it: not masked
        out.append(gt.contiguous())
    return sc, cams, out, mono


def options(cams, **kw):
    o = dict(iterations=48, position_lr_max_steps=48, hard_depth_start=0, soft_depth_start=6, densify_from_iter=12,
             densification_interval=10, densify_until_iter=35, clean_iterations=[6000, 1], densify_grad_threshold=GRAD_THRESHOLD,
             seed=3, cameras_extent=cameras_extent([c.camera_center for c in cams]), patch_range=(17, 40),
             bg_threshold=BG_THRESHOLD, soft_gate=SOFT_GATE, black_rule=BLACK_RULE, white_rule=WHITE_RULE,
             # the reference resets opacities to 0.1 and splits on `opacity > 0.1`: which side sigmoid(inverse_sigmoid(0.1))
             # falls on is one rounding.  The margin condition on the inputs moves the split threshold off the reset value
             split_opacity_thresh=0.15)
    o.update(kw)
    return DngDtuOptions(**o)


def background_mask(gt, threshold, run=50):
    return dr.background_mask(gt.clone(), threshold, run)


def colour_rule(colour, stat, opacity_raw, black=None, white=None, value=None):
    return dr.colour_rules(colour, stat, opacity_raw, black, white, value)


def make_trainer(oracle, opt=None, **kw):
    sc, cams, gts, mono = inputs()
    model = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    model.active_sh_degree = 0
    return TrainerDNGDTU(model, cams, gts, mono, opt=opt, neural=dtr.stand_in_for(sc), bg=torch.zeros(3),
                         Rasterizer=oracle.FsgsRasterizer, Settings=oracle.FsgsSettings, depth_loss=depr.depth_regulariser,
                         regulariser=llff.regulariser, view_dirs=rgr.view_dirs, background_mask=background_mask,
                         masked_fill=dr.masked_mean_fill, alpha_penalty=dr.alpha_penalty, colour_rule=colour_rule, **kw)


def event(r):
    return dict(camera=r["camera"], patches=tuple(r["patches"]), xyz_lr=r["xyz_lr"], stepped=dict(r["stepped"]),
                densified=r["densified"] is not None, cleaned=r["cleaned"] is not None, P=r["P"], soft_gate_open=r["soft_gate_open"])


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
    out = [tr.train_iteration(it, opt) for it in range(1, N_ITERS + 1)]
    ref32 = dtu.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float32)
    ref64 = dtu.run(oracle, sc, cams, gts, mono, opt, N_ITERS, torch.float64)
    return dict(trainer=tr, out=out, ref32=ref32, ref64=ref64, opt=opt, gts=gts)


def test_the_inputs_alone_satisfy_the_margin_conditions(runs):
    """a condition on the INPUTS, asserted on the restatement's float64 twin before anything is compared against it: the gate,
    the densification threshold and both colour thresholds lie in gaps of its traces"""
    r64, opt = runs["ref64"], runs["opt"]
    ema = [e for i, e in enumerate(r64["ema"], 1) if i > opt.soft_depth_start]
    below, above = [e for e in ema if e < opt.soft_gate], [e for e in ema if e >= opt.soft_gate]
    print("ema_loss_hard past the soft leg's start: nearest below %.6e, gate %.6e, nearest above %.6e" % (max(below), opt.soft_gate, min(above)))
    assert below and above and min(opt.soft_gate - max(below), min(above) - opt.soft_gate) > 1e-3 * opt.soft_gate
    for g in r64["statistic"]:
        thr = opt.densify_grad_threshold
        lo, hi = g[g < thr], g[g >= thr]
        print("statistic: %d rows, nearest below %.6e, threshold %.6e, nearest above %.6e"
              % (g.numel(), float(lo.max()) if lo.numel() else float("nan"), thr, float(hi.min()) if hi.numel() else float("nan")))
    assert len(r64["margins"]) == 2 and min(r64["margins"]) > 1e-5, r64["margins"]
    assert len(r64["colours"]) == 2
    for mx, mn in r64["colours"]:
        for name, v, thr in (("max_c", mx, opt.black_rule[0]), ("min_c", mn, opt.white_rule[0])):
            lo, hi = v[v < thr], v[v > thr]
            print("%s: %d rows, nearest below %.6e, threshold %.6e, nearest above %.6e" % (name, v.numel(), float(lo.max()), thr, float(hi.min())))
            assert lo.numel() and hi.numel() and min(thr - float(lo.max()), float(hi.min()) - thr) > 1e-5
    # and the float32 restatement took every decision as its twin did
    a, b = runs["ref32"]["trace"], r64["trace"]
    for k in EVENT_KEYS + ("rule_counts", "masked"):
        assert [e[k] for e in a] == [e[k] for e in b], k


def test_the_schedule_passes_every_event(runs):
    out, opt = runs["out"], runs["opt"]
    gates = [r["soft_gate_open"] for r in out]
    assert gates[:6] == [None] * 6 and True in gates and False in gates          # the gate both open and closed
    shut = [i + 1 for i, r in enumerate(out) if r["soft_gate_open"] is False]
    assert shut and all(out[i - 1]["loss_soft"] is None and out[i - 1]["patches"][2:] == (None, None) for i in shut)
    assert all(out[i - 1]["patches"][:2] != (None, None) and not out[i - 1]["stepped"]["soft"] for i in shut)
    opened = [i + 1 for i, r in enumerate(out) if r["soft_gate_open"]]
    assert all(out[i - 1]["loss_soft"] is not None and None not in out[i - 1]["patches"] for i in opened)
    assert all(r["loss_hard"] is not None and r["loss_alpha"] is not None and r["stepped"]["alpha"] for r in out)
    assert all(r["near_pruned"] is None for r in out)
    assert [i + 1 for i, r in enumerate(out) if r["densified"] is not None] == [20, 30]
    counts = {i + 1: r["rule_counts"] for i, r in enumerate(out) if r["rule_counts"] is not None}
    print("colour rule counts (black, white):", counts, "densifications:", [r["densified"] for r in out if r["densified"] is not None])
    assert sorted(counts) == [20, 30] and all(min(c) > 0 for c in counts.values())   # both rules, non-zero counts
    assert 30 % opt.white_rule[2] == 0 and 20 % opt.white_rule[2] != 0               # the white rule's reset iteration is reached
    assert [i + 1 for i, r in enumerate(out) if r["cleaned"] is not None] == [1]
    assert out[0]["stepped"] == dict(hard=True, soft=False, alpha=True, gaussians=False, neural=True)
    assert out[1]["stepped"] == dict(hard=True, soft=False, alpha=True, gaussians=True, neural=True)
    assert out[-1]["stepped"] == dict(hard=False, soft=False, alpha=True, gaussians=False, neural=False)   # the last iteration
    assert all(p is None or 17 <= p <= 40 for r in out for p in r["patches"])
    # a camera with an empty mask: NaN alpha loss, and the step happened all the same
    empty = [r for r in out if r["camera"] == 3]
    assert empty and all(bool(torch.as_tensor(r["loss_alpha"]).isnan()) and r["stepped"]["alpha"] for r in empty)
    assert all(not bool(torch.as_tensor(r["loss_alpha"]).isnan()) for r in out if r["camera"] != 3)
    masked = [int(m.sum()) for m in runs["trainer"].bg_masks]
    assert masked[3] == 0 and min(masked[:3]) > 0, masked


def test_the_masks_the_zeroed_images_and_the_filled_targets_are_the_restatements(runs):
    tr = runs["trainer"]
    _, _, gts, mono = inputs()
    for ci, gt in enumerate(gts):
        mask, zeroed = dr.background_mask(gt.clone(), BG_THRESHOLD, 50)
        assert torch.equal(tr.bg_masks[ci], mask) and torch.equal(tr.gts[ci], zeroed)
        assert torch.equal(mask, dr.background_mask_runs(gt, BG_THRESHOLD, 50))
        want = dr.masked_mean_fill((255.0 - mono[ci]).reshape(1, H, W), mask)
        assert torch.equal(tr.mono[ci].reshape(1, H, W), want)
        assert not bool(mask[0, 40, 5]) or ci == 3


def test_the_event_trace_is_the_restatements(runs):
    got = [event(r) for r in runs["out"]]
    for name in ("ref32", "ref64"):
        want = [{k: e[k] for k in EVENT_KEYS} for e in runs[name]["trace"]]
        assert got == want, [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:3]
        counts = [tuple(int(c) for c in r["rule_counts"]) if r["rule_counts"] is not None else None for r in runs["out"]]
        assert counts == [e["rule_counts"] for e in runs[name]["trace"]]
    ema = [r["ema_loss_hard"] for r in runs["out"]]
    assert max(abs(a - b) for a, b in zip(ema, runs["ref64"]["ema"])) < 1e-3 * max(ema)


def test_the_step_counts_are_the_restatements(runs):
    tr = runs["trainer"]
    got = {k: tr.model.optimizer.seg_steps[k] for k in ("xyz", "opacity", "scaling", "rotation", "features")}
    neural = [int(tr.neural_optimizer.state[p]["step"]) for p in tr.neural_parameters()]
    print("Adam step counts:", got, "neural:", neural)
    for name in ("ref32", "ref64"):
        assert got == {k: runs[name]["steps"][k] for k in got}, (name, got, runs[name]["steps"])
        assert neural == runs[name]["neural_steps"]
    n_soft = sum(1 for r in runs["out"] if r["stepped"]["soft"])
    n_photo = sum(1 for r in runs["out"] if r["stepped"]["gaussians"])
    assert got["features"] == 0 and n_photo == 44 and 0 < n_soft < 41
    # xyz: 47 hard legs, the last iteration's alpha step (the hard leg's gradient is still standing), the photometric steps
    assert got["xyz"] == 47 + 1 + n_photo and got["opacity"] == n_soft + 48 + n_photo and got["scaling"] == got["rotation"] == n_photo
    assert neural == [47] * 6


def test_P_after_each_densification_is_the_restatements(runs):
    got = [r["P"] for r in runs["out"] if r["densified"] is not None]
    assert got == runs["ref32"]["P_after_densify"] == runs["ref64"]["P_after_densify"]
    assert [r["P"] for r in runs["out"]] == [e["P"] for e in runs["ref32"]["trace"]]
    assert got[0] != runs["out"][18]["P"]


def test_the_gradients_of_the_first_iteration_are_the_restatements(oracle):
    """one iteration from the same state with the soft leg's start at 0 (the running hard loss is 0.1 loss_hard, under the
    gate): hard, soft, alpha and photometric, each behind its own backward"""
    sc, cams, gts, mono = inputs()
    opt = options(cams, soft_depth_start=0)
    got, want = {}, {}
    tr = make_trainer(oracle, opt=opt)
    tr.after_backward = lambda leg, trainer: got.__setitem__(leg, grads_of(trainer.model.params, trainer.model.P, trainer.neural_parameters()))
    r = tr.train_iteration(1, opt)
    assert r["soft_gate_open"] is True and r["stepped"]["soft"]
    dtu.run(oracle, sc, cams, gts, mono, opt, 1, torch.float32,
            after_backward=lambda leg, it, ref, neural: want.__setitem__(leg, grads_of(ref.p, ref.P, list(neural.parameters()))))
    assert set(got) == set(want) == {"hard", "soft", "alpha", "photometric"}
    for leg, field in (("hard", "xyz"), ("soft", "opacity"), ("alpha", "opacity")):
        assert all(v is None for k, v in want[leg].items() if k != field) and all(v is None for k, v in got[leg].items() if k != field), leg
        e = rel_err(got[leg][field], want[leg][field])
        print("%-5s leg  dL/d%-9s rel err %.2e" % (leg, field, e))
        assert float(want[leg][field].abs().max()) > 0 and e <= TOL, (leg, e)
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


def test_a_checkpoint_carries_the_running_hard_loss(oracle):
    _, cams, _, _ = inputs()
    opt = options(cams)
    a = make_trainer(oracle, opt=opt)
    for it in (1, 2, 3):
        a.train_iteration(it, opt)
    ck = a.checkpoint()
    assert ck["ema_loss_hard"] == a.ema_loss_hard > 0
    b = make_trainer(oracle, opt=opt)
    b.restore(ck)
    assert b.ema_loss_hard == a.ema_loss_hard
    ra, rb = a.train_iteration(4, opt), b.train_iteration(4, opt)
    assert ra["ema_loss_hard"] == rb["ema_loss_hard"] and ra["patches"] == rb["patches"] and ra["camera"] == rb["camera"]
    assert torch.equal(a.model.flat, b.model.flat)


def test_the_options_carry_the_references_defaults_and_its_scan_exceptions():
    o = DngDtuOptions()
    assert isinstance(o, DngOptions) and issubclass(TrainerDNGDTU, TrainerDNG)
    assert o.patch_range == (17, 53) and o.bg_threshold == 30 / 255 and o.bg_run == 50 and o.soft_gate == 0.1 and o.ema == (0.1, 0.9)
    assert o.alpha_leg is True and o.black_rule == (20 / 255, 10, True) and o.white_rule == (240 / 255, 2, 2001)
    assert o.fused_depth_legs is False and o.smooth_start is None and o.near_prune_start is None
    assert (o.iterations, o.soft_depth_start, o.hard_depth_start, o.densify_from_iter, o.opacity_lr) == (30_000, 1000, 0, 500, 0.05)
    s = DngDtuOptions.for_scan("data/dtu/scan110")
    assert s.bg_threshold == 15 / 255 and s.black_rule is None and s.white_rule is None
    for name in ("scan114", "dtu/scan21"):
        s = DngDtuOptions.for_scan(name)
        assert s.bg_threshold == 30 / 255 and s.black_rule == (20 / 255, 10, True) and s.white_rule is None
    s = DngDtuOptions.for_scan("scan8", iterations=6000)
    assert s.white_rule == (240 / 255, 2, 2001) and s.iterations == 6000
    with pytest.raises(TypeError):
        DngDtuOptions(bg_thresholds=0.1)
    # DngOptions itself is what it was
    assert not hasattr(DngOptions(), "bg_threshold") and DngOptions().patch_range == (5, 17)


def test_what_is_closed_to_the_llff_trainer_is_closed_here(oracle):
    with pytest.raises(RuntimeError, match="world_size"):
        make_trainer(oracle, world_size=2)
    with pytest.raises(RuntimeError, match="fused photometric step"):
        make_trainer(oracle, fused_step=True)
    tr = make_trainer(oracle)
    assert not tr.fused_legs_available()
    from gsplat_amd.trainer import GraphedStep
    with pytest.raises(RuntimeError, match="GraphedStep"):
        GraphedStep(tr)
