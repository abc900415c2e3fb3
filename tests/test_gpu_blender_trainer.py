"""TrainerDNGBlender and TrainerDNGBlenderSH on the GPU: the scene and compressed schedule of tests/test_blender_trainer_cpu.py
(257 Gaussians, 64 x 48, 4 cameras, one of them without a white pixel) with the real dng_neural.GridRenderer and the HIP kernels
for every piece.  Masks and targets are formed on the device; fused_depth_legs against the un-fused legs over the whole
schedule, both loops, bit for bit; the SH loop's white rule after a densification against white_rule on the colour of a fresh
render_sh-style evaluation, bit for bit; and a plain iteration of either loop makes no synchronising call (counted as
tests/tools/dtu_step_timing.py counts them: torch.cuda.set_sync_debug_mode)."""
import copy
import warnings

import pytest
import torch

import blender_reference as br
import test_blender_trainer_cpu as cpu
from gsplat_amd import dng_blender
from gsplat_amd.trainer import GaussianModelLite, TrainerDNGBlender, TrainerDNGBlenderSH, camera_to
from test_gpu_dng_trainer import assert_same_bits, state_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def gpu_inputs():
    sc, cams, gts, mono = cpu.inputs()
    return sc, [camera_to(c, DEV) for c in cams], [g.to(DEV) for g in gts], [m.to(DEV) for m in mono]


def make_trainer(hip, opt, neural=None, sh=False):
    sc, cams, gts, mono = gpu_inputs()
    model = GaussianModelLite(sc, DEV, api=hip.api)
    model.active_sh_degree = 0
    if sh:
        return TrainerDNGBlenderSH(model, cams, gts, mono, opt=opt)
    return TrainerDNGBlender(model, cams, gts, mono, opt=opt, neural=neural)


def sh_state_of(tr):
    m, o = tr.model, tr.model.optimizer
    out = dict(flat=m.flat, exp_avg=o.exp_avg, exp_avg_sq=o.exp_avg_sq, accum=m.xyz_gradient_accum, denom=m.denom,
               max_radii2D=m.max_radii2D)
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.parametrize("sh", (False, True))
def test_construction_forms_masks_and_targets_on_the_device(hip, sh):
    _, cams, gts, mono = cpu.inputs()
    tr = make_trainer(hip, cpu.sh_options(cams) if sh else cpu.options(cams), sh=sh)
    for ci, gt in enumerate(gts):
        mask = br.background_mask(gt, 254 / 255)
        assert tr.bg_masks[ci].is_cuda and torch.equal(tr.bg_masks[ci].cpu(), mask)
        want = br.depth_target(mono[ci], mask)
        got = tr.mono[ci]
        assert got.is_cuda and got.shape == (1, 1, cpu.H, cpu.W)
        assert torch.equal(got.cpu().reshape(want.shape).view(torch.int32), want.view(torch.int32))
        assert torch.equal(tr.gts[ci].cpu(), gt)                    # the ground truth is not edited
    assert int(tr.bg_masks[3].sum()) == 0 and int(tr.bg_masks[0].sum()) > 0


def test_fused_legs_are_the_unfused_ones_over_the_whole_schedule_bit_for_bit(hip):
    _, cams, _, _ = cpu.inputs()
    fused, plain = cpu.options(cams, fused_depth_legs=True), cpu.options(cams, fused_depth_legs=False)
    a = make_trainer(hip, fused)
    b = make_trainer(hip, plain, neural=copy.deepcopy(a.neural))
    assert a.fused_legs_available()
    assert_same_bits(state_of(a), state_of(b), "before the run")
    ra = [a.train_iteration(it, fused) for it in range(1, cpu.N_ITERS + 1)]
    rb = [b.train_iteration(it, plain) for it in range(1, cpu.N_ITERS + 1)]
    for it, (x, y) in enumerate(zip(ra, rb), 1):
        hard, soft = x["loss_hard"] is not None, x["loss_soft"] is not None
        assert hard == (it % 2 == 0 and it < fused.densify_until_iter) and soft == (hard and it > fused.soft_depth_start)
        assert x["path"] == dict(hard="fused" if hard else None, soft="fused" if soft else None), (it, x["path"])
        assert y["path"] == dict(hard="unfused" if hard else None, soft="unfused" if soft else None), (it, y["path"])
        for k in ("camera", "patches", "xyz_lr", "stepped", "densified", "cleaned", "P", "height_pruned"):
            assert x[k] == y[k], (it, k, x[k], y[k])
        assert (x["rule_count"] is None) == (y["rule_count"] is None)
        if x["rule_count"] is not None:
            assert int(x["rule_count"]) == int(y["rule_count"])
        if hard:
            assert float(x["loss_hard"]) == float(y["loss_hard"]), it
    print("rule counts:", {i + 1: int(r["rule_count"]) for i, r in enumerate(ra) if r["rule_count"] is not None},
          "height prunes:", {i + 1: r["height_pruned"] for i, r in enumerate(ra) if r["height_pruned"] is not None}, "P:", a.model.P)
    assert [it for it, r in enumerate(ra, 1) if r["densified"] is not None] == [20, 30]
    assert ra[-1]["stepped"] == dict(hard=False, soft=False, gaussians=False, neural=False)
    assert dict(a.model.optimizer.seg_steps) == dict(b.model.optimizer.seg_steps)
    assert a.model.optimizer.seg_steps["xyz"] > a.model.optimizer.seg_steps["scaling"] > 0
    assert_same_bits(state_of(a), state_of(b), "after %d iterations" % cpu.N_ITERS)


def test_sh_loop_fused_leg_is_the_unfused_one_over_the_whole_schedule_bit_for_bit(hip):
    _, cams, _, _ = cpu.inputs()
    fused, plain = cpu.sh_options(cams, fused_depth_legs=True), cpu.sh_options(cams, fused_depth_legs=False)
    a, b = make_trainer(hip, fused, sh=True), make_trainer(hip, plain, sh=True)
    assert a.fused_legs_available()
    ra = [a.train_iteration(it, fused) for it in range(1, cpu.N_ITERS + 1)]
    rb = [b.train_iteration(it, plain) for it in range(1, cpu.N_ITERS + 1)]
    for it, (x, y) in enumerate(zip(ra, rb), 1):
        hard = x["loss_hard"] is not None
        assert hard == (it % 2 == 0 and it < fused.densify_until_iter)
        assert x["path"] == ("fused" if hard else None) and y["path"] == ("unfused" if hard else None), (it, x["path"], y["path"])
        for k in ("camera", "patches", "xyz_lr", "sh_degree", "stepped", "densified", "cleaned", "reset", "P", "height_pruned"):
            assert x[k] == y[k], (it, k, x[k], y[k])
        assert (x["rule_count"] is None) == (y["rule_count"] is None)
        if x["rule_count"] is not None:
            assert int(x["rule_count"]) == int(y["rule_count"])
    print("SH loop: densifications", [r["densified"] for r in ra if r["densified"] is not None], "rule counts",
          {i + 1: int(r["rule_count"]) for i, r in enumerate(ra) if r["rule_count"] is not None}, "P:", a.model.P)
    assert [it for it, r in enumerate(ra, 1) if r["reset"]] == [10, 30]
    assert [it for it, r in enumerate(ra, 1) if r["densified"] is not None] == [20, 30]
    assert ra[9]["stepped"] == dict(hard=True, gaussians=True, opacity=False)
    assert dict(a.model.optimizer.seg_steps) == dict(b.model.optimizer.seg_steps)
    s = a.model.optimizer.seg_steps
    assert s["features"] == s["scaling"] == s["opacity"] + 1 > 0
    assert_same_bits(sh_state_of(a), sh_state_of(b), "after %d iterations" % cpu.N_ITERS)


def test_sh_white_rule_after_a_densification_is_white_rule_on_a_fresh_colour(hip):
    """the trainer's call spied on and its inputs copied.  Independent of the kernel: the colour is within 1 ulp of
    tests/blender_reference.sh_colour64 on those inputs - render_sh's statements in float64 -, and the count and the firing rows
    are the float64 colour's wherever that lies farther than 1e-6 from the threshold.  Kernel against kernel, bit for bit: the
    model the trainer left is white_rule applied to that colour, minus the height prune's rows."""
    _, cams, _, _ = cpu.inputs()
    opt = cpu.sh_options(cams)
    tr = make_trainer(hip, opt, sh=True)
    seen = {}

    def spy(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor=0.1, return_colour=False):
        seen.update(xyz=xyz.clone(), shs=shs.clone(), degree=degree, campos=campos.clone(), stat=stat.clone(),
                    opacity=opacity_raw.clone(), threshold=threshold, factor=factor)
        return dng_blender.white_rule_sh(xyz, shs, degree, campos, stat, opacity_raw, threshold, factor, return_colour)
    tr._white_rule_sh = spy
    for it in range(1, 21):
        r = tr.train_iteration(it, opt)
    assert r["densified"] is not None and seen["degree"] == 1 and seen["threshold"] == opt.white_rule[0]
    s0, o0 = seen["stat"].clone(), seen["opacity"].clone()
    n0, colour = dng_blender.white_rule_sh(seen["xyz"], seen["shs"], 1, seen["campos"], s0, o0, float("inf"), return_colour=True)
    assert int(n0[0]) == 0 and torch.equal(o0.view(torch.int32), seen["opacity"].view(torch.int32))
    assert torch.equal(colour.view(torch.int32), tr.last_colour.view(torch.int32))
    n = dng_blender.white_rule(colour, s0, o0, *opt.white_rule)
    assert int(n[0]) == int(r["rule_count"][0]) > 0
    # the model the trainer left = those rows minus the height prune's
    keep = ~(seen["xyz"][:, -1] < opt.height_prune)
    assert int(keep.sum()) == tr.model.P
    assert torch.equal(tr.model.params["opacity"].detach().view(torch.int32), o0[keep].view(torch.int32))
    c64 = br.sh_colour64(seen["xyz"].cpu(), seen["shs"].cpu(), 1, seen["campos"].cpu())
    assert float(((colour.cpu().double() - c64).abs() / br.spacing(c64)).max()) <= 1.0
    mn64 = c64.min(-1).values
    thr = float(torch.tensor(opt.white_rule[0], dtype=torch.float32))
    clear = (mn64 - thr).abs() > 1e-6                               # (an fp32 colour near 0.6 is 6e-8 apart from its neighbour)
    fired = (o0 != seen["opacity"]).reshape(-1).cpu()
    assert torch.equal(fired[clear], (mn64 > thr)[clear])
    assert abs(int(n[0]) - int((mn64 > thr).sum())) <= int((~clear).sum())


@pytest.mark.parametrize("sh", (False, True))
def test_a_plain_iteration_makes_no_synchronising_call(hip, sh):
    """iterations 2 .. 9 of the schedule: legs on the even ones, no densification, clean or reset"""
    _, cams, _, _ = cpu.inputs()
    opt = cpu.sh_options(cams) if sh else cpu.options(cams)
    tr = make_trainer(hip, opt, sh=sh)
    tr.train_iteration(1, opt)        # (the clean: its prune reads a count back)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = [tr.train_iteration(it, opt) for it in range(2, 10)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    stalls = [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]
    assert sum(1 for r in out if r["loss_hard"] is not None) == 4
    assert not stalls, stalls[:3]
