"""TrainerDNGDTU on the GPU: the scene and compressed schedule of tests/test_dtu_trainer_cpu.py (257 Gaussians, 64 x 48, 4
cameras, one of them with an empty mask) with the real dng_neural.GridRenderer and the HIP kernels for every piece.  The
alpha leg fused (depth_pass.depth_leg_step) against depth_pass -> alpha_penalty -> backward -> gs_adam_step, and the whole
schedule with fused_depth_legs against the un-fused legs from the same state: bit for bit."""
import copy

import pytest
import torch

import dtu_reference as dr
import test_dtu_trainer_cpu as cpu
from gsplat_amd.trainer import GaussianModelLite, TrainerDNGDTU, camera_to
from test_gpu_dng_trainer import assert_same_bits, state_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def gpu_inputs():
    sc, cams, gts, mono = cpu.inputs()
    return sc, [camera_to(c, DEV) for c in cams], [g.to(DEV) for g in gts], [m.to(DEV) for m in mono]


def make_trainer(hip, opt, neural=None):
    sc, cams, gts, mono = gpu_inputs()
    model = GaussianModelLite(sc, DEV, api=hip.api)
    model.active_sh_degree = 0
    return TrainerDNGDTU(model, cams, gts, mono, opt=opt, neural=neural)


def test_construction_forms_masks_zeroed_images_and_filled_targets_on_the_device(hip):
    _, cams, gts, mono = cpu.inputs()
    tr = make_trainer(hip, cpu.options(cams))
    for ci, gt in enumerate(gts):
        mask, zeroed = dr.background_mask(gt.clone(), cpu.BG_THRESHOLD, 50)
        assert tr.bg_masks[ci].is_cuda and torch.equal(tr.bg_masks[ci].cpu(), mask)
        assert torch.equal(tr.gts[ci].cpu().view(torch.int32), zeroed.view(torch.int32))
        target = (255.0 - mono[ci]).reshape(1, cpu.H, cpu.W)
        got = tr.mono[ci].cpu().reshape(1, cpu.H, cpu.W)
        assert torch.equal(got[~mask].view(torch.int32), target[~mask].view(torch.int32))
        if int(mask.sum()):
            want = float(target.double()[~mask].mean())
            assert abs(float(got[mask][0]) - want) <= dr.ulp(want) and bool((got[mask] == got[mask][0]).all())
    assert int(tr.bg_masks[3].sum()) == 0 and int(tr.bg_masks[0].sum()) > 0


def test_the_fused_alpha_leg_is_pass_penalty_backward_adam_bit_for_bit(hip):
    """two alpha legs in a row from the same state - a mask holding pixels (camera 0), then an empty one (camera 3: a NaN
    loss, a zero cotangent, and a step that the first leg's moments still move) - fused against un-fused: the opacity rows,
    both moments and everything else the same bits"""
    _, cams, _, _ = cpu.inputs()
    fused, plain = cpu.options(cams, fused_depth_legs=True), cpu.options(cams, fused_depth_legs=False)
    a = make_trainer(hip, fused)
    b = make_trainer(hip, plain, neural=copy.deepcopy(a.neural))
    assert a.fused_legs_available()
    P = a.model.P
    for ci in (0, 3):
        before = state_of(a)
        assert_same_bits(before, state_of(b), "before camera %d" % ci)
        losses = []
        for tr, opt, want in ((a, fused, "fused"), (b, plain, "unfused")):
            tr._set_rates(1, opt)
            loss, path = tr._depth_leg(ci, "opacity", None, None, 0.0, opt, True, leg="alpha")
            assert path == want
            losses.append(loss)
        if ci == 3:
            assert bool(losses[0].isnan()) and bool(losses[1].isnan())
        else:
            assert float(losses[0]) == float(losses[1]) > 0
        after = state_of(a)
        assert_same_bits(after, state_of(b), "after camera %d" % ci)
        moved = (after["flat"] != before["flat"]).nonzero().reshape(-1)
        assert moved.numel() > 0 and int(moved.min()) >= 51 * P and int(moved.max()) < 52 * P   # the opacity rows alone
        assert a.model.optimizer.seg_steps == b.model.optimizer.seg_steps
    assert a.model.optimizer.seg_steps["opacity"] == 2 and a.model.optimizer.seg_steps["xyz"] == 0


def test_fused_legs_are_the_unfused_ones_over_the_whole_schedule_bit_for_bit(hip):
    _, cams, _, _ = cpu.inputs()
    fused, plain = cpu.options(cams, fused_depth_legs=True), cpu.options(cams, fused_depth_legs=False)
    a = make_trainer(hip, fused)
    b = make_trainer(hip, plain, neural=copy.deepcopy(a.neural))
    assert_same_bits(state_of(a), state_of(b), "before the run")
    ra = [a.train_iteration(it, fused) for it in range(1, cpu.N_ITERS + 1)]
    rb = [b.train_iteration(it, plain) for it in range(1, cpu.N_ITERS + 1)]
    for it, (x, y) in enumerate(zip(ra, rb), 1):
        last = it == cpu.N_ITERS    # the last iteration: one un-fused step for every gradient left standing
        soft = x["loss_soft"] is not None
        f = "unfused" if last else "fused"
        assert x["path"] == dict(hard=f, soft=f if soft else None, alpha=f), (it, x["path"])
        assert y["path"] == dict(hard="unfused", soft="unfused" if soft else None, alpha="unfused"), (it, y["path"])
        for k in ("camera", "patches", "xyz_lr", "stepped", "densified", "cleaned", "P", "soft_gate_open", "ema_loss_hard"):
            assert x[k] == y[k], (it, k, x[k], y[k])
        assert (x["rule_counts"] is None) == (y["rule_counts"] is None)
        if x["rule_counts"] is not None:
            assert x["rule_counts"].tolist() == y["rule_counts"].tolist()
        assert float(x["loss_hard"]) == float(y["loss_hard"]), it
    gates = [r["soft_gate_open"] for r in ra]
    print("gate:", gates, "rule counts:", {i + 1: r["rule_counts"].tolist() for i, r in enumerate(ra) if r["rule_counts"] is not None},
          "P:", a.model.P)
    assert gates[:6] == [None] * 6
    assert [it for it, r in enumerate(ra, 1) if r["densified"] is not None] == [20, 30]
    assert ra[-1]["stepped"] == dict(hard=False, soft=False, alpha=True, gaussians=False, neural=False)
    assert dict(a.model.optimizer.seg_steps) == dict(b.model.optimizer.seg_steps)
    assert a.model.optimizer.seg_steps["opacity"] > a.model.optimizer.seg_steps["scaling"] > 0
    assert_same_bits(state_of(a), state_of(b), "after %d iterations" % cpu.N_ITERS)


def test_a_checkpoint_round_trip_carries_the_running_hard_loss(hip):
    _, cams, _, _ = cpu.inputs()
    opt = cpu.options(cams)
    a = make_trainer(hip, opt)
    for it in range(1, 5):
        a.train_iteration(it, opt)
    ck = a.checkpoint()
    ra = a.train_iteration(5, opt)
    b = make_trainer(hip, opt, neural=copy.deepcopy(a.neural))
    b.restore(ck)
    assert b.ema_loss_hard == ck["ema_loss_hard"] > 0
    rb = b.train_iteration(5, opt)
    for k in ("camera", "patches", "stepped", "P", "ema_loss_hard"):
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert_same_bits(state_of(a), state_of(b), "iteration 5 after the round trip")
