"""DNGaussian/train_dtu.py:64-247 restated literally, in the reference's order, on top of tests/dng_train_reference.py's pieces
(model, neural stand-in, rasterizer compositions, losses) and tests/dtu_reference.py's statements - the yardstick of
tests/test_dtu_trainer_cpu.py.

What differs from dng_train_reference.run, as in the script:
  * the object mask and the zeroed ground truth are formed EVERY iteration with the literal 49-step loop (in place, on this
    run's own copy of the image), the mono target and both depth images are filled with their unmasked means;
  * no smoothness term; patch_range is the options';
  * ema_loss_hard = 0.1 loss_hard.item() + 0.9 ema_loss_hard, and the soft leg runs iff iteration > soft_depth_start and
    ema_loss_hard < soft_gate - its two randint draws happen only then;
  * the alpha leg, unconditional: render_for_opa, (alpha[bg_mask] ** 2).mean().backward(), optimizer.step(), zero_grad -
    also at the last iteration, where the legs before it have stepped nothing and cleared nothing, so that this one step takes
    every gradient still standing (xyz from the hard leg, opacity from the soft and alpha legs);
  * in front of densify_and_prune the colour rules, on the colour of a SECOND render as the script has it;
  * no near-camera prune.
The fill is applied out of place (tests/dtu_reference.masked_mean_fill: the same values and the same gradient as the script's
in-place assignment into the rasterizer's output)."""
import random

import torch

import dng_train_reference as dtr
import dtu_reference as dr
from gsplat_amd.trainer import expon_lr


def render_for_opa(oracle, cam, ref, bg, dtype):
    """gaussian_renderer/__init__.py:201-269 -> (depth, alpha)"""
    P = ref.P
    scales, rotations, opacity = dtr.activations(ref)
    _, _, depth, alpha, _ = dtr.rasterize(oracle, cam, bg, ref.p["xyz"].detach(), torch.ones((P, 3)), opacity, scales.detach(),
                                          rotations.detach(), dtype)
    return depth, alpha


def depth_loss(depth, mono, p_local, p_global, opt):
    return dtr.depr.depth_regulariser(depth[None], mono, p_local, p_global, opt.error_tolerance, w_local=0.1, w_global=1.0,
                                      w_smooth=0.0)


def rule_now(rule, iteration):
    if rule is None:
        return None
    thr, div, reset = rule
    return thr, div, bool(reset) and iteration % int(reset) == 0


def run(oracle, scene, cams, gts, depth_mono, opt, n_iters, dtype=torch.float32, bg=None, after_backward=None, neural_seed=0):
    """iterations 1 .. n_iters.  opt: gsplat_amd.trainer.DngDtuOptions.  after_backward(leg, iteration, ref, neural) behind each
    backward.  -> dict(trace, P_after_densify, margins, statistic, ema (after each iteration), colours (max_c, min_c of every row
    at each densification, float64), model, neural, steps, neural_steps)"""
    bg = torch.zeros(3) if bg is None else bg
    ref = dtr.make_model(scene, dtype)
    neural = dtr.stand_in_for(scene, dtype, neural_seed)
    nopt = torch.optim.Adam(neural.get_params(opt.neural_grid, opt.neural_net), lr=0.0, eps=1e-15)
    images = [g.clone().to(dtype) for g in gts]        # zeroed in place, as viewpoint_cam.original_image is
    rng = random.Random(opt.seed)
    viewpoint_stack = None
    trace, P_after, margins, statistic, ema_trace, colours = [], [], [], [], [], []
    ema_loss_hard = 0.0

    def step_and_zero():
        ref.optimizer.step()
        nopt.step()
        ref.optimizer.zero_grad(set_to_none=True)
        nopt.zero_grad(set_to_none=True)

    with dtr._default_dtype(dtype):
        for iteration in range(1, n_iters + 1):
            xyz_lr = expon_lr(max(iteration - opt.position_lr_start, 0), dtr.LR["xyz"], opt.position_lr_final,
                              lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
            for g in ref.optimizer.param_groups:
                if g["name"] == "xyz":
                    g["lr"] = xyz_lr
            if not viewpoint_stack:
                viewpoint_stack = list(range(len(cams)))
            ci = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
            cam = cams[ci]
            bg_mask, gt = dr.background_mask(images[ci], opt.bg_threshold, opt.bg_run)
            ev = dict(camera=ci, patches=[None] * 4, xyz_lr=xyz_lr, densified=False, near_pruned=False, cleaned=False,
                      soft_gate_open=None, rule_counts=None, masked=int(bg_mask.sum()))
            s0 = dtr.steps_of(ref)
            nbefore = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            mono = 255.0 - depth_mono[ci].to(dtype).reshape(1, *depth_mono[ci].shape)
            # ---- hard depth
            if iteration > opt.hard_depth_start:
                depth = dtr.render_for_depth(oracle, cam, ref, bg, dtype)
                target = dr.masked_mean_fill(mono, bg_mask)
                depth = dr.masked_mean_fill(depth, bg_mask)
                ev["patches"][0] = rng.randint(*opt.patch_range)
                ev["patches"][1] = rng.randint(*opt.patch_range)
                loss_hard = depth_loss(depth, target[None], ev["patches"][0], ev["patches"][1], opt)
                loss_hard.backward()
                if after_backward is not None:
                    after_backward("hard", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
                ema_loss_hard = opt.ema[0] * loss_hard.item() + opt.ema[1] * ema_loss_hard
            s1 = dtr.steps_of(ref)
            # ---- soft depth
            if iteration > opt.soft_depth_start:
                ev["soft_gate_open"] = ema_loss_hard < opt.soft_gate
            if iteration > opt.soft_depth_start and ema_loss_hard < opt.soft_gate:
                depth, alpha = render_for_opa(oracle, cam, ref, bg, dtype)
                target = dr.masked_mean_fill(mono, bg_mask)
                depth = dr.masked_mean_fill(depth, bg_mask)
                ev["patches"][2] = rng.randint(*opt.patch_range)
                ev["patches"][3] = rng.randint(*opt.patch_range)
                loss_soft = depth_loss(depth, target[None], ev["patches"][2], ev["patches"][3], opt)
                loss_soft.backward()
                if after_backward is not None:
                    after_backward("soft", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
            s2 = dtr.steps_of(ref)
            # ---- alpha
            if opt.alpha_leg:
                depth, alpha = render_for_opa(oracle, cam, ref, bg, dtype)
                (alpha[bg_mask] ** 2).mean().backward()
                if after_backward is not None:
                    after_backward("alpha", iteration, ref, neural)
                step_and_zero()
            s3 = dtr.steps_of(ref)
            # ---- photometric
            pkg = dtr.render(oracle, cam, ref, neural, bg, dtype)
            loss = dtr.photometric_loss(pkg, gt, opt)
            loss.backward()
            if after_backward is not None:
                after_backward("photometric", iteration, ref, neural)
            with torch.no_grad():
                vf, radii, vs = pkg["visibility_filter"], pkg["radii"], pkg["viewspace_points"]
                if iteration in opt.clean_iterations:
                    visible = None
                    for c in cams:
                        f = dtr.render(oracle, c, ref, neural, bg, dtype)["visibility_filter"]
                        visible = f if visible is None else visible | f
                    ref.prune_points(~visible)
                    ev["cleaned"] = True
                if iteration < opt.densify_until_iter and iteration not in opt.clean_iterations:
                    ref.max_radii2D[vf] = torch.max(ref.max_radii2D[vf], radii[vf].to(dtype))
                    ref.xyz_gradient_accum[vf] += torch.norm(vs.grad[vf, :2], dim=-1, keepdim=True).to(dtype)
                    ref.denom[vf] += 1
                    if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                        black, white = rule_now(opt.black_rule, iteration), rule_now(opt.white_rule, iteration)
                        if black is not None or white is not None:
                            color = dtr.render(oracle, cam, ref, neural, bg, dtype)["color"]
                            colours.append((color.max(-1).values.double().clone(), color.min(-1).values.double().clone()))
                            value = dtr.inverse_sigmoid(torch.ones((1,)) * opt.reset_opacity_to)[0]
                            ev["rule_counts"] = dr.colour_rules(color, ref.xyz_gradient_accum, ref.p["opacity"], black, white, value)
                        margins.append(dtr.margin_of(ref, opt))
                        g = ref.xyz_gradient_accum / ref.denom
                        statistic.append(torch.where(g.isnan(), torch.zeros_like(g), g).reshape(-1).double().clone())
                        gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
                        ref.densify_and_prune(opt.densify_grad_threshold, opt.min_opacity, opt.cameras_extent, None,
                                              opt.split_opacity_thresh, None, generator=gen)
                        ev["densified"] = True
                        P_after.append(ref.P)
                if iteration < opt.iterations:
                    step_and_zero()
            now = dtr.steps_of(ref)
            nnow = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            ev["stepped"] = dict(hard=s1["xyz"] > s0["xyz"], soft=s2["opacity"] > s1["opacity"], alpha=s3["opacity"] > s2["opacity"],
                                 gaussians=now["scaling"] > s3["scaling"], neural=nnow[0] > nbefore[0])
            ev["patches"] = tuple(ev["patches"])
            ev["P"] = ref.P
            ev["loss"] = float(loss.detach())
            trace.append(ev)
            ema_trace.append(ema_loss_hard)
    return dict(trace=trace, P_after_densify=P_after, margins=margins, statistic=statistic, ema=ema_trace, colours=colours,
                model=ref, neural=neural, steps=dtr.steps_of(ref),
                neural_steps=[int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()])
