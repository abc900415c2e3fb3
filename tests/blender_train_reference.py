"""DNGaussian/train_blender.py:66-228 (`training`, the neural loop) restated literally, in the reference's order, on top of
tests/dng_train_reference.py's pieces (model, neural stand-in, rasterizer compositions, losses) and
tests/blender_reference.py's statements - the yardstick of tests/test_blender_trainer_cpu.py.

What differs from dng_train_reference.run, as in the script:
  * the background mask is formed EVERY iteration, and the mono target 255 - depth_mono with the masked pixels zero again in
    each leg; the depth image is not masked;
  * the legs run only when iteration < densify_until_iter and iteration % depth_leg_interval == 0; no smoothness term;
  * loss_reg *= reg_decay once iteration > densify_until_iter;
  * in front of densify_and_prune the white rule, on the colour of a SECOND render as the script has it; behind it the height
    prune; no near-camera prune.
run_sh restates `training_sh` (:265-388) the same way on a plain SH model (scene/gaussian_model_sh.py: six Adam groups, f_dc and
f_rest apart; densify_and_prune without an opacity gate and with the world-size prune beside the screen-size one; reset_opacity
through replace_tensor_to_optimizer): the SH ramp, the hard leg alone, render_sh with the rasterizer evaluating the SH rows,
L1 + lambda_dssim (1 - SSIM), the white rule AFTER the densification on render_sh's "color" of the re-laid-out model, the height
prune, the opacity reset every opacity_reset_interval and at densify_from_iter."""
import math
import random

import torch

import blender_reference as br
import dng_train_reference as dtr
from gsplat_amd.trainer import expon_lr


def depth_loss(depth, mono, p_local, p_global, opt):
    return dtr.depr.depth_regulariser(depth[None], mono, p_local, p_global, opt.error_tolerance, w_local=0.1, w_global=1.0,
                                      w_smooth=0.0)


def photometric_loss(pkg, gt, opt, iteration):
    loss = dtr.l1_loss(pkg["render"], gt) + opt.lambda_dssim * (1.0 - dtr.ssim(pkg["render"], gt))
    t = dtr.rgr.terms(pkg["scales"], pkg["opacity"])
    loss_reg = opt.shape_pena * t[0] + opt.scale_pena * t[1] + opt.opa_pena * t[2]
    if iteration > opt.densify_until_iter:
        loss_reg = loss_reg * opt.reg_decay
    return loss + loss_reg


def run(oracle, scene, cams, gts, depth_mono, opt, n_iters, dtype=torch.float32, bg=None, after_backward=None, neural_seed=0):
    """iterations 1 .. n_iters.  opt: gsplat_amd.trainer.DngBlenderOptions.  after_backward(leg, iteration, ref, neural) behind
    each backward.  -> dict(trace, P_after_densify, margins, statistic, colours (min_c of every row at each densification,
    float64), heights (the last coordinate at each height prune, float64), model, neural, steps, neural_steps)"""
    bg = torch.ones(3) if bg is None else bg
    ref = dtr.make_model(scene, dtype)
    neural = dtr.stand_in_for(scene, dtype, neural_seed)
    nopt = torch.optim.Adam(neural.get_params(opt.neural_grid, opt.neural_net), lr=0.0, eps=1e-15)
    rng = random.Random(opt.seed)
    viewpoint_stack = None
    trace, P_after, margins, statistic, colours, heights = [], [], [], [], [], []

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
            gt_image = gts[ci].to(dtype)
            bg_mask = br.background_mask(gt_image, opt.bg_threshold)
            ev = dict(camera=ci, patches=[None] * 4, xyz_lr=xyz_lr, densified=False, cleaned=False, rule_count=None,
                      height_pruned=None, masked=int(bg_mask.sum()))
            s0 = dtr.steps_of(ref)
            nbefore = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            stored = depth_mono[ci].to(dtype).reshape(1, *depth_mono[ci].shape)
            # ---- hard depth
            if iteration > opt.hard_depth_start and iteration < opt.densify_until_iter and iteration % opt.depth_leg_interval == 0:
                depth = dtr.render_for_depth(oracle, cam, ref, bg, dtype)
                target = br.depth_target(stored, bg_mask)
                ev["patches"][0] = rng.randint(*opt.patch_range)
                ev["patches"][1] = rng.randint(*opt.patch_range)
                loss_hard = depth_loss(depth, target[None], ev["patches"][0], ev["patches"][1], opt)
                loss_hard.backward()
                if after_backward is not None:
                    after_backward("hard", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
            s1 = dtr.steps_of(ref)
            # ---- soft depth
            if iteration > opt.soft_depth_start and iteration < opt.densify_until_iter and iteration % opt.depth_leg_interval == 0:
                depth = dtr.render_for_opa(oracle, cam, ref, bg, dtype)
                target = br.depth_target(stored, bg_mask)
                ev["patches"][2] = rng.randint(*opt.patch_range)
                ev["patches"][3] = rng.randint(*opt.patch_range)
                loss_soft = depth_loss(depth, target[None], ev["patches"][2], ev["patches"][3], opt)
                loss_soft.backward()
                if after_backward is not None:
                    after_backward("soft", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
            s2 = dtr.steps_of(ref)
            # ---- photometric
            pkg = dtr.render(oracle, cam, ref, neural, bg, dtype)
            loss = photometric_loss(pkg, gt_image, opt, iteration)
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
                        if opt.white_rule is not None:
                            color = dtr.render(oracle, cam, ref, neural, bg, dtype)["color"]
                            colours.append(color.min(-1).values.double().clone())
                            ev["rule_count"] = br.white_rule(color, ref.xyz_gradient_accum, ref.p["opacity"], *opt.white_rule)
                        margins.append(dtr.margin_of(ref, opt))
                        g = ref.xyz_gradient_accum / ref.denom
                        statistic.append(torch.where(g.isnan(), torch.zeros_like(g), g).reshape(-1).double().clone())
                        gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
                        ref.densify_and_prune(opt.densify_grad_threshold, opt.min_opacity, opt.cameras_extent, None,
                                              opt.split_opacity_thresh, None, generator=gen)
                        ev["densified"] = True
                        if opt.height_prune is not None:
                            heights.append(ref.p["xyz"][:, -1].double().clone())
                            before = ref.P
                            ref.prune_points(ref.p["xyz"][:, -1] < opt.height_prune)
                            ev["height_pruned"] = before - ref.P
                        P_after.append(ref.P)
                if iteration < opt.iterations:
                    step_and_zero()
            now = dtr.steps_of(ref)
            nnow = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            ev["stepped"] = dict(hard=s1["xyz"] > s0["xyz"], soft=s2["opacity"] > s1["opacity"],
                                 gaussians=now["scaling"] > s2["scaling"], neural=nnow[0] > nbefore[0])
            ev["patches"] = tuple(ev["patches"])
            ev["P"] = ref.P
            ev["loss"] = float(loss.detach())
            trace.append(ev)
    return dict(trace=trace, P_after_densify=P_after, margins=margins, statistic=statistic, colours=colours, heights=heights,
                model=ref, neural=neural, steps=dtr.steps_of(ref),
                neural_steps=[int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()])


# ---------------------------------------------------------------------------------------------------------------- training_sh
LR_SH = dict(xyz=0.00016, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)
SH_FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


class ReferenceSH(dtr.ddr.Reference):
    """scene/gaussian_model_sh.py on plain tensors: Reference's optimizer surgery with GaussianModelSH's densification rule"""

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, generator=None):
        """gaussian_model_sh.py:389-401 -> (n_clone, n_split, n_pruned)"""
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        # (densify_and_clone / densify_and_split, :349-387: Reference's with a gate every opacity passes)
        n_clone = self.densify_and_clone(grads, max_grad, extent, -1.0)
        n_split = self.densify_and_split(grads, max_grad, extent, -1.0, generator)
        prune_mask = (self.get_opacity < min_opacity).squeeze(1)
        if max_screen_size:
            big_points_vs = self.max_radii2D > max_screen_size
            big_points_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
        self.prune_points(prune_mask)
        return n_clone, n_split, int(prune_mask.sum())


def make_sh_model(scene, dtype):
    op = scene["opacities"].float().clamp(1e-6, 1 - 1e-6)
    shs = scene["shs"].float()
    P = shs.shape[0]
    raw = dict(xyz=scene["means3D"].float(), f_dc=shs[:, :1, :].reshape(P, 3), f_rest=shs[:, 1:, :].reshape(P, 45),
               opacity=dtr.inverse_sigmoid(op).reshape(-1, 1), scaling=torch.log(scene["scales"].float()),
               rotation=scene["rotations"].float())
    raw = {k: raw[k].to(dtype) for k in SH_FIELDS}
    zeros = {k: torch.zeros_like(v) for k, v in raw.items()}
    ref = ReferenceSH(raw, zeros, zeros, torch.zeros((P, 1), dtype=dtype), torch.zeros((P, 1), dtype=dtype),
                      torch.zeros((P,), dtype=dtype))
    for g in ref.optimizer.param_groups:
        g["lr"] = LR_SH[g["name"]]
    return ref


def features_of(ref):
    """get_features: cat(_features_dc, _features_rest) -> [P,16,3]"""
    P = ref.P
    return torch.cat((ref.p["f_dc"].reshape(P, 1, 3), ref.p["f_rest"].reshape(P, 15, 3)), dim=1)


def flat_of_sh(ref):
    """the parameters in GaussianModelLite's flat order (xyz, features [P,16,3], opacity, scaling, rotation)"""
    return torch.cat([ref.p["xyz"].detach().reshape(-1), features_of(ref).detach().reshape(-1), ref.p["opacity"].detach().reshape(-1),
                      ref.p["scaling"].detach().reshape(-1), ref.p["rotation"].detach().reshape(-1)])


def render_sh(oracle, cam, ref, bg, dtype, sh_degree):
    """gaussian_renderer/__init__.py:285-367 on the checker's FSGS rasterizer (float32 copies; autograd carries the gradients
    back into `dtype`), without the "color" key (sh_colour below, where the loop reads it)"""
    P = ref.P
    scales, rotations, opacity = dtr.activations(ref)
    xyz32 = ref.p["xyz"].float()
    screenspace_points = torch.zeros_like(xyz32, requires_grad=True) + 0
    if screenspace_points.requires_grad:
        screenspace_points.retain_grad()
    rs = oracle.FsgsSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=False,
        confidence=torch.ones((P, 1)))
    image, radii, depth, alpha = oracle.FsgsRasterizer(raster_settings=rs)(
        means3D=xyz32, means2D=screenspace_points, shs=features_of(ref).float(), colors_precomp=None, opacities=opacity.float(),
        scales=scales.float(), rotations=rotations.float(), cov3D_precomp=None)
    return dict(render=image.to(dtype), depth=depth.to(dtype), alpha=alpha.to(dtype), viewspace_points=screenspace_points,
                visibility_filter=radii > 0, radii=radii, opacity=opacity)


def run_sh(oracle, scene, cams, gts, depth_mono, opt, n_iters, dtype=torch.float32, bg=None, after_backward=None, sh_degree=0):
    """iterations 1 .. n_iters of training_sh.  opt: DngBlenderOptions(use_sh=True).  after_backward(leg, iteration, ref).
    -> dict(trace, P_after_densify, statistic, colours, heights, model, steps)"""
    bg = torch.ones(3) if bg is None else bg
    ref = make_sh_model(scene, dtype)
    active_sh_degree, max_sh_degree = sh_degree, 3
    rng = random.Random(opt.seed)
    viewpoint_stack = None
    trace, P_after, statistic, colours, heights = [], [], [], [], []

    def step_and_zero():
        ref.optimizer.step()
        ref.optimizer.zero_grad(set_to_none=True)

    with dtr._default_dtype(dtype):
        for iteration in range(1, n_iters + 1):
            xyz_lr = expon_lr(max(iteration - opt.position_lr_start, 0), LR_SH["xyz"], opt.position_lr_final,
                              lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
            for g in ref.optimizer.param_groups:
                if g["name"] == "xyz":
                    g["lr"] = xyz_lr
            if iteration % opt.sh_increase_interval == 0:
                if active_sh_degree < max_sh_degree:
                    active_sh_degree += 1
            if not viewpoint_stack:
                viewpoint_stack = list(range(len(cams)))
            ci = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
            cam = cams[ci]
            gt_image = gts[ci].to(dtype)
            bg_mask = br.background_mask(gt_image, opt.bg_threshold)
            ev = dict(camera=ci, patches=[None] * 2, xyz_lr=xyz_lr, sh_degree=active_sh_degree, densified=False, cleaned=False,
                      reset=False, rule_count=None, height_pruned=None, masked=int(bg_mask.sum()))
            s0 = dtr.steps_of(ref)
            stored = depth_mono[ci].to(dtype).reshape(1, *depth_mono[ci].shape)
            # ---- depth
            if iteration > opt.hard_depth_start and iteration < opt.densify_until_iter and iteration % opt.depth_leg_interval == 0:
                depth = dtr.render_for_depth(oracle, cam, ref, bg, dtype)
                target = br.depth_target(stored, bg_mask)
                ev["patches"][0] = rng.randint(*opt.patch_range)
                ev["patches"][1] = rng.randint(*opt.patch_range)
                loss_hard = depth_loss(depth, target[None], ev["patches"][0], ev["patches"][1], opt)
                loss_hard.backward()
                if after_backward is not None:
                    after_backward("hard", iteration, ref)
                if iteration < opt.iterations:
                    step_and_zero()
            s1 = dtr.steps_of(ref)
            # ---- photometric
            pkg = render_sh(oracle, cam, ref, bg, dtype, active_sh_degree)
            image = pkg["render"]
            loss = dtr.l1_loss(image, gt_image) + opt.lambda_dssim * (1.0 - dtr.ssim(image, gt_image))
            loss.backward()
            if after_backward is not None:
                after_backward("photometric", iteration, ref)
            with torch.no_grad():
                vf, radii, vs = pkg["visibility_filter"], pkg["radii"], pkg["viewspace_points"]
                if iteration in opt.clean_iterations:
                    visible = None
                    for c in cams:
                        f = render_sh(oracle, c, ref, bg, dtype, active_sh_degree)["visibility_filter"]
                        visible = f if visible is None else visible | f
                    ref.prune_points(~visible)
                    ev["cleaned"] = True
                if iteration < opt.densify_until_iter and iteration not in opt.clean_iterations:
                    ref.max_radii2D[vf] = torch.max(ref.max_radii2D[vf], radii[vf].to(dtype))
                    ref.xyz_gradient_accum[vf] += torch.norm(vs.grad[vf, :2], dim=-1, keepdim=True).to(dtype)
                    ref.denom[vf] += 1
                    if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                        size_threshold = opt.size_threshold if iteration > opt.opacity_reset_interval else None
                        g = ref.xyz_gradient_accum / ref.denom
                        statistic.append(torch.where(g.isnan(), torch.zeros_like(g), g).reshape(-1).double().clone())
                        gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
                        ref.densify_and_prune(opt.densify_grad_threshold, opt.prune_opacity, opt.cameras_extent, size_threshold,
                                              generator=gen)
                        ev["densified"] = True
                        if opt.white_rule is not None:
                            color = br.sh_colour(ref.p["xyz"].detach(), features_of(ref).detach(), active_sh_degree,
                                                 cam.camera_center.to(dtype))
                            colours.append(color.min(-1).values.double().clone())
                            ev["rule_count"] = br.white_rule(color, ref.xyz_gradient_accum, ref.p["opacity"], *opt.white_rule)
                        if opt.height_prune is not None:
                            heights.append(ref.p["xyz"][:, -1].double().clone())
                            before = ref.P
                            ref.prune_points(ref.p["xyz"][:, -1] < opt.height_prune)
                            ev["height_pruned"] = before - ref.P
                        P_after.append(ref.P)
                    if iteration % opt.opacity_reset_interval == 0 or (
                            opt.white_background and opt.reset_at_densify_from and iteration == opt.densify_from_iter):
                        ref.reset_opacity()
                        ev["reset"] = True
                if iteration < opt.iterations:
                    step_and_zero()
            now = dtr.steps_of(ref)
            ev["stepped"] = dict(hard=s1["xyz"] > s0["xyz"], gaussians=now["scaling"] > s1["scaling"],
                                 opacity=now["opacity"] > s1["opacity"])
            ev["patches"] = tuple(ev["patches"])
            ev["P"] = ref.P
            ev["loss"] = float(loss.detach())
            trace.append(ev)
    return dict(trace=trace, P_after_densify=P_after, statistic=statistic, colours=colours, heights=heights, model=ref,
                steps=dtr.steps_of(ref))
