"""DNGaussian/train_llff.py:68-228 restated literally, in the reference's order - the yardstick of tests/test_dng_trainer_cpu.py
and tests/test_gpu_dng_trainer.py.

  * the per-Gaussian model is tests/dng_densify_reference.Reference: one leaf tensor and one torch.optim.Adam(lr=0, eps=1e-15)
    group per field, whose prune_points / densify_and_prune re-register every tensor (so that its gradient is gone and
    optimizer.step() skips it), and `optimizer.zero_grad(set_to_none=True)` after every step;
  * the neural renderer's three groups live in a second torch.optim.Adam with the same hyper-parameters, stepped wherever the
    reference's one optimizer is: torch skips a parameter whose gradient is None, so two optimizers stepped together are one
    (Reference's optimizer surgery walks every group of its optimizer as a per-Gaussian one);
  * the hard and soft legs are the reference's render_for_depth / render_for_opa compositions on the checker's FSGS rasterizer
    (colours of ones, opacity 0.95 / the model's, the other inputs detached), the loss tests/dng_depth_reference's
    depth_regulariser, the regulariser tests/dng_reg_reference's terms, view directions and near mask that file's too;
  * L1 and SSIM are plain torch (tests/fsgs_train_reference.py's);
  * `dtype`: float32, or the float64 TWIN - losses, neural renderer and optimizer arithmetic (parameters, moments, statistics,
    densification) in float64; the rasterizer stays the float32 checker, fed the rounded parameters;
  * not carried, as in the product: the `_features [P,32]` and `_depth_err [P,1]` groups, which never get a gradient.

StandInGrid is the small neural renderer both sides of a test use behind the `neural` interface: tests/encoding_reference's
hash grid (4 levels, table 2^10, 2 features) and degree-4 SH into tests/neural_reference's two heads."""
import contextlib
import math
import random

import torch

import dng_densify_reference as ddr
import dng_depth_reference as depr
import dng_reg_reference as rgr
import encoding_reference as er
import neural_reference as nr
from fsgs_train_reference import l1_loss, ssim
from gsplat_amd.trainer import expon_lr

LR = dict(xyz=0.00016, features=0.0025, opacity=0.05, scaling=0.005, rotation=0.001)   # arguments/__init__.py:78-87
FIELDS = (("xyz", 3), ("features", 48), ("opacity", 1), ("scaling", 3), ("rotation", 4))
GAUSSIAN = ("xyz", "opacity", "scaling", "rotation")


class StandInGrid(torch.nn.Module):
    """forward(x [N,3], d [N,3] unit) -> (sigma [N], colour [N,3]); get_params(lr, lr_net) -> DNGaussian's three groups."""
    L, C, H0, LOG2_T, RES = 4, 2, 4, 10, 32

    def __init__(self, bound, coord_center, dtype=torch.float32, seed=0):
        super().__init__()
        self.dtype = dtype
        self.register_buffer("bound", torch.as_tensor(bound, dtype=torch.float32).detach())
        self.register_buffer("coord_center", torch.as_tensor(coord_center, dtype=torch.float32).detach())
        self.scale = er.per_level_scale_of(self.L, self.H0, desired_resolution=self.RES)
        self.offsets = er.grid_offsets(3, self.L, self.scale, self.H0, self.LOG2_T, False)
        g = torch.Generator().manual_seed(seed)
        self.embeddings = torch.nn.Parameter(((torch.rand((self.offsets[-1], self.C), generator=g) * 2 - 1) * 0.3).to(dtype))
        shapes = ((64, self.L * self.C), (64, 64), (65, 64), (64, 80), (3, 64))
        self.w = torch.nn.ParameterList(
            [torch.nn.Parameter(((torch.rand(s, generator=g) * 2 - 1) / math.sqrt(s[1])).to(dtype)) for s in shapes])

    def forward(self, x, d):
        x = x.to(self.dtype)
        u = (x - self.coord_center.to(self.dtype) + self.bound.to(self.dtype)) / (2 * self.bound.to(self.dtype))
        enc_x = er.grid_encode_ref(u, self.embeddings, self.offsets, self.scale, self.H0, dtype=self.dtype)
        enc_d = er.sh_encode_ref(d.to(self.dtype), 4, dtype=self.dtype)
        return nr.torch_chain(enc_x, enc_d, list(self.w))

    def get_params(self, lr, lr_net, wd=0):
        return [{"params": [self.embeddings], "name": "neural_encoder", "lr": lr},
                {"params": list(self.w[:3]), "name": "neural_sigma", "lr": lr_net, "weight_decay": wd},
                {"params": list(self.w[3:]), "name": "neural_color", "lr": lr_net, "weight_decay": wd}]


def stand_in_for(scene, dtype=torch.float32, seed=0):
    """gaussian_model.py:197-200: bound = (max - min).max() / 2 * 1.2 and coord_center = mean(xyz), fixed at creation"""
    xyz = scene["means3D"].float()
    return StandInGrid(float((xyz.max(0).values - xyz.min(0).values).max()) / 2 * 1.2, xyz.mean(0), dtype, seed)


@contextlib.contextmanager
def _default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def make_model(scene, dtype):
    """tests/dng_densify_reference.Reference of a gsplat_amd.synthetic scene (GaussianModelLite's input), zero Adam state"""
    op = scene["opacities"].float().clamp(1e-6, 1 - 1e-6)
    raw = dict(xyz=scene["means3D"].float(), features=scene["shs"].float().reshape(-1, 48), opacity=inverse_sigmoid(op).reshape(-1, 1),
               scaling=torch.log(scene["scales"].float()), rotation=scene["rotations"].float())
    raw = {k: v.to(dtype) for k, v in raw.items()}
    P = raw["xyz"].shape[0]
    zeros = {k: torch.zeros_like(v) for k, v in raw.items()}
    ref = ddr.Reference(raw, zeros, zeros, torch.zeros((P, 1), dtype=dtype), torch.zeros((P, 1), dtype=dtype),
                        torch.zeros((P,), dtype=dtype))
    for g in ref.optimizer.param_groups:
        g["lr"] = LR[g["name"]]
    return ref


def steps_of(ref):
    return {k: int(ref.optimizer.state[ref.p[k]]["step"]) for k in ref.names}


def flat_of(ref):
    """the parameters in GaussianModelLite's flat order"""
    return torch.cat([ref.p[k].detach().reshape(-1) for k, _ in FIELDS])


def settings(oracle, cam, bg, P):
    return oracle.FsgsSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center, prefiltered=False, debug=False,
        confidence=torch.ones((P, 1)))


def rasterize(oracle, cam, bg, xyz, colours, opacity, scales, rotations, dtype):
    """the checker's FSGS rasterizer on float32 copies (autograd carries the gradients back into `dtype`)"""
    xyz32 = xyz.float()
    screenspace_points = torch.zeros_like(xyz32, requires_grad=True) + 0
    if screenspace_points.requires_grad:   # (not under clean_views' no_grad)
        screenspace_points.retain_grad()
    image, radii, depth, alpha = oracle.FsgsRasterizer(raster_settings=settings(oracle, cam, bg, xyz.shape[0]))(
        means3D=xyz32, means2D=screenspace_points, shs=None, colors_precomp=colours.float(), opacities=opacity.float(),
        scales=scales.float(), rotations=rotations.float(), cov3D_precomp=None)
    return image.to(dtype), radii, depth.to(dtype), alpha.to(dtype), screenspace_points


def activations(ref):
    return torch.exp(ref.p["scaling"]), torch.nn.functional.normalize(ref.p["rotation"]), torch.sigmoid(ref.p["opacity"])


def render_for_depth(oracle, cam, ref, bg, dtype):
    """gaussian_renderer/__init__.py:128-197: colours of ones, opacity 0.95, everything but the means detached"""
    P = ref.P
    scales, rotations, _ = activations(ref)
    _, _, depth, _, _ = rasterize(oracle, cam, bg, ref.p["xyz"], torch.ones((P, 3)), torch.ones((P, 1)) * 0.95, scales.detach(),
                                  rotations.detach(), dtype)
    return depth


def render_for_opa(oracle, cam, ref, bg, dtype):
    """gaussian_renderer/__init__.py:201-269: colours of ones, the model's opacity, everything else detached"""
    P = ref.P
    scales, rotations, opacity = activations(ref)
    _, _, depth, _, _ = rasterize(oracle, cam, bg, ref.p["xyz"].detach(), torch.ones((P, 3)), opacity, scales.detach(),
                                  rotations.detach(), dtype)
    return depth


def render(oracle, cam, ref, neural, bg, dtype):
    """gaussian_renderer/__init__.py:21-123"""
    xyz = ref.p["xyz"]
    dirs = rgr.view_dirs(xyz, cam.camera_center.to(dtype))
    sigma, colour = neural(xyz, dirs)
    scales, rotations, opacity = activations(ref)   # combine_opacity: the model's own opacity, sigma unused
    image, radii, depth, alpha, ssp = rasterize(oracle, cam, bg, xyz, colour, opacity, scales, rotations, dtype)
    return dict(render=image, depth=depth, alpha=alpha, viewspace_points=ssp, visibility_filter=radii > 0, radii=radii,
                opacity=opacity, color=colour, scales=scales)


def depth_loss(depth, mono, p_local, p_global, opt, iteration):
    return depr.depth_regulariser(depth[None], mono, p_local, p_global, opt.error_tolerance, w_local=0.1, w_global=1.0,
                                  w_smooth=0.1 if iteration > opt.smooth_start else 0.0)


def photometric_loss(pkg, gt, opt):
    loss = l1_loss(pkg["render"], gt) + opt.lambda_dssim * (1.0 - ssim(pkg["render"], gt))
    t = rgr.terms(pkg["scales"], pkg["opacity"])
    return loss + opt.shape_pena * t[0] + opt.scale_pena * t[1] + opt.opa_pena * t[2]


def margin_of(ref, opt):
    """tests/dng_densify_reference.smallest_margin on the restatement's state (what the next densification decides on)"""
    class _M:
        pass
    m = _M()
    m.params, m.xyz_gradient_accum, m.denom, m.P, m.percent_dense = ref.p, ref.xyz_gradient_accum, ref.denom, ref.P, ref.percent_dense
    return ddr.smallest_margin(m, 2, opt.split_opacity_thresh, opt.min_opacity, opt.densify_grad_threshold, opt.cameras_extent,
                               constructed=False)


def run(oracle, scene, cams, gts, depth_mono, opt, n_iters, dtype=torch.float32, near_centers=None, near_range=0.0, bg=None,
        after_backward=None, neural_seed=0):
    """iterations 1 .. n_iters.  opt: gsplat_amd.trainer.DngOptions.  near_range: a number (the script's --near), or a callable
    iteration -> number.  after_backward(leg, iteration, ref, neural): behind each
    backward (the gradients are there, nothing has been stepped).
    -> dict(trace, P_after_densify, margins, statistic (g of every row before each densification), model, neural, steps,
    neural_steps)"""
    bg = torch.zeros(3) if bg is None else bg
    ref = make_model(scene, dtype)
    neural = stand_in_for(scene, dtype, neural_seed)
    nopt = torch.optim.Adam(neural.get_params(opt.neural_grid, opt.neural_net), lr=0.0, eps=1e-15)
    mono = [(255.0 - d.to(dtype)).reshape(1, 1, *d.shape) for d in depth_mono]
    rng = random.Random(opt.seed)
    viewpoint_stack = None
    trace, P_after, margins, statistic = [], [], [], []

    def step_and_zero():
        ref.optimizer.step()
        nopt.step()
        ref.optimizer.zero_grad(set_to_none=True)
        nopt.zero_grad(set_to_none=True)

    with _default_dtype(dtype):
        for iteration in range(1, n_iters + 1):
            xyz_lr = expon_lr(max(iteration - opt.position_lr_start, 0), LR["xyz"], opt.position_lr_final,
                              lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
            for g in ref.optimizer.param_groups:
                if g["name"] == "xyz":
                    g["lr"] = xyz_lr
            if not viewpoint_stack:
                viewpoint_stack = list(range(len(cams)))
            ci = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
            cam, gt = cams[ci], gts[ci].to(dtype)
            ev = dict(camera=ci, patches=[None] * 4, xyz_lr=xyz_lr, stepped=dict(hard=False, soft=False, gaussians=False, neural=False),
                      densified=False, near_pruned=False, cleaned=False)
            before = steps_of(ref)
            nbefore = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            # ---- hard depth
            if iteration > opt.hard_depth_start:
                depth = render_for_depth(oracle, cam, ref, bg, dtype)
                ev["patches"][0] = rng.randint(*opt.patch_range)
                ev["patches"][1] = rng.randint(*opt.patch_range)
                loss_hard = depth_loss(depth, mono[ci], ev["patches"][0], ev["patches"][1], opt, iteration)
                loss_hard.backward()
                if after_backward is not None:
                    after_backward("hard", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
            # ---- soft depth
            if iteration > opt.soft_depth_start:
                depth = render_for_opa(oracle, cam, ref, bg, dtype)
                ev["patches"][2] = rng.randint(*opt.patch_range)
                ev["patches"][3] = rng.randint(*opt.patch_range)
                loss_pnt = depth_loss(depth, mono[ci], ev["patches"][2], ev["patches"][3], opt, iteration)
                loss_pnt.backward()
                if after_backward is not None:
                    after_backward("soft", iteration, ref, neural)
                if iteration < opt.iterations:
                    step_and_zero()
            after_legs = steps_of(ref)
            # ---- photometric
            pkg = render(oracle, cam, ref, neural, bg, dtype)
            loss = photometric_loss(pkg, gt, opt)
            loss.backward()
            if after_backward is not None:
                after_backward("photometric", iteration, ref, neural)
            with torch.no_grad():
                vf, radii, vs = pkg["visibility_filter"], pkg["radii"], pkg["viewspace_points"]
                if iteration in opt.clean_iterations:   # clean_views: one render per training camera
                    visible = None
                    for c in cams:
                        f = render(oracle, c, ref, neural, bg, dtype)["visibility_filter"]
                        visible = f if visible is None else visible | f
                    ref.prune_points(~visible)
                    ev["cleaned"] = True
                if iteration < opt.densify_until_iter and iteration not in opt.clean_iterations:
                    ref.max_radii2D[vf] = torch.max(ref.max_radii2D[vf], radii[vf].to(dtype))
                    ref.xyz_gradient_accum[vf] += torch.norm(vs.grad[vf, :2], dim=-1, keepdim=True).to(dtype)
                    ref.denom[vf] += 1
                    if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                        margins.append(margin_of(ref, opt))
                        g = ref.xyz_gradient_accum / ref.denom
                        statistic.append(torch.where(g.isnan(), torch.zeros_like(g), g).reshape(-1).double().clone())
                        gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
                        ref.densify_and_prune(opt.densify_grad_threshold, opt.min_opacity, opt.cameras_extent, None,
                                              opt.split_opacity_thresh, None, generator=gen)
                        ev["densified"] = True
                        P_after.append(ref.P)
                if (iteration - 1) % opt.near_prune_interval == 0 and iteration > opt.near_prune_start:
                    mask_near = None
                    near = near_range(iteration) if callable(near_range) else near_range
                    for c in near_centers:
                        mask_temp = (ref.p["xyz"] - c.to(dtype).repeat(ref.P, 1)).norm(dim=1, keepdim=True) < near
                        mask_near = mask_near + mask_temp if mask_near is not None else mask_temp
                    ref.prune_points(mask_near.squeeze(1))
                    ev["near_pruned"] = True
                if iteration < opt.iterations:
                    step_and_zero()
            # which steps happened, read off torch's own per-parameter counters
            now = steps_of(ref)
            nnow = [int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()]
            ev["stepped"] = dict(hard=after_legs["xyz"] > before["xyz"], soft=after_legs["opacity"] > before["opacity"],
                                 gaussians=now["scaling"] > before["scaling"], neural=nnow[0] > nbefore[0])
            ev["patches"] = tuple(ev["patches"])
            ev["P"] = ref.P
            ev["loss"] = float(loss.detach())
            trace.append(ev)
    return dict(trace=trace, P_after_densify=P_after, margins=margins, statistic=statistic, model=ref, neural=neural,
                steps=steps_of(ref), neural_steps=[int(nopt.state[p]["step"]) if p in nopt.state else 0 for p in neural.parameters()])
