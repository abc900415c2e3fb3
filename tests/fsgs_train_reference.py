"""FSGS/train.py:81-176 restated literally, in the reference's order - the yardstick of tests/test_fsgs_trainer_cpu.py and
tests/test_gpu_fsgs_step.py.

  * the model is the reference's six leaf tensors (_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation) under
    torch.optim.Adam(lr=0, eps=1e-15) with its six groups (scene/gaussian_model.py:165-181);
  * a view is rendered through the checker's FSGS rasterizer (oracle.FsgsRasterizer, float32), un-clamped, confidence = ones;
  * L1 and SSIM are plain torch (utils/loss_utils.py), the Pearson terms those of tests/fsgs_loss_reference.py, the
    densification that of tests/fsgs_densify_reference.py (cat_tensors_to_optimizer / _prune_optimizer keep a tensor's Adam
    step count; so does reset_opacity's replace_tensor_to_optimizer);
  * `dtype`: float32, or the float64 TWIN - the same loop with the loss and the optimizer arithmetic (parameters, moments,
    statistics, densification) in float64; the rasterizer stays the float32 checker, fed the rounded parameters.

`run` returns what the tests compare: the event trace, P after every densification, the decision margins of every
densification, the gradients of the first iteration and the final parameters."""
import contextlib
import random
from math import exp

import torch
import torch.nn.functional as F

import fsgs_densify_reference as fdr
import fsgs_loss_reference as flr
from gsplat_amd.knn import dist2_with_indices
from gsplat_amd.trainer import expon_lr

LR = dict(xyz=0.00016, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, scaling=0.005, rotation=0.001)  # arguments/__init__.py:77-84
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


# ---- utils/loss_utils.py ------------------------------------------------------------------------------------------------
def l1_loss(a, b):
    return torch.abs(a - b).mean()


def _window(channels, dtype, size=11, sigma=1.5):
    g = torch.Tensor([exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)])
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
    return w.expand(channels, 1, size, size).contiguous().to(dtype)


def ssim(img1, img2):
    ch = img1.size(-3)
    w = _window(ch, img1.dtype)
    a, b = img1.unsqueeze(0), img2.unsqueeze(0)
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=ch), F.conv2d(b, w, padding=5, groups=ch)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(a * a, w, padding=5, groups=ch) - mu1_sq
    s2 = F.conv2d(b * b, w, padding=5, groups=ch) - mu2_sq
    s12 = F.conv2d(a * b, w, padding=5, groups=ch) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))).mean()


def train_loss(image, depth, gt, midas, depth_weight, lambda_dssim=0.2):
    """train.py:94-109 -> (loss, branch of the min)"""
    loss = (1.0 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1.0 - ssim(image, gt))
    depth_loss, branch = flr.depth_pearson_loss(depth.reshape(-1, 1), midas.reshape(-1, 1), return_branch=True)
    return loss + depth_weight * depth_loss, branch


# ---- the model ----------------------------------------------------------------------------------------------------------
def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


class Model:
    def __init__(self, scene, dtype, spatial_lr_scale=1.0):
        """scene: activated tensors as gsplat_amd.synthetic makes them (GaussianModelLite's input)"""
        self.dtype = dtype
        f = scene["shs"].float()
        raw = dict(xyz=scene["means3D"].float(), f_dc=f[:, :1, :], f_rest=f[:, 1:, :],
                   opacity=inverse_sigmoid(scene["opacities"].float()).reshape(-1, 1), scaling=torch.log(scene["scales"].float()),
                   rotation=scene["rotations"].float())
        self.spatial_lr_scale = spatial_lr_scale
        self.active_sh_degree, self.max_sh_degree = 0, 3
        self._install({k: v.to(dtype) for k, v in raw.items()}, None, None, {k: 0 for k in GROUPS})
        self.reset_stats()

    @property
    def P(self):
        return self.p["xyz"].shape[0]

    def reset_stats(self):
        self.xyz_gradient_accum = torch.zeros((self.P, 1), dtype=self.dtype)
        self.denom = torch.zeros((self.P, 1), dtype=self.dtype)
        self.max_radii2D = torch.zeros((self.P,), dtype=self.dtype)

    def _install(self, raw, exp_avg, exp_avg_sq, steps, xyz_lr=None):
        """new leaf tensors and a new Adam over them, carrying moments and step counts (what cat_tensors_to_optimizer,
        _prune_optimizer and replace_tensor_to_optimizer do to the optimizer's state)"""
        self.p = {k: raw[k].detach().clone().contiguous().requires_grad_(True) for k in GROUPS}
        lrs = dict(LR)
        lrs["xyz"] = LR["xyz"] * self.spatial_lr_scale if xyz_lr is None else xyz_lr
        self.opt = torch.optim.Adam([{"params": [self.p[k]], "lr": lrs[k], "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
        for k in GROUPS:
            if steps[k] > 0:
                self.opt.state[self.p[k]] = {"step": torch.tensor(float(steps[k])), "exp_avg": exp_avg[k].detach().clone(),
                                             "exp_avg_sq": exp_avg_sq[k].detach().clone()}

    def steps(self):
        return {k: int(self.opt.state[self.p[k]]["step"]) if self.p[k] in self.opt.state else 0 for k in GROUPS}

    def moments(self, which):
        return {k: (self.opt.state[self.p[k]][which] if self.p[k] in self.opt.state else torch.zeros_like(self.p[k])) for k in GROUPS}

    def xyz_lr(self):
        return next(g["lr"] for g in self.opt.param_groups if g["name"] == "xyz")

    # -- the five-field rows of tests/fsgs_densify_reference.py <-> the six tensors
    @staticmethod
    def _to_rows(d):
        n = d["xyz"].shape[0]
        return dict(xyz=d["xyz"], features=torch.cat((d["f_dc"], d["f_rest"]), dim=1).reshape(n, 48), opacity=d["opacity"],
                    scaling=d["scaling"], rotation=d["rotation"])

    @staticmethod
    def _from_rows(r):
        n = r["xyz"].shape[0]
        f = r["features"].reshape(n, 16, 3)
        return dict(xyz=r["xyz"], f_dc=f[:, :1, :], f_rest=f[:, 1:, :], opacity=r["opacity"], scaling=r["scaling"],
                    rotation=r["rotation"])

    def flat(self):
        """the parameters in GaussianModelLite's flat order (xyz | features | opacity | scaling | rotation)"""
        r = self._to_rows({k: v.detach() for k, v in self.p.items()})
        return torch.cat([r[k].reshape(-1) for k in ("xyz", "features", "opacity", "scaling", "rotation")])

    def grads(self):
        """the gradients under the names tests/helpers.check_grads compares"""
        g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in self.p.items()}
        return dict(xyz=g["xyz"], features=torch.cat((g["f_dc"], g["f_rest"]), dim=1), opacity=g["opacity"], scaling=g["scaling"],
                    rotation=g["rotation"])

    def update_learning_rate(self, iteration, opt):
        lr = expon_lr(iteration, LR["xyz"] * self.spatial_lr_scale, opt.position_lr_final * self.spatial_lr_scale,
                      lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
        for g in self.opt.param_groups:
            if g["name"] == "xyz":
                g["lr"] = lr

    def reset_opacity(self):
        """scene/gaussian_model.py:230-234: opacity <- min(opacity, 0.05); replace_tensor_to_optimizer zeroes its moments"""
        new = inverse_sigmoid(torch.min(torch.sigmoid(self.p["opacity"].detach()), torch.ones_like(self.p["opacity"]) * 0.05))
        raw = {k: v.detach() for k, v in self.p.items()}
        raw["opacity"] = new
        ea, eas = self.moments("exp_avg"), self.moments("exp_avg_sq")
        ea["opacity"], eas["opacity"] = torch.zeros_like(new), torch.zeros_like(new)
        self._install(raw, ea, eas, self.steps(), self.xyz_lr())

    def densify_and_prune(self, knn, opt, iteration, generator):
        state = tuple(self._to_rows({k: v.detach().reshape(self.P, -1) if k not in ("f_dc", "f_rest") else v.detach()
                                     for k, v in d.items()}) for d in (self.p, self.moments("exp_avg"), self.moments("exp_avg_sq")))
        accum, denom = self.xyz_gradient_accum.clone(), self.denom.clone()
        with _default_dtype(self.dtype):   # (the restatement's torch.zeros(...) scratch tensors follow the run's precision)
            state, counts, info = fdr.densify_and_prune(state, accum, denom, lambda x: knn(x.float()), opt.densify_grad_threshold,
                                                        opt.min_opacity, opt.cameras_extent, None, iteration, generator,
                                                        dist_thres=opt.dist_thres, prune_from_iter=opt.prune_from_iter,
                                                        proximity_until_iter=opt.proximity_until_iter)
        margin = fdr.smallest_margin(info, accum, denom, 2, None, extent=opt.cameras_extent, dist_thres=opt.dist_thres,
                                     max_grad=opt.densify_grad_threshold, min_opacity=opt.min_opacity, constructed=False)
        p, ea, eas = (self._from_rows(part) for part in state)
        self._install({k: v.to(self.dtype) for k, v in p.items()}, ea, eas, self.steps(), self.xyz_lr())
        self.reset_stats()
        return counts, margin


@contextlib.contextmanager
def _default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def render(oracle, cam, model, bg):
    """gaussian_renderer/__init__.py:20-132 on the checker's FSGS rasterizer (float32), un-clamped"""
    import math
    p = model.p
    xyz = p["xyz"].float()
    screenspace_points = torch.zeros_like(xyz, requires_grad=True) + 0
    screenspace_points.retain_grad()
    rs = oracle.FsgsSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=model.active_sh_degree, campos=cam.camera_center, prefiltered=False,
        debug=False, confidence=torch.ones((model.P, 1)))
    image, radii, depth, alpha = oracle.FsgsRasterizer(raster_settings=rs)(
        means3D=xyz, means2D=screenspace_points, shs=torch.cat((p["f_dc"], p["f_rest"]), dim=1).float(), colors_precomp=None,
        opacities=torch.sigmoid(p["opacity"]).float(), scales=torch.exp(p["scaling"]).float(),
        rotations=F.normalize(p["rotation"]).float(), cov3D_precomp=None)
    return {"render": image.to(model.dtype), "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii,
            "depth": depth.to(model.dtype)}


def run(oracle, scene, cams, gts, midas, opt, n_iters, dtype=torch.float32, pseudo_cams=None, depth_estimator=None, bg=None,
        after_backward=None):
    """iterations 1 .. n_iters of FSGS/train.py:81-176.  opt: gsplat_amd.trainer.FsgsOptions (the reference's args / opt).
    after_backward(iteration, model): called behind loss.backward() (the gradients are there, nothing has been stepped).
    -> dict(trace, P_after_densify, margins, model)"""
    bg = torch.zeros(3) if bg is None else bg
    knn = lambda xyz: dist2_with_indices(oracle.api, xyz)   # noqa: E731
    gaussians = Model(scene, dtype)
    rng = random.Random(opt.seed)
    viewpoint_stack, pseudo_stack = None, None
    depth_weight = opt.depth_weight
    trace, P_after, margins = [], [], []
    for iteration in range(1, n_iters + 1):
        if iteration % opt.sh_increase_interval == 0:
            if gaussians.active_sh_degree < gaussians.max_sh_degree:
                gaussians.active_sh_degree += 1
        if not viewpoint_stack:
            viewpoint_stack = list(range(len(cams)))
        ci = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
        render_pkg = render(oracle, cams[ci], gaussians, bg)
        image, viewspace_point_tensor, visibility_filter, radii = (render_pkg["render"], render_pkg["viewspace_points"],
                                                                   render_pkg["visibility_filter"], render_pkg["radii"])
        ev = dict(camera=ci, sh_degree=gaussians.active_sh_degree, xyz_lr=gaussians.xyz_lr(), depth_weight=depth_weight,
                  stepped=False, densified=False, reset=False, pseudo=False)
        loss, _ = train_loss(image, render_pkg["depth"][0], gts[ci].to(dtype), midas[ci].to(dtype), depth_weight)
        if iteration > opt.end_sample_pseudo:
            depth_weight = 0.001
        if (pseudo_cams and depth_estimator is not None and iteration % opt.sample_pseudo_interval == 0
                and iteration > opt.start_sample_pseudo and iteration < opt.end_sample_pseudo):
            if not pseudo_stack:
                pseudo_stack = list(range(len(pseudo_cams)))
            pseudo_cam = pseudo_cams[pseudo_stack.pop(rng.randint(0, len(pseudo_stack) - 1))]
            render_pkg_pseudo = render(oracle, pseudo_cam, gaussians, bg)
            rendered_depth_pseudo = render_pkg_pseudo["depth"][0].reshape(-1, 1)
            midas_depth_pseudo = depth_estimator(render_pkg_pseudo["render"]).reshape(-1, 1)
            depth_loss_pseudo = flr.pseudo_depth_pearson_loss(rendered_depth_pseudo, midas_depth_pseudo).mean()
            if torch.isnan(depth_loss_pseudo).sum() == 0:
                loss_scale = min((iteration - opt.start_sample_pseudo) / 500., 1)
                loss = loss + loss_scale * opt.depth_pseudo_weight * depth_loss_pseudo
                ev["pseudo"] = True
        loss.backward()
        if after_backward is not None:
            after_backward(iteration, gaussians)
        with torch.no_grad():
            densified_now = False
            if iteration < opt.densify_until_iter:
                vf = visibility_filter
                gaussians.max_radii2D[vf] = torch.max(gaussians.max_radii2D[vf], radii[vf].to(dtype))
                gaussians.xyz_gradient_accum[vf] += torch.norm(viewspace_point_tensor.grad[vf, :2], dim=-1, keepdim=True).to(dtype)
                gaussians.denom[vf] += 1
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    gen = torch.Generator().manual_seed(opt.seed * 1000003 + iteration)
                    counts, margin = gaussians.densify_and_prune(knn, opt, iteration, gen)
                    densified_now = True
                    ev["densified"] = True
                    P_after.append(gaussians.P)
                    margins.append(margin)
            if iteration < opt.iterations:
                # (the tensors a densification replaced have no gradient: optimizer.step() leaves them, their moments and
                #  their step counts alone - every group, since every tensor was replaced)
                if not densified_now:
                    gaussians.opt.step()
                    ev["stepped"] = True
                gaussians.opt.zero_grad(set_to_none=True)
            gaussians.update_learning_rate(iteration, opt)
            if (iteration - opt.start_sample_pseudo - 1) % opt.opacity_reset_interval == 0 and iteration > opt.start_sample_pseudo:
                gaussians.reset_opacity()
                ev["reset"] = True
        ev["loss"] = float(loss.detach())
        trace.append(ev)
    return dict(trace=trace, P_after_densify=P_after, margins=margins, model=gaussians)
