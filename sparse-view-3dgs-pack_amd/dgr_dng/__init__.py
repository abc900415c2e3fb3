"""Drop-in for `dgr_dng`, DNGaussian's rasterizer package (DNGaussian/gaussian_renderer/__init__.py:14;
DNGaussian/submodules/diff-gaussian-rasterization/dgr_dng/__init__.py).  Its CUDA sources are byte-identical to the
FSGS fork's (depth + alpha outputs and their gradients); the Python wrapper has no `confidence` field and does not
rescale gradients.  Served by the same entry points as `dgr_fsgs` (gs_forward_render_fsgs / gs_backward_fsgs)."""
from typing import NamedTuple

import torch
import torch.nn as nn

import dgr_fsgs
from dgr_fsgs import _C  # noqa: F401


class _RasterizeGaussians(dgr_fsgs._RasterizeGaussians):
    @classmethod
    def backward(cls, ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        rs = ctx.raster_settings
        ctx.raster_settings = _WithConfidence(rs)
        try:
            return super().backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha)
        finally:
            ctx.raster_settings = rs


class _WithConfidence:
    """View of the 12-field settings with the neutral confidence the shared backward multiplies by."""

    def __init__(self, rs):
        self._rs = rs
        self.confidence = torch.ones((1, 1), device=rs.bg.device)

    def __getattr__(self, name):
        return getattr(self._rs, name)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizer(dgr_fsgs.GaussianRasterizer):
    _fn = _RasterizeGaussians


# ---- DNGaussian's two depth passes, served by the depth-only kernels (gsplat_amd.depth_pass) ------------------------------
def _depth_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier):
    import math
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=pipe.debug)


def _depth_shape(pc, pipe, scaling_modifier):
    """-> (scales, rotations, cov3D_precomp), detached.  (The reference's render_for_opa leaves a Python-side covariance
    attached; this pass produces no gradient for it.)"""
    if pipe.compute_cov3D_python:
        return None, None, pc.get_covariance(scaling_modifier).detach()
    return pc.get_scaling.detach(), pc.get_rotation.detach(), None


def render_for_depth(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, value=0.95):
    """DNGaussian's "hard depth" pass (gaussian_renderer/__init__.py:128-197): every opacity is `value`, the loss reaches the
    means only.  Same arguments and returned keys as the reference's function, except that there is no "render" (a colour
    image of ones that neither training script reads)."""
    from gsplat_amd.depth_pass import depth_pass
    xyz = pc.get_xyz
    screenspace_points = torch.zeros_like(xyz, requires_grad=True)
    scales, rotations, cov = _depth_shape(pc, pipe, scaling_modifier)
    depth, alpha, radii = depth_pass(_depth_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier), xyz, float(value),
                                     scales, rotations, cov, grad="means", means2D=screenspace_points)
    return {"depth": depth, "alpha": alpha, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii}


def render_for_opa(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0):
    """DNGaussian's "soft depth" pass (gaussian_renderer/__init__.py:201-269): the model's opacities, the loss reaches them
    only.  Same arguments and returned keys as the reference's function, without "render"; `viewspace_points` receives no
    gradient in this pass (the means are detached there too)."""
    from gsplat_amd.depth_pass import depth_pass
    xyz = pc.get_xyz
    screenspace_points = torch.zeros_like(xyz, requires_grad=True)
    opacity = pc.get_opacity
    scales, rotations, cov = _depth_shape(pc, pipe, scaling_modifier)
    depth, alpha, radii = depth_pass(_depth_settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier), xyz.detach(),
                                     opacity, scales, rotations, cov, grad="opacity")
    return {"depth": depth, "alpha": alpha, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
            "radii": radii, "opacity": opacity}
