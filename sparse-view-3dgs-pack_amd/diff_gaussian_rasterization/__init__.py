"""Drop-in for the reference's `diff_gaussian_rasterization` / `dgr_3dgs` Python package
(diff-gaussian-rasterization/dgr_3dgs/__init__.py, API of the `dr_aa` branch: antialiasing flag,
inverse-depth output), backed by the MI355X HIP rasterizer.

Public surface (same names, argument order, defaults, return values and error behaviour):
  GaussianRasterizationSettings   NamedTuple, 13 fields        dgr_3dgs/__init__.py:143-156
  GaussianRasterizer(nn.Module)   forward / markVisible         dgr_3dgs/__init__.py:158-207
  rasterize_gaussians, _RasterizeGaussians                      dgr_3dgs/__init__.py:21-141
`SparseGaussianAdam` is absent from THIS package on purpose: LGDWT-GS/train.py:42-46 probes for it and, finding it,
switches the optimizer and the renderer (`rasterizer(dc=..., shs=...)`) by itself - a maintainer opts into that.  The
opt-in is one more PYTHONPATH entry: sparse-view-3dgs-pack_amd/accel in front of this directory's parent puts a package
of the same name first that exports everything below, the class, and a GaussianRasterizer whose forward() takes `dc=`
(gsplat_amd.accel, gsplat_amd.optim).
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    # `_C` is looked up through this attribute so that the test-suite can run the identical
    # autograd plumbing against another implementation of the same C ABI (it swaps it on a subclass).
    _impl = _C

    @classmethod
    def forward(cls, ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        rs = raster_settings
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
                rs.sh_degree, rs.campos, rs.prefiltered, rs.antialiasing, rs.debug)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, invdepths = \
            cls._impl.rasterize_gaussians(*args)
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities,
                              geomBuffer, binningBuffer, imgBuffer)
        ctx.mark_non_differentiable(radii)
        # The reference lets autograd materialise a zero gradient for an unused inverse-depth output, which keeps its
        # depth branch alive in every backward (rasterize_points.cu:176-182).  A zero image gradient
        # contributes exactly nothing, so here an unused output arrives as None and the backward kernel without
        # that channel runs - same numbers, less work.
        ctx.set_materialize_grads(False)
        return color, radii, invdepths

    @classmethod
    def backward(cls, ctx, grad_out_color, _, grad_out_depth):
        num_rendered = ctx.num_rendered
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, opacities, geomBuffer,
         binningBuffer, imgBuffer) = ctx.saved_tensors
        if grad_out_color is None:  # only the inverse depth was used
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        args = (rs.bg, means3D, radii, colors_precomp, opacities, scales, rotations, rs.scale_modifier,
                cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color,
                grad_out_depth, sh, rs.sh_degree, rs.campos, geomBuffer, num_rendered, binningBuffer, imgBuffer,
                rs.antialiasing, rs.debug)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
         grad_scales, grad_rotations) = cls._impl.rasterize_gaussians_backward(*args)
        return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp, None)


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
    antialiasing: bool


class GaussianRasterizer(nn.Module):
    _fn = _RasterizeGaussians
    # Optional, not part of the reference's API: a stable identity of the camera this rasterizer renders (any hashable -
    # an index, an image name).  The backend keeps per-camera scheduling state between visits (tile order, verified depth
    # limits: INTEGRATION.md section 4) and tells cameras apart by this key; without one it falls back to a hash of the view
    # matrix's contents (one small device-to-host copy per NEW tensor object).
    camera_key = None
    # With a camera_key the backend may also render this camera's LATER visits from depth-limited instance lists (exact: the
    # forward verifies every cut list and renders the view again when one proved too short - INTEGRATION.md section 4).
    # False: the key only names the camera (tile-order hint); gsplat_amd.trainer manages the limits itself.
    camera_limits = True

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            visible = self._fn._impl.mark_visible(positions, rs.viewmatrix, rs.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        raster_settings = self.raster_settings

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        if shs is None:
            shs = torch.Tensor([])
        if colors_precomp is None:
            colors_precomp = torch.Tensor([])
        if scales is None:
            scales = torch.Tensor([])
        if rotations is None:
            rotations = torch.Tensor([])
        if cov3D_precomp is None:
            cov3D_precomp = torch.Tensor([])

        if self.camera_key is not None:
            backend = getattr(self._fn._impl, "backend", None)
            if backend is not None:
                backend.camera_key = self.camera_key   # one-shot: consumed by the forward below
                backend.camera_key_limits = bool(self.camera_limits)
        return self._fn.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                              raster_settings)
