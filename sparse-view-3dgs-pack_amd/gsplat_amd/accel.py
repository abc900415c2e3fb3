"""The rasterizer call of the reference's accelerated path: `rasterizer(dc=pc.get_features_dc, shs=pc.get_features_rest, ...)`
(LGDWT-GS/gaussian_renderer/__init__.py:82-100, taken when train.py:42-46 finds `SparseGaussianAdam`), served from the model's
two SH tensors where they are - no `torch.cat` of 192 B per Gaussian forward, no copy of a strided gradient slice backward.

  GaussianRasterizer    the default package's class with one more keyword, `dc`, appended LAST to forward()
  _RasterizeGaussians   autograd function over (means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings)
  rasterize_gaussians   the same, as a function

With dc [P,1,3], shs [P,K,3] (1 <= K <= 15), scales and rotations given and an implementation that has gs_backward_split, the
forward hands the kernels `dc` as the DC rows and `shs` as GsGaussians.shs_rest, and the backward writes one contiguous gradient
per tensor (gs_backward_split).  K == 0 (a degree-0 model): `dc` alone is the SH tensor.  Every other case - a precomputed 3D
covariance, an implementation bound to another library of the C ABI that lacks the entry point - concatenates and makes the
ordinary call; autograd splits the gradient: the same numbers, only slower.

Exported by the opt-in packages under sparse-view-3dgs-pack_amd/accel; the default packages do not
change.  The FSGS / DNGaussian rasterizer generations have no `dc=` in the reference and get none here."""
import importlib.util
import os
import sys

import torch

_BASE_INIT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff_gaussian_rasterization",
                          "__init__.py")


def _base_package():
    """The DEFAULT drop-in package, whatever `diff_gaussian_rasterization` resolves to on sys.path (with the opt-in directory
    in front it is the package that imports this module)."""
    spec = importlib.util.find_spec("diff_gaussian_rasterization") if "diff_gaussian_rasterization" not in sys.modules else None
    if spec is not None and spec.origin and os.path.abspath(spec.origin) == _BASE_INIT:
        import diff_gaussian_rasterization
        return diff_gaussian_rasterization
    mod = sys.modules.get("diff_gaussian_rasterization")
    if mod is not None and os.path.abspath(getattr(mod, "__file__", None) or "") == _BASE_INIT:
        return mod
    name = "gsplat_amd._dgr_default"
    mod = sys.modules.get(name)
    if mod is None:
        spec = importlib.util.spec_from_file_location(name, _BASE_INIT, submodule_search_locations=[os.path.dirname(_BASE_INIT)])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        try:
            spec.loader.exec_module(mod)
        except BaseException:
            del sys.modules[name]
            raise
    return mod


_base = _base_package()
GaussianRasterizationSettings = _base.GaussianRasterizationSettings
_C = _base._C


def _none_if_empty(t):
    return None if t is None or (t.dim() == 1 and t.numel() == 0) else t


def rasterize_gaussians(means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    """The default package's autograd function with `dc` in front of `sh`.  dc empty: that function exactly (sh holds every
    coefficient).  dc given: sh holds coefficients 1..K and the implementation's backend serves the split rows."""
    _impl = _C   # (looked up through this attribute: the test-suite swaps it on a subclass, as on the default package)

    @classmethod
    def split_backend(cls):
        """The implementation's backend if it serves split SH rows (forward AND gs_backward_split), else None."""
        backend = getattr(cls._impl, "backend", None)
        if backend is None or "backward_split" in getattr(backend.api, "missing", ()):
            return None
        return backend

    @classmethod
    def forward(cls, ctx, means3D, means2D, dc, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        rs = raster_settings
        split = _none_if_empty(dc) is not None
        args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, dc if split else sh,
                rs.sh_degree, rs.campos, rs.prefiltered, rs.antialiasing, rs.debug)
        if split:
            backend = cls.split_backend()
            if backend is None:
                raise RuntimeError("this implementation does not serve split SH rows (GaussianRasterizer.forward concatenates)")
            backend.sh_rest, backend.sh_rest_activated = sh, True   # one-shot: taken by the forward below
            try:
                out = cls._impl.rasterize_gaussians(*args)
            finally:
                backend.sh_rest, backend.sh_rest_activated = None, False
        else:
            out = cls._impl.rasterize_gaussians(*args)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, invdepths = out
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.split = split
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, dc, sh, opacities,
                              geomBuffer, binningBuffer, imgBuffer)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)   # (an unused inverse-depth output arrives as None: see the default package)
        return color, radii, invdepths

    @classmethod
    def backward(cls, ctx, grad_out_color, _, grad_out_depth):
        rs = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, dc, sh, opacities, geomBuffer,
         binningBuffer, imgBuffer) = ctx.saved_tensors
        if grad_out_color is None:  # only the inverse depth was used
            grad_out_color = torch.zeros((3, rs.image_height, rs.image_width), dtype=torch.float32, device=means3D.device)
        args = (rs.bg, means3D, radii, colors_precomp, opacities, scales, rotations, rs.scale_modifier,
                cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color,
                grad_out_depth, dc if ctx.split else sh, rs.sh_degree, rs.campos, geomBuffer, ctx.num_rendered, binningBuffer,
                imgBuffer, rs.antialiasing, rs.debug)
        grad_dc = None
        if ctx.split:
            backend = cls.split_backend()
            backend.sh_rest, backend.sh_rest_activated = sh, True   # one-shot: taken by the backward below (gs_backward_split)
            try:
                (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_dc,
                 grad_scales, grad_rotations, grad_sh) = cls._impl.rasterize_gaussians_backward(*args)
            finally:
                backend.sh_rest, backend.sh_rest_activated = None, False
        else:
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = cls._impl.rasterize_gaussians_backward(*args)
        return (grad_means3D, grad_means2D, grad_dc, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp, None)


class GaussianRasterizer(_base.GaussianRasterizer):
    _fn = _RasterizeGaussians

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, dc=None):
        raster_settings = self.raster_settings

        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None) or \
                (dc is not None and shs is None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')

        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')

        if dc is not None:
            if dc.dim() != 3 or shs.dim() != 3 or dc.shape[1] != 1 or dc.shape[0] != shs.shape[0]:
                raise Exception("dc must have dimensions (num_points, 1, 3) and shs (num_points, K, 3)")
            K = int(shs.shape[1])
            if K == 0:     # a degree-0 model: the DC rows are the whole SH tensor
                shs, dc = dc, None
            elif not (K <= 15 and cov3D_precomp is None and self._fn.split_backend() is not None):
                shs, dc = torch.cat((dc, shs), dim=1), None   # the ordinary call; autograd splits the gradient

        if shs is None:
            shs = torch.Tensor([])
        if dc is None:
            dc = torch.Tensor([])
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
        return self._fn.apply(means3D, means2D, dc, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                              raster_settings)
