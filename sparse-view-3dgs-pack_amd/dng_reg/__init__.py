"""Per-Gaussian pieces of a DNGaussian training step on the MI355X kernels (csrc/gs_dng_reg.hip through
gsplat_amd/dng_reg.py, csrc/gs_dng_dtu.hip through gsplat_amd/dng_dtu.py, csrc/gs_dng_blender.hip through
gsplat_amd/dng_blender.py).  No CPU fallback.

  gaussian_regulariser(scaling, opacity, ...)        train_llff.py:159-165 (train_dtu.py:176-182, train_blender.py:161-167): the
                                                     shape / scale / opacity penalty on get_scaling and the opacity column
  gaussian_regulariser_raw(_scaling, _opacity, ...)  the same on the raw rows, exp and sigmoid inside the kernels
  view_dirs(xyz, campos)                             gaussian_renderer/__init__.py:22-23: the unit directions the SH encoder takes
  near_camera_mask(xyz, centers, near)               train_llff.py:209-213, render.py:113, spiral.py:106: one launch for all cameras
  colour_rule(colour, stat, opacity_raw, ...)        train_dtu.py:218-230: the black / white edits of xyz_gradient_accum and the raw
                                                     opacity in front of a densification, in place, one launch
  white_rule(colour, stat, opacity_raw, thr, factor) train_blender.py:207-211: statistic zeroed, raw opacity to
                                                     inverse_sigmoid(factor sigmoid(opacity)) where the colour is white
  white_rule_sh(xyz, shs, degree, campos, ...)       train_blender.py:366-370: the same on the colour of the SH rows, evaluated
                                                     inside the kernel as render_sh does

Divergences: fp32 and CUDA(HIP) tensors only; the sums are float64 in a fixed order (the same bits on every run); no host
synchronisation (the reference's two boolean-index gathers block the host).  As in the reference, an empty opacity set gives
a NaN loss, and a Gaussian at the camera centre a NaN direction."""
from gsplat_amd import dng_reg as _k
from gsplat_amd.dng_blender import white_rule, white_rule_sh  # noqa: F401
from gsplat_amd.dng_dtu import colour_rule, reset_value  # noqa: F401
from gsplat_amd.dng_reg import near_camera_mask, view_dirs  # noqa: F401

__all__ = ["gaussian_regulariser", "gaussian_regulariser_raw", "view_dirs", "near_camera_mask"]
# (colour_rule, reset_value, white_rule and white_rule_sh are importable by name)


def gaussian_regulariser(scaling, opacity, shape_pena=0.001, scale_pena=0.001, opa_pena=0.01, return_terms=False):
    return _k.gaussian_regulariser(scaling, opacity, shape_pena, scale_pena, opa_pena, return_terms)


def gaussian_regulariser_raw(scaling, opacity, shape_pena=0.001, scale_pena=0.001, opa_pena=0.01, return_terms=False):
    return _k.gaussian_regulariser_raw(scaling, opacity, shape_pena, scale_pena, opa_pena, return_terms)
