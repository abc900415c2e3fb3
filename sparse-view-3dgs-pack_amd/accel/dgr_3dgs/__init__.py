"""Opt-in alias package (`dgr_<model>` convention): the same objects as the opt-in diff_gaussian_rasterization beside it."""
from diff_gaussian_rasterization import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                                         SparseGaussianAdam, _C, _RasterizeGaussians, rasterize_gaussians)
