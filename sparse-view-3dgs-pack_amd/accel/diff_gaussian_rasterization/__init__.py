"""Opt-in: `diff_gaussian_rasterization` WITH the reference's accelerated path.  Put this
directory's parent, sparse-view-3dgs-pack_amd/accel, IN FRONT OF sparse-view-3dgs-pack_amd on PYTHONPATH: LGDWT-GS/train.py:42-46
then finds `SparseGaussianAdam`, builds it for optimizer_type="sparse_adam", steps it with `step(radii > 0, N)` and renders
with `rasterizer(dc=..., shs=...)`.  Everything the default package exports, with the rasterizer classes of gsplat_amd.accel."""
from gsplat_amd.accel import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                              _RasterizeGaussians, rasterize_gaussians)
from . import _C  # noqa: F401
from gsplat_amd.optim import SparseGaussianAdam  # noqa: F401
