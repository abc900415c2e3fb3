"""`diff_gaussian_rasterization._C` of the opt-in package: the default package's stand-in for the compiled extension."""
from gsplat_amd.accel import _C as _default

backend = _default.backend
rasterize_gaussians = _default.rasterize_gaussians
rasterize_gaussians_backward = _default.rasterize_gaussians_backward
mark_visible = _default.mark_visible
