"""The depth-only pass: depth = sum z_i alpha_i T_i and alpha = sum alpha_i T_i of a view, with gradients to the means
and / or the opacities only (gs_depth_forward / gs_depth_backward, csrc/gs_depth_pass.hip).

It is what DNGaussian's two depth passes read (DNGaussian/gaussian_renderer/__init__.py:128-269: `render_for_depth`, the
"hard depth" pass - opacity 0.95 everywhere, gradient to the means - and `render_for_opa`, the "soft depth" pass - gradient to
the opacities): constant colour 1, colour image never used, scales and rotations detached.  `dgr_dng.GaussianRasterizer` serves
them too, through the general kernels; this module is the opt-in, leaner form.  `dgr_dng.render_for_depth` /
`dgr_dng.render_for_opa` wrap it under the reference's names.

`depth_leg_step` is a whole depth leg of DNGaussian's loop - forward, loss, backward and the Adam step of the leg's one tensor
inside the backward's per-Gaussian kernel (gs_depth_backward_step) - without an autograd node for the pass.

Outputs are the general path's bit for bit.  Not served: a colour image, `confidence` (the FSGS settings tuple), depth-limited
lists, gradients to scales / rotations / a precomputed covariance.
"""
import torch

_GRADS = {None: 0, "means": 1, "opacity": 2, "both": 3}
_filled = {}


def _filled_opacity(device, P, value):
    """The [P,1] tensor of a constant opacity, kept per (device, P, value): the hard pass asks for the same one every step."""
    key = (str(device), int(P), float(value))
    t = _filled.get(key)
    if t is None:
        if len(_filled) > 16:
            _filled.clear()
        t = _filled[key] = torch.full((int(P), 1), float(value), dtype=torch.float32, device=device)
    return t


class _DepthPass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, opacities, means2D, settings, scales, rotations, cov3D_precomp, flags):
        from . import hip_backend
        rs = settings
        backend = hip_backend()
        depth, alpha, radii, rec = backend.depth_forward(
            means3D, opacities, scales, rotations, cov3D_precomp, rs.scale_modifier, rs.bg, rs.viewmatrix, rs.projmatrix,
            rs.campos, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.debug)
        ctx.rec, ctx.flags, ctx.backend = rec, flags, backend
        ctx.carrier = means2D is not None
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return depth, alpha, radii

    @staticmethod
    def backward(ctx, grad_depth, grad_alpha, _grad_radii):
        flags, rec = ctx.flags, ctx.rec
        none = (None,) * 8
        if rec is None or (grad_depth is None and grad_alpha is None):
            return none
        dm3, dm2, dop = ctx.backend.depth_backward(rec, grad_depth, grad_alpha, flags)
        return (dm3, dop, dm2 if ctx.carrier else None) + none[3:]


def depth_pass(settings, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None, grad="means", means2D=None):
    """-> (depth [1,H,W], alpha [1,H,W], radii [P] int32): one autograd node.

    settings       dgr_dng.GaussianRasterizationSettings (a tuple with a `confidence` field raises: this pass does not rescale
                   gradients)
    opacities      [P,1] tensor, or a Python float - the hard pass's 0.95 - which becomes a cached filled tensor and has no gradient
    scales, rotations | cov3D_precomp   exactly one of the two, as the reference demands; neither ever gets a gradient
    grad           "means" | "opacity" | "both" | None: the gradient family the backward produces - nothing else is computed
    means2D        optional [P,3] carrier that receives dL_dmeans2D (the reference's `viewspace_points`) when grad has the means
    """
    if hasattr(settings, "confidence"):
        raise ValueError("depth_pass takes dgr_dng.GaussianRasterizationSettings: it does not rescale gradients by `confidence`")
    if grad not in _GRADS:
        raise ValueError("grad must be 'means', 'opacity', 'both' or None, not %r" % (grad,))
    flags = _GRADS[grad]
    const = isinstance(opacities, (int, float))
    if const and flags & 2:
        raise ValueError("a constant opacity has no gradient: grad=%r needs an opacity tensor" % (grad,))
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    if means3D.device.type != "cuda" or (not const and opacities.device.type != "cuda"):
        raise RuntimeError("gsplat depth pass got a tensor on %s - the rasterizer has no fallback path" % (means3D.device,))
    if const:
        opacities = _filled_opacity(means3D.device, means3D.shape[0], opacities)
    scales, rotations, cov3D_precomp = (None if t is None else t.detach() for t in (scales, rotations, cov3D_precomp))
    if flags == 0:
        with torch.no_grad():
            return _DepthPass.apply(means3D, opacities, None, settings, scales, rotations, cov3D_precomp, 0)
    return _DepthPass.apply(means3D if flags & 1 else means3D.detach(), opacities if flags & 2 else opacities.detach(),
                            means2D if flags & 1 else None, settings, scales, rotations, cov3D_precomp, flags)


def depth_leg_step(settings, means3D, opacities, scales, rotations, grad, loss_fn, param, exp_avg, exp_avg_sq, lr, step,
                   betas=(0.9, 0.999), eps=1e-15, cov3D_precomp=None):
    """One DNGaussian depth leg as forward + loss + ONE fused backward-and-step (gs_depth_backward_step): the depth pass runs
    without an autograd node, loss_fn(depth [1,H,W], alpha [1,H,W]) -> scalar is differentiated on its own small graph for the
    two image cotangents, and the entry consumes them - the blend backward, then a per-Gaussian kernel that differentiates a
    row and applies torch.optim.Adam's update at (lr, step) to it.  No gradient tensor of the leg's parameter exists.

    grad "means":   param / exp_avg / exp_avg_sq [P,3]; param is the tensor the pass reads as means3D (stepped in place).
    grad "opacity": param / moments [P,1] are the RAW opacity row and `opacities` its sigmoid, as the pass reads it.
    The result equals depth_pass(...) -> loss.backward() -> [sigmoid backward] -> gs_adam_step on that one tensor bit for bit.
    -> (loss (detached), radii)"""
    from . import hip_backend
    if grad not in ("means", "opacity"):
        raise ValueError("depth_leg_step steps one tensor: grad is 'means' or 'opacity', not %r" % (grad,))
    if hasattr(settings, "confidence"):
        raise ValueError("depth_leg_step takes dgr_dng.GaussianRasterizationSettings: it does not rescale gradients by `confidence`")
    const = isinstance(opacities, (int, float))
    if const and grad == "opacity":
        raise ValueError("a constant opacity has no gradient: grad='opacity' needs the activated opacity tensor")
    if means3D.device.type != "cuda":
        raise RuntimeError("gsplat depth pass got a tensor on %s - the rasterizer has no fallback path" % (means3D.device,))
    if const:
        opacities = _filled_opacity(means3D.device, means3D.shape[0], opacities)
    rs = settings
    backend = hip_backend()
    with torch.no_grad():
        det = lambda t: None if t is None else t.detach()   # noqa: E731
        depth, alpha, radii, rec = backend.depth_forward(
            means3D.detach(), opacities.detach(), det(scales), det(rotations), det(cov3D_precomp), rs.scale_modifier, rs.bg,
            rs.viewmatrix, rs.projmatrix, rs.campos, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, rs.debug)
    d, a = depth.requires_grad_(True), alpha.requires_grad_(True)
    loss = loss_fn(d, a)
    gd, ga = torch.autograd.grad(loss, (d, a), allow_unused=True)
    if rec is not None and not (gd is None and ga is None):
        with torch.no_grad():
            backend.depth_backward_step(rec, gd, ga, 1 if grad == "means" else 2, param, exp_avg, exp_avg_sq, lr, step, betas, eps)
    return loss.detach(), radii
