"""Three per-Gaussian pieces of a DNGaussian training step over libgsplat_hip.so (csrc/gs_dng_reg.hip): the shape / scale /
opacity regulariser (DNGaussian/train_llff.py:159-165) as ONE autograd node, on the activated tensors or on the model's raw
rows; the view directions fed to the SH encoder (gaussian_renderer/__init__.py:22-23); the near-camera prune mask over all
spiral cameras (train_llff.py:209-213) in one launch.

Nothing here synchronises with the host: the reference's two boolean-index gathers (a nonzero each, so a blocking read-back
each) become counts kept in device memory; the regulariser's forward is two launches, its backward one, the directions one
each way, the mask one.  The weights travel as kernel arguments, the set sizes, the incoming gradient and the camera centres
stay in device memory.  fp32 and CUDA(HIP) tensors only, no CPU path.  An empty opacity set gives a NaN loss with finite
gradients, a Gaussian at the camera centre a NaN direction, as in torch."""

import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of

RAW = 1  # GS_DNG_REG_RAW
# what one workgroup sweeps at a time, and the largest grid (GS_DNG_REG_BLOCK_ROWS, GS_DNG_REG_MAX_BLOCKS of include/gsplat.h;
# tests/test_dng_reg_cpu.py holds them to the header)
BLOCK_ROWS = 1024
MAX_BLOCKS = 1024


def _rows3(what, name, t):
    if not (t.dim() == 2 and t.shape[1] == 3):
        raise ValueError("%s: %s must be [P,3], got shape %s" % (what, name, tuple(t.shape)))
    if t.shape[0] < 1:
        raise ValueError("%s: needs at least one Gaussian, got P = 0" % what)
    return int(t.shape[0])


def check_regulariser(what, scaling, opacity):
    """-> P; shapes are checked before devices, devices before dtypes."""
    P = _rows3(what, "scaling", scaling)
    if not (opacity.dim() == 1 or (opacity.dim() == 2 and opacity.shape[1] == 1)):
        raise ValueError("%s: opacity must be [P] or [P,1], got shape %s" % (what, tuple(opacity.shape)))
    if opacity.shape[0] != P:
        raise ValueError("%s: scaling has %d rows and opacity has %d" % (what, P, opacity.shape[0]))
    gpu_tensors(what, (scaling, opacity))
    return P


def check_view_dirs(what, xyz, campos):
    P = _rows3(what, "xyz", xyz)
    if tuple(campos.shape) != (3,):
        raise ValueError("%s: campos must be [3], got shape %s" % (what, tuple(campos.shape)))
    gpu_tensors(what, (xyz, campos))
    return P


def check_near_mask(what, xyz, centers):
    P = _rows3(what, "xyz", xyz)
    if not (centers.dim() == 2 and centers.shape[1] == 3):
        raise ValueError("%s: centers must be [K,3], got shape %s" % (what, tuple(centers.shape)))
    if centers.shape[0] < 1:
        raise ValueError("%s: needs at least one camera centre, got K = 0" % what)
    gpu_tensors(what, (xyz, centers))
    return P, int(centers.shape[0])


class _Regulariser(Function):
    """(scaling, opacity, w_shape, w_scale, w_opa, flags, max_blocks) -> (total [], terms [3])."""

    @staticmethod
    def forward(ctx, scaling, opacity, w_shape, w_scale, w_opa, flags, max_blocks):
        ctx.set_materialize_grads(False)
        ctx.shapes = (scaling.shape, opacity.shape)
        P = int(scaling.shape[0])
        sf, of = scaling.detach().contiguous(), opacity.detach().contiguous().view(-1)
        dev = sf.device
        api = hip_api()
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        tmp = torch.empty((int(api.raw("dng_reg_tmp_bytes")(P)),), dtype=torch.uint8, device=dev)
        api.call("dng_reg_fwd", sf.data_ptr(), of.data_ptr(), P, float(w_shape), float(w_scale), float(w_opa), int(flags),
                 int(max_blocks), tmp.data_ptr(), out.data_ptr(), stream_of(sf))
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(sf, of)
            ctx.tmp = tmp  # the record (P, n_hi, n_lo, weights): alive until the backward has been enqueued
            ctx.cfg = (P, int(flags))
        return out[3], out[:3]

    @staticmethod
    def backward(ctx, g_total, g_terms):
        if g_total is None and g_terms is None:
            return (None,) * 7
        sf, of = ctx.saved_tensors
        P, flags = ctx.cfg
        g_total = None if g_total is None else g_total.float().contiguous()
        g_terms = None if g_terms is None else g_terms.float().contiguous()
        gs = torch.empty_like(sf) if ctx.needs_input_grad[0] else None
        go = torch.empty_like(of) if ctx.needs_input_grad[1] else None
        hip_api().call("dng_reg_bwd", sf.data_ptr(), of.data_ptr(), P, flags, ctx.tmp.data_ptr(),
                       None if g_terms is None else g_terms.data_ptr(), None if g_total is None else g_total.data_ptr(),
                       None if gs is None else gs.data_ptr(), None if go is None else go.data_ptr(), stream_of(sf))
        ctx.tmp = None
        return (None if gs is None else gs.view(ctx.shapes[0]), None if go is None else go.view(ctx.shapes[1]),
                None, None, None, None, None)


class _ViewDirs(Function):
    """(xyz [P,3], campos [3]) -> [P,3]; no gradient to campos."""

    @staticmethod
    def forward(ctx, xyz, campos):
        ctx.set_materialize_grads(False)
        P = int(xyz.shape[0])
        xf, cf = xyz.detach().contiguous(), campos.detach().contiguous()
        out = torch.empty_like(xf)
        hip_api().call("view_dirs_fwd", xf.data_ptr(), cf.data_ptr(), P, out.data_ptr(), stream_of(xf))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(xf, cf)
        return out

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None
        xf, cf = ctx.saved_tensors
        g = g.float().contiguous()
        gx = torch.empty_like(xf)
        hip_api().call("view_dirs_bwd", xf.data_ptr(), cf.data_ptr(), int(xf.shape[0]), g.data_ptr(), gx.data_ptr(), stream_of(xf))
        return gx, None


def _regulariser(what, scaling, opacity, shape_pena, scale_pena, opa_pena, return_terms, flags, max_blocks):
    check_regulariser(what, scaling, opacity)
    total, terms = _Regulariser.apply(scaling, opacity, shape_pena, scale_pena, opa_pena, flags, max_blocks)
    return (total, terms) if return_terms else total


def gaussian_regulariser(scaling, opacity, shape_pena=0.001, scale_pena=0.001, opa_pena=0.01, return_terms=False, max_blocks=0):
    """shape_pena * mean(max / min of a scaling row) + scale_pena * mean(max^2) + opa_pena * (1 - mean(o^2 | o > 0.2) +
    mean((1 - o)^2 | o < 0.2)) on the ACTIVATED scaling [P,3] and opacity [P,1] or [P]: the scalar total, differentiable in
    both; return_terms: also the differentiable [3] terms (shape, scale, opa).  max_blocks caps the forward's grid (tests)."""
    return _regulariser("gaussian_regulariser", scaling, opacity, shape_pena, scale_pena, opa_pena, return_terms, 0, max_blocks)


def gaussian_regulariser_raw(scaling, opacity, shape_pena=0.001, scale_pena=0.001, opa_pena=0.01, return_terms=False,
                             max_blocks=0):
    """The same on the model's raw rows (_scaling, _opacity): exp and sigmoid are evaluated inside the kernels, the gradients
    are with respect to the raw values, no activated tensor is written."""
    return _regulariser("gaussian_regulariser_raw", scaling, opacity, shape_pena, scale_pena, opa_pena, return_terms, RAW,
                        max_blocks)


def view_dirs(xyz, campos):
    """(xyz - campos) / |xyz - campos| per row, [P,3]; campos is a device tensor [3] and gets no gradient."""
    check_view_dirs("view_dirs", xyz, campos)
    return _ViewDirs.apply(xyz, campos)


def near_camera_mask(xyz, centers, near):
    """bool [P]: the Gaussian lies within `near` of any of the camera centres [K,3].  Not differentiable."""
    P, K = check_near_mask("near_camera_mask", xyz, centers)
    xf, cf = xyz.detach().contiguous(), centers.detach().contiguous()
    mask = torch.empty((P,), dtype=torch.bool, device=xf.device)
    hip_api().call("near_mask", xf.data_ptr(), P, cf.data_ptr(), K, float(near), mask.data_ptr(), stream_of(xf))
    return mask
