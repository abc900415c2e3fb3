"""What DNGaussian's DTU loop (train_dtu.py) adds to the LLFF one, over libgsplat_hip.so (csrc/gs_dng_dtu.hip): the object
mask of a ground-truth image (:84-94), the masked-mean fill in front of both depth legs (:103-105, :136-138) and the alpha
penalty behind the mask (:155-159) as ONE autograd node each, and the colour-gated edits of the densification statistic and
the raw opacity in front of a densification (:218-230).

Nothing here synchronises with the host: the reference's boolean-index statements (a nonzero, so a blocking read-back, each)
become counts kept in device memory.  fp32 and CUDA(HIP) tensors only, no CPU path.  As in torch, a fill without an unmasked
pixel gives NaN, and a penalty over an empty mask a NaN loss with a gradient of zeros."""

import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of


def _ready(what, *tensors):
    gpu_tensors(what, tensors, dtypes=(torch.float32, torch.bool, torch.uint8))


def _mask_bytes(what, x, mask):
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s: the mask must be bool (or bytes), got %s" % (what, mask.dtype))
    if mask.numel() != x.numel():
        raise ValueError("%s: the image has %d elements and the mask %d" % (what, x.numel(), mask.numel()))
    if x.numel() < 1:
        raise ValueError("%s: an empty image" % what)
    return mask.detach().contiguous().view(torch.uint8)


def _tmp(n, device):
    return torch.empty((int(hip_api().raw("masked_tmp_bytes")(n)),), dtype=torch.uint8, device=device)


def dtu_background_mask(gt, threshold, run=50, out=None, return_count=False):
    """train_dtu.py:84-94 on gt [3,H,W]: dark = max over the channels < float32(threshold), strictly; a pixel is masked iff the
    run of dark pixels that ends at it going UP its column is at least min(y + 1, run) long (the reference's 49 shifted in-place
    products run along the rows).  -> (mask bool [1,H,W], gt with the masked pixels zero in all three channels).
    out: where the zeroed image goes; `gt` itself is allowed (the reference zeroes in place); default: a new tensor.
    return_count: also the masked count, an int32 tensor [1] on the device."""
    what = "dtu_background_mask"
    if not (gt.dim() == 3 and gt.shape[0] == 3 and gt.shape[1] >= 1 and gt.shape[2] >= 1):
        raise ValueError("%s: gt must be [3,H,W], got shape %s" % (what, tuple(gt.shape)))
    if int(run) < 1:
        raise ValueError("%s: run must be at least 1, got %d" % (what, run))
    _ready(what, gt)
    if gt.dtype != torch.float32:
        raise RuntimeError("%s: fp32 only (got %s)" % (what, gt.dtype))
    if not gt.is_contiguous():
        if out is gt:
            raise ValueError("%s: an in-place call needs a contiguous image" % what)
        gt = gt.contiguous()
    H, W = int(gt.shape[1]), int(gt.shape[2])
    if out is None:
        out = torch.empty_like(gt)
    elif not (out.shape == gt.shape and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous fp32 tensor of gt's shape on the GPU" % what)
    mask = torch.empty((1, H, W), dtype=torch.uint8, device=gt.device)
    count = torch.empty((1,), dtype=torch.int32, device=gt.device)
    hip_api().call("dtu_mask", gt.data_ptr(), H, W, float(threshold), int(run), mask.data_ptr(), count.data_ptr(), out.data_ptr(),
                   stream_of(gt))
    mask = mask.view(torch.bool)
    return (mask, out, count) if return_count else (mask, out)


class _MaskedMeanFill(Function):
    """(x, mask bytes, want_mean) -> (filled, mean [1] or None)"""

    @staticmethod
    def forward(ctx, x, mask, want_mean):
        ctx.set_materialize_grads(False)
        xf = x.detach().contiguous()
        n = xf.numel()
        out = torch.empty_like(xf)
        mean = torch.empty((1,), dtype=torch.float32, device=xf.device) if want_mean else None
        tmp = _tmp(n, xf.device)
        hip_api().call("masked_fill_fwd", xf.data_ptr(), mask.data_ptr(), n, tmp.data_ptr(), out.data_ptr(),
                       None if mean is None else mean.data_ptr(), stream_of(xf))
        ctx.mask = mask
        if mean is not None:
            ctx.mark_non_differentiable(mean)
        return out.view(x.shape), mean

    @staticmethod
    def backward(ctx, g, _gmean):
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        g = g.float().contiguous()
        gx = torch.empty_like(g)
        hip_api().call("masked_fill_bwd", g.data_ptr(), ctx.mask.data_ptr(), g.numel(), gx.data_ptr(), stream_of(g))
        return gx, None, None


class _AlphaPenalty(Function):
    """(alpha, mask bytes) -> loss []"""

    @staticmethod
    def forward(ctx, alpha, mask):
        af = alpha.detach().contiguous()
        n = af.numel()
        out = torch.empty((1,), dtype=torch.float32, device=af.device)
        tmp = _tmp(n, af.device)
        hip_api().call("alpha_penalty_fwd", af.data_ptr(), mask.data_ptr(), n, tmp.data_ptr(), out.data_ptr(), stream_of(af))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(af)
            ctx.mask, ctx.tmp, ctx.shape = mask, tmp, alpha.shape   # tmp: the masked count, alive until the backward is enqueued
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (af,) = ctx.saved_tensors
        g = g.float().contiguous()
        ga = torch.empty_like(af)
        hip_api().call("alpha_penalty_bwd", af.data_ptr(), ctx.mask.data_ptr(), af.numel(), ctx.tmp.data_ptr(), g.data_ptr(),
                       ga.data_ptr(), stream_of(af))
        ctx.tmp = None
        return ga.view(ctx.shape), None


def masked_mean_fill(x, mask, return_mean=False):
    """x with the pixels under `mask` (bool, x's element count) replaced by the mean of the others: `x[mask] =
    x[~mask].mean().detach()`.  The mean is a float64 sum in a fixed order, rounded to fp32 once; the other pixels keep their
    bits.  Backward: the masked pixels' cotangent is dropped, the others pass through; nothing flows through the mean.
    return_mean: also the mean, a tensor [1] on the device."""
    what = "masked_mean_fill"
    mb = _mask_bytes(what, x, mask)
    _ready(what, x, mb)
    if x.dtype != torch.float32:
        raise RuntimeError("%s: fp32 only (got %s)" % (what, x.dtype))
    out, mean = _MaskedMeanFill.apply(x, mb, bool(return_mean))
    return (out, mean) if return_mean else out


def alpha_penalty(alpha, mask):
    """mean(alpha[mask] ** 2): squares and sum in float64 in a fixed order, rounded once.  Backward: (g / count) * (2 alpha) in
    fp32 where masked, zero elsewhere.  An empty mask: a NaN loss and a gradient of zeros."""
    what = "alpha_penalty"
    mb = _mask_bytes(what, alpha, mask)
    _ready(what, alpha, mb)
    if alpha.dtype != torch.float32:
        raise RuntimeError("%s: fp32 only (got %s)" % (what, alpha.dtype))
    return _AlphaPenalty.apply(alpha, mb)


def reset_value(opacity=0.1):
    """inverse_sigmoid(opacity) as torch forms it in fp32 on the host: log(x / (1 - x)) - the bits the reference stores"""
    x = torch.full((1,), float(opacity), dtype=torch.float32)
    return float(torch.log(x / (1 - x))[0])


def _rule(what, name, rule):
    if rule is None:
        return 0, 0.0, 1.0, 0
    thr, div, reset = rule
    if not float(div) > 0.0:
        raise ValueError("%s: the %s rule's divisor must be positive, got %r" % (what, name, div))
    return 1, float(thr), float(div), int(bool(reset))


def colour_rule(colour, stat, opacity_raw, black=None, white=None, value=None):
    """train_dtu.py:218-230 in place, one launch: colour [P,3] (render()'s per-Gaussian colour), stat [P] or [P,1]
    (xyz_gradient_accum) and opacity_raw [P] or [P,1] (the model's raw opacity row), the last two contiguous and EDITED.
    black / white = (threshold, divisor, reset) or None (the rule is off): where max_c < float32(threshold) (black) or
    min_c > float32(threshold) (white), strictly, stat is divided by the divisor in fp32 and, if `reset`, the raw opacity becomes
    `value` (default reset_value(0.1)).  Black is applied before white.  Optimizer moments are not touched.
    -> counts, an int32 tensor [2] on the device: rows the black / the white rule fired on."""
    what = "colour_rule"
    if not (colour.dim() == 2 and colour.shape[1] == 3 and colour.shape[0] >= 1):
        raise ValueError("%s: colour must be [P,3] with P >= 1, got shape %s" % (what, tuple(colour.shape)))
    P = int(colour.shape[0])
    for name, t in (("stat", stat), ("opacity_raw", opacity_raw)):
        if not (t.numel() == P and (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1))):
            raise ValueError("%s: %s must be [P] or [P,1] with P = %d, got shape %s" % (what, name, P, tuple(t.shape)))
    b, w = _rule(what, "black", black), _rule(what, "white", white)
    gpu_tensors(what, (colour, stat, opacity_raw))
    for name, t in (("stat", stat), ("opacity_raw", opacity_raw)):
        if not t.is_contiguous():
            raise ValueError("%s: %s is edited in place and must be contiguous" % (what, name))
    value = reset_value(0.1) if value is None else float(value)
    cf = colour.detach().contiguous()
    counts = torch.empty((2,), dtype=torch.int32, device=cf.device)
    hip_api().call("dng_colour_rule", cf.data_ptr(), stat.data_ptr(), opacity_raw.data_ptr(), P, b[0], b[1], b[2], b[3],
                   w[0], w[1], w[2], w[3], value, counts.data_ptr(), stream_of(cf))
    return counts
