"""DNGaussian's depth-normalisation regulariser over libgsplat_hip.so (csrc/gs_depth_norm.hip): the patch-normalised
margin losses (utils/loss_utils.py: patch_norm_{mse,l1}_loss[_global]), loss_depth_smoothness, and the fused node that
serves a training script's whole `0.1 local + 0.1 smoothness + 1 global` call with one forward and one backward.

Divergences from the reference, all raised or documented: batch 1 and one channel only, no gradient to the target,
fp32 only, CUDA(HIP) tensors only.  An empty mask gives a NaN loss and a zero gradient, as in the reference.

Nothing here synchronises with the host: the masked count stays on the device and the backward reads the incoming
dL/dloss from device memory."""

import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of

GLOBAL, L1 = 1, 2  # GS_DN_GLOBAL, GS_DN_L1


def _image(t, what, channels_one=True):
    """[1,C,H,W] (or [C,H,W]) -> (contiguous fp32 tensor, C, H, W); shapes are checked before devices."""
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError("%s: expected a [1,C,H,W] image, got shape %s" % (what, tuple(t.shape)))
    if t.shape[0] != 1:
        raise ValueError("%s: batch 1 only (got batch %d) - call it once per image" % (what, t.shape[0]))
    if channels_one and t.shape[1] != 1:
        raise ValueError("%s: one channel only (got %d)" % (what, t.shape[1]))
    return t, int(t.shape[1]), int(t.shape[2]), int(t.shape[3])


def _ready(what, *tensors):
    """Tensor by tensor: the first tensor's dtype is reported before the second one's device."""
    return [gpu_tensors(what, (t,), contiguous=True)[0] for t in tensors]


def _patch_size(what, p, H, W):
    p = int(p)
    if p < 2 or p > min(H, W):
        raise ValueError("%s: patch size %d outside 2..min(H, W) = %d" % (what, p, min(H, W)))
    return p


class _Workspaces:
    """Device scratch that lives from a forward to its backward, then serves the next forward (a training step runs the
    same few shapes over and over).  A forward whose backward never runs just drops its buffer."""
    KEEP = 8

    def __init__(self):
        self.free = []

    def take(self, device, nbytes):
        for i, b in enumerate(self.free):
            if b.device == device and b.numel() >= nbytes:
                return self.free.pop(i)
        return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)

    def give(self, buf):
        if len(self.free) < self.KEEP:
            self.free.append(buf)


_ws = _Workspaces()


def _tmp(device, H, W, p0, p1):
    nbytes = int(hip_api().raw("depth_norm_tmp_bytes")(H, W, p0, p1))
    if nbytes == 0:
        raise ValueError("depth_norm: no workspace for H=%d W=%d p=(%d, %d)" % (H, W, p0, p1))
    return _ws.take(device, nbytes)


class _PatchNormLoss(Function):
    """(input [1,1,H,W], target, p, margin, flags, want_mask) -> (loss, mask [L, p*p] bool or None)."""

    @staticmethod
    def forward(ctx, input, target, p, margin, flags, want_mask):
        what = "patch_norm_loss"
        ctx.set_materialize_grads(False)  # no zero tensors for the mask / parts outputs in the backward
        ctx.shape = input.shape
        input, _, H, W = _image(input, what + " input")
        target, _, Ht, Wt = _image(target, what + " target")
        if (Ht, Wt) != (H, W):
            raise ValueError("%s: input %dx%d and target %dx%d differ" % (what, H, W, Ht, Wt))
        p = _patch_size(what, p, H, W)
        input, target = _ready(what, input, target)
        dev = input.device
        L = (H // p) * (W // p)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        mask = torch.empty((L, p * p), dtype=torch.uint8, device=dev) if want_mask else None
        tmp = _tmp(dev, H, W, p, 0)
        hip_api().call("depth_norm_fwd", input.data_ptr(), target.data_ptr(), H, W, p, float(margin), int(flags),
                       tmp.data_ptr(), loss.data_ptr(), mask.data_ptr() if want_mask else None, stream_of(input))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(input, target)
            ctx.tmp = tmp
            ctx.cfg = (H, W, p, float(margin), int(flags))
        else:
            _ws.give(tmp)
        if want_mask:
            mask = mask.view(torch.bool)
            ctx.mark_non_differentiable(mask)
        return loss, mask

    @staticmethod
    def backward(ctx, gloss, _gmask):
        input, target = ctx.saved_tensors
        H, W, p, margin, flags = ctx.cfg
        gloss = gloss.float().contiguous()
        grad = torch.empty_like(input)
        hip_api().call("depth_norm_bwd", input.data_ptr(), target.data_ptr(), H, W, p, margin, flags, ctx.tmp.data_ptr(),
                       gloss.data_ptr(), grad.data_ptr(), stream_of(input))
        _ws.give(ctx.tmp)
        ctx.tmp = None
        return grad.view(ctx.shape), None, None, None, None, None


class _DepthSmoothness(Function):
    """(depth [1,1,H,W], img [1,C,H,W]) -> loss."""

    @staticmethod
    def forward(ctx, depth, img):
        what = "loss_depth_smoothness"
        ctx.set_materialize_grads(False)  # no zero tensors for the mask / parts outputs in the backward
        ctx.shape = depth.shape
        depth, _, H, W = _image(depth, what + " depth")
        img, Cn, Hi, Wi = _image(img, what + " img", channels_one=False)
        if (Hi, Wi) != (H, W):
            raise ValueError("%s: depth %dx%d and img %dx%d differ" % (what, H, W, Hi, Wi))
        depth, img = _ready(what, depth, img)
        loss = torch.empty((), dtype=torch.float32, device=depth.device)
        tmp = _tmp(depth.device, H, W, 0, 0)
        hip_api().call("depth_smooth_fwd", depth.data_ptr(), img.data_ptr(), Cn, H, W, tmp.data_ptr(), loss.data_ptr(),
                       stream_of(depth))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(depth, img)
            ctx.tmp = tmp
            ctx.cfg = (Cn, H, W)
        else:
            _ws.give(tmp)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        depth, img = ctx.saved_tensors
        Cn, H, W = ctx.cfg
        gloss = gloss.float().contiguous()
        grad = torch.empty_like(depth)
        hip_api().call("depth_smooth_bwd", depth.data_ptr(), img.data_ptr(), Cn, H, W, ctx.tmp.data_ptr(), gloss.data_ptr(),
                       grad.data_ptr(), stream_of(depth))
        _ws.give(ctx.tmp)
        ctx.tmp = None
        return grad.view(ctx.shape), None


class _DepthRegulariser(Function):
    """(depth, depth_mono, p_local, p_global, margin, w_local, w_global, w_smooth, want_masks) ->
    (total, parts [4] = total / local / global / smoothness, mask_local, mask_global)."""

    @staticmethod
    def forward(ctx, depth, mono, p_local, p_global, margin, w_local, w_global, w_smooth, want_masks):
        what = "depth_regulariser"
        ctx.set_materialize_grads(False)  # no zero tensors for the mask / parts outputs in the backward
        ctx.shape = depth.shape
        depth, _, H, W = _image(depth, what + " depth")
        mono, _, Hm, Wm = _image(mono, what + " depth_mono")
        if (Hm, Wm) != (H, W):
            raise ValueError("%s: depth %dx%d and depth_mono %dx%d differ" % (what, H, W, Hm, Wm))
        p_local, p_global = _patch_size(what, p_local, H, W), _patch_size(what, p_global, H, W)
        depth, mono = _ready(what, depth, mono)
        dev = depth.device
        parts = torch.empty((4,), dtype=torch.float32, device=dev)
        ml = mg = None
        if want_masks:
            ml = torch.empty(((H // p_local) * (W // p_local), p_local * p_local), dtype=torch.uint8, device=dev)
            mg = torch.empty(((H // p_global) * (W // p_global), p_global * p_global), dtype=torch.uint8, device=dev)
        tmp = _tmp(dev, H, W, p_local, p_global)
        cfg = (H, W, p_local, p_global, float(margin), float(w_local), float(w_global), float(w_smooth))
        hip_api().call("dng_depth_reg_fwd", depth.data_ptr(), mono.data_ptr(), *cfg, tmp.data_ptr(), parts.data_ptr(),
                       ml.data_ptr() if want_masks else None, mg.data_ptr() if want_masks else None, stream_of(depth))
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(depth, mono)
            ctx.tmp = tmp
            ctx.cfg = cfg
        else:
            _ws.give(tmp)
        total = parts[0]
        ctx.mark_non_differentiable(parts)
        if want_masks:
            ml, mg = ml.view(torch.bool), mg.view(torch.bool)
            ctx.mark_non_differentiable(ml, mg)
        return total, parts, ml, mg

    @staticmethod
    def backward(ctx, gtotal, _gparts, _gml, _gmg):
        depth, mono = ctx.saved_tensors
        gtotal = gtotal.float().contiguous()
        grad = torch.empty_like(depth)
        hip_api().call("dng_depth_reg_bwd", depth.data_ptr(), mono.data_ptr(), *ctx.cfg, ctx.tmp.data_ptr(),
                       gtotal.data_ptr(), grad.data_ptr(), stream_of(depth))
        _ws.give(ctx.tmp)
        ctx.tmp = None
        return grad.view(ctx.shape), None, None, None, None, None, None, None, None


def patch_norm_loss(input, target, patch_size, margin, flags, return_mask=False):
    loss, mask = _PatchNormLoss.apply(input, target, patch_size, margin, flags, bool(return_mask))
    return (loss, mask) if return_mask else loss


def depth_smoothness(depth, img):
    return _DepthSmoothness.apply(depth, img)


def depth_regulariser(depth, depth_mono, p_local, p_global, margin, w_local=0.1, w_global=1.0, w_smooth=0.0,
                      return_parts=False):
    """w_local * patch_norm_mse_loss(depth, depth_mono, p_local, margin)
    + w_smooth * loss_depth_smoothness(depth, depth_mono)        (skipped when w_smooth == 0)
    + w_global * patch_norm_mse_loss_global(depth, depth_mono, p_global, margin)
    in one forward and one backward.  depth_mono is what the reference passes as the target (255 - the mono depth).
    return_parts: also (parts [4] = total / local / global / smoothness, mask_local, mask_global)."""
    total, parts, ml, mg = _DepthRegulariser.apply(depth, depth_mono, p_local, p_global, margin, w_local, w_global, w_smooth,
                                                   bool(return_parts))
    return (total, parts, ml, mg) if return_parts else total
