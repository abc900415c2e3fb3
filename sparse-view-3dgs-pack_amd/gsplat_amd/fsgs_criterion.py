"""The loss of one FSGS iteration (FSGS/train.py:94-109) on the kernels of the C ABI:

    loss = (1 - lambda) * L1(image, gt) + lambda * (1 - SSIM(image, gt))
           + depth_weight * min(1 - r(-midas, depth), 1 - r(1 / (midas + 200), depth))

on the UN-clamped render (FSGS's render() does not clamp).  `FsgsCriterion.fused_call` is ONE autograd node with two
differentiable inputs, the colour image and the depth image of the FSGS rasterizer generation; its photometric half is
FusedLGDWTLoss's kernel sequence with the clamp, the DWT and the patch terms off (gs_l1_fwd_p, gs_ssim_fwd_partials,
gs_lgdwt_combine_pp; backward gs_lgdwt_fused_bwd with flags = 0, or gs_l1_bwd_dev + gs_ssim_bwd_uniform where the image is
no multiple of 4 x 4), its depth half gs_pearson_fwd / gs_pearson_bwd, the branch of the min picked on the device.  No host
synchronisation; the only torch elementwise launch is the scalar `photometric + depth_weight * depth_term`.  The sums are
added in a fixed order (per-workgroup partials, combined in index order) whenever 3 * H * W is a multiple of 4; otherwise
the L1 sum falls back to gs_l1_fwd's float atomics, as in LGDWTCriterion.

`FsgsCriterion.__call__` is the same loss from differentiable ops (LossOps.l1_loss / fused_ssim) - the un-fused path and the
CPU checker's; the Pearson term is an injected callable there, because gsplat_amd.pearson has no CPU path."""

import torch

from ._lib import stream_of
from .losses import FusedLGDWTLoss, _FusedParams

_NEG, _RECIP200 = 1, 2   # GS_PEARSON_NEG, GS_PEARSON_RECIP200


class _Ctx:
    """What FusedLGDWTLoss.forward / backward use of an autograd context: the photometric half runs inside this node."""

    def __init__(self):
        self.saved_tensors = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *a):
        pass

    def set_materialize_grads(self, v):
        pass


class FusedFsgsLoss(torch.autograd.Function):
    """(criterion, image [3,H,W], depth [1,H,W] or [H,W], gt, midas, depth_weight) -> (loss, out [24] of gs_lgdwt_combine_pp,
    pearson [4] = chosen 1 - r, its r, both candidates; branch int32 [])."""

    @staticmethod
    def forward(ctx, crit, image, depth, gt, midas, depth_weight):
        ops = crit.ops
        api = ops.api
        dev = image.device
        fp, sums, rm, nomask = crit._buffers(tuple(image.shape), dev)
        pctx = _Ctx()
        photo, out = FusedLGDWTLoss.forward(pctx, ops, image.detach(), gt, nomask, sums, rm, fp, None)
        xf, tf = depth.detach().contiguous().view(-1), midas.detach().contiguous().view(-1)
        if xf.dtype != torch.float32 or tf.dtype != torch.float32:
            raise RuntimeError("FsgsCriterion: fp32 depth images only")
        n = int(xf.numel())
        if n != int(tf.numel()) or n < 2:
            raise ValueError("FsgsCriterion: the rendered depth has %d elements, the MiDaS depth %d" % (n, int(tf.numel())))
        pout = torch.empty((4,), dtype=torch.float32, device=dev)
        branch = torch.empty((), dtype=torch.int32, device=dev)
        tmp = torch.empty((int(api.raw("pearson_tmp_bytes")(n)),), dtype=torch.uint8, device=dev)
        api.call("pearson_fwd", xf.data_ptr(), tf.data_ptr(), n, _NEG, _RECIP200, tmp.data_ptr(), pout.data_ptr(),
                 branch.data_ptr(), stream_of(xf))
        loss = torch.add(photo, pout[0], alpha=float(depth_weight))   # (the node's one elementwise launch)
        ctx.crit, ctx.pctx, ctx.weight, ctx.n, ctx.depth_shape = crit, pctx, float(depth_weight), n, depth.shape
        ctx.tmp = tmp   # the statistics record: alive until the backward has been enqueued
        ctx.save_for_backward(xf, tf)
        ctx.mark_non_differentiable(out, pout, branch)
        ctx.set_materialize_grads(False)
        return loss, out, pout, branch

    @staticmethod
    def backward(ctx, g, _gout, _gp, _gb):
        if g is None:
            return (None,) * 6
        crit = ctx.crit
        api = crit.ops.api
        xf, tf = ctx.saved_tensors
        g_image = g_depth = None
        if ctx.needs_input_grad[2]:
            # dL/d(depth term) = upstream x depth_weight, read on the device: the cached constant when the backward was seeded
            # with LossOps.unit_grad (the train step), else one scalar multiply
            unit = crit.ops._unit.get(g.device)
            if unit is not None and g.data_ptr() == unit.data_ptr():
                coef = crit._weight_dev(ctx.weight, g.device)
            else:
                coef = (g.detach().reshape(1).to(torch.float32) * ctx.weight).contiguous()
            gx = torch.empty_like(xf)
            api.call("pearson_bwd", xf.data_ptr(), tf.data_ptr(), ctx.n, _NEG, _RECIP200, 0, ctx.tmp.data_ptr(), coef.data_ptr(),
                     gx.data_ptr(), None, stream_of(xf))
            g_depth = gx.view(ctx.depth_shape)
        if ctx.needs_input_grad[1]:
            g_image = FusedLGDWTLoss.backward(ctx.pctx, g, None)[1]
        ctx.tmp = None
        return None, g_image, g_depth, None, None, None


class FsgsCriterion:
    """FSGS/train.py:94-109 (see the module's docstring).  ops: a gsplat_amd.losses.LossOps.
    pearson: the depth term of the un-fused __call__, a callable (rendered_depth, midas_depth) -> scalar loss that is
    differentiable in rendered_depth; default gsplat_amd.pearson.depth_pearson_loss (HIP tensors only)."""

    # what _FusedParams reads of a criterion: the photometric base alone, on the image as it is
    dwt_enable = patch_dwt_enable = False
    clamp = False
    dwt_weights = (0.0,) * 8
    patch_size, patch_dwt_weight, patch_lh1_weight, patch_hl1_weight = 128, 0.0, 0.0, 0.0

    def __init__(self, ops, lambda_dssim=0.2, pearson=None):
        self.ops = ops
        self.lambda_dssim = lambda_dssim
        self.pearson = pearson
        # the one-node form needs the device library's partial-sum kernels and its Pearson kernels
        self.fused = all(hasattr(ops.api, "_" + n) for n in ("pearson_fwd", "pearson_bwd", "ssim_fwd_partials", "lgdwt_combine_pp"))
        self._fp, self._dev, self._weights = {}, {}, {}

    def _buffers(self, shape, dev):
        fp = self._fp.get(shape)
        if fp is None:
            if len(shape) != 3:
                raise ValueError("FsgsCriterion: the image is [C,H,W]")
            fp = self._fp[shape] = _FusedParams(self, *shape)
        d = self._dev.get(dev)
        if d is None:   # the combine kernel's accumulator (left zero by every call), its unused running mean, the absent patch mask
            d = self._dev[dev] = (torch.zeros((16,), dtype=torch.float32, device=dev),
                                  torch.ones((1,), dtype=torch.float32, device=dev),
                                  torch.zeros((1,), dtype=torch.uint8, device=dev))
        return (fp,) + d

    def _weight_dev(self, w, dev):
        key = (dev, w)
        t = self._weights.get(key)
        if t is None:   # (depth_weight takes two values in a run, FSGS/train.py:109-112)
            if len(self._weights) > 16:
                self._weights.clear()
            t = self._weights[key] = torch.full((1,), w, dtype=torch.float32, device=dev)
        return t

    def fused_call(self, image, depth, gt_image, midas_depth, depth_weight):
        """-> (loss, parts); parts: l1, ssim, base (the photometric loss), depth (the chosen 1 - r), r, branch (device int32:
        0 = the -midas form, 1 = the 1 / (midas + 200) form).  A constant depth image gives a NaN loss and a zero depth
        gradient; the image gradient is unaffected."""
        if not self.fused:
            raise RuntimeError("FsgsCriterion.fused_call needs the device library (no fallback): use __call__")
        if midas_depth.requires_grad:
            raise RuntimeError("FsgsCriterion: no gradient to midas_depth - detach it")
        loss, out, pout, branch = FusedFsgsLoss.apply(self, image, depth, gt_image, midas_depth, depth_weight)
        return loss, {"l1": out[5], "ssim": out[6], "base": out[1], "depth": pout[0], "r": pout[1], "branch": branch}

    def photometric(self, image, gt_image, l1_weight=None):
        """The photometric half on its own: l1_weight * L1 + lambda_dssim * (1 - SSIM) on the image as it is -> (base, L1, SSIM).
        l1_weight None: FSGS's 1 - lambda_dssim; DNGaussian's loop (train_llff.py:154-155) weighs L1 by 1."""
        ops = self.ops
        Ll1 = ops.l1_loss(image, gt_image)
        ssim_value = ops.fused_ssim(image.unsqueeze(0), gt_image.unsqueeze(0))
        w = (1.0 - self.lambda_dssim) if l1_weight is None else l1_weight
        return w * Ll1 + self.lambda_dssim * (1.0 - ssim_value), Ll1, ssim_value

    def __call__(self, image, depth, gt_image, midas_depth, depth_weight, pearson=None):
        base, Ll1, ssim_value = self.photometric(image, gt_image)
        pearson = pearson or self.pearson
        if pearson is None:
            if not depth.is_cuda:
                raise RuntimeError("FsgsCriterion: the Pearson depth term has no CPU path - pass `pearson`")
            from .pearson import depth_pearson_loss as pearson
        depth_loss = pearson(depth.reshape(-1, 1), midas_depth.reshape(-1, 1))
        loss = base + depth_weight * depth_loss
        return loss, {"l1": Ll1.detach(), "ssim": ssim_value.detach(), "base": base.detach(), "depth": depth_loss.detach()}
