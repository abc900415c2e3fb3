"""FSGS's depth-correlation term over libgsplat_hip.so (csrc/gs_pearson.hip): Pearson's r of two fp32 sequences, and the
training script's `min(1 - r(-midas, depth), 1 - r(1 / (midas + 200), depth))` (FSGS/train.py:105-108) as ONE autograd node
whose branch is picked on the device.

Nothing here synchronises with the host: the forward is two launches, the backward one; the chosen branch, the statistics
and the incoming gradient all stay in device memory.  fp32 and CUDA(HIP) tensors only, no CPU path.  A constant sequence
gives NaN and a zero gradient."""

import torch
from torch.autograd import Function

from ._lib import gpu_tensors, hip_api, stream_of

ID, NEG, RECIP200 = 0, 1, 2  # GS_PEARSON_ID, GS_PEARSON_NEG, GS_PEARSON_RECIP200
WRT_R = 1                    # GS_PEARSON_WRT_R
# what one workgroup sweeps at a time, and the largest grid (GS_PEARSON_BLOCK_ELEMS, GS_PEARSON_MAX_BLOCKS of include/gsplat.h;
# tests/test_fsgs_loss_cpu.py holds them to the header)
BLOCK_ELEMS = 4096
MAX_BLOCKS = 512


def flat_pair(what, a, b, names, columns=False):
    """Two tensors with the same element count -> that count; shapes are checked before devices, devices before dtypes.
    columns: torchmetrics' contract - [N] or [N,1] only, [N,d] with d > 1 (its multi-output form) raises."""
    for t, name in zip((a, b), names):
        if columns and not (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1)):
            raise ValueError("%s: %s must be [N] or [N,1], got shape %s" % (what, name, tuple(t.shape)))
    if a.numel() != b.numel():
        raise ValueError("%s: %s has %d elements and %s has %d" % (what, names[0], a.numel(), names[1], b.numel()))
    if a.numel() < 2:
        raise ValueError("%s: needs at least 2 elements, got %d" % (what, a.numel()))
    gpu_tensors(what, (a, b))
    return int(a.numel())


class _Pearson(Function):
    """(x, t, form_a, form_b, want_r) -> (1 - r of the chosen form, or r itself; branch int32 [])."""

    @staticmethod
    def forward(ctx, x, t, form_a, form_b, want_r):
        ctx.set_materialize_grads(False)
        ctx.shapes = (x.shape, t.shape)
        n = int(x.numel())
        xf, tf = x.detach().contiguous().view(-1), t.detach().contiguous().view(-1)
        dev = xf.device
        api = hip_api()
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        branch = torch.empty((), dtype=torch.int32, device=dev)
        tmp = torch.empty((int(api.raw("pearson_tmp_bytes")(n)),), dtype=torch.uint8, device=dev)
        api.call("pearson_fwd", xf.data_ptr(), tf.data_ptr(), n, form_a, form_b, tmp.data_ptr(), out.data_ptr(),
                 branch.data_ptr(), stream_of(xf))
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(xf, tf)
            ctx.tmp = tmp  # the statistics record: alive until the backward has been enqueued
            ctx.cfg = (n, int(form_a), int(form_b), WRT_R if want_r else 0)
        ctx.mark_non_differentiable(branch)
        return out[1 if want_r else 0], branch

    @staticmethod
    def backward(ctx, g, _gbranch):
        if g is None:
            return None, None, None, None, None
        xf, tf = ctx.saved_tensors
        n, form_a, form_b, flags = ctx.cfg
        g = g.float().contiguous()
        gx = torch.empty_like(xf) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(tf) if ctx.needs_input_grad[1] else None
        hip_api().call("pearson_bwd", xf.data_ptr(), tf.data_ptr(), n, form_a, form_b, flags, ctx.tmp.data_ptr(), g.data_ptr(),
                       None if gx is None else gx.data_ptr(), None if gt is None else gt.data_ptr(), stream_of(xf))
        ctx.tmp = None
        return (None if gx is None else gx.view(ctx.shapes[0]), None if gt is None else gt.view(ctx.shapes[1]), None, None,
                None)


def pearson_corrcoef(preds, target):
    """torchmetrics.functional.pearson_corrcoef for one output: [N] or [N,1] each -> the scalar r, differentiable in both."""
    flat_pair("pearson_corrcoef", preds, target, ("preds", "target"), columns=True)
    return _Pearson.apply(preds, target, ID, -1, True)[0]


def depth_pearson_loss(rendered_depth, midas_depth, return_branch=False):
    """min(1 - r(-midas, depth), 1 - r(1 / (midas + 200), depth)), FSGS/train.py:105-108, with Python's min rule (the second
    only if it is smaller; a tie or a NaN keeps the first) applied on the device.  Gradient to rendered_depth only.
    return_branch: also the branch taken, 0 / 1, as a device int32 scalar."""
    if midas_depth.requires_grad:
        raise RuntimeError("depth_pearson_loss: no gradient to midas_depth (1 / (midas + 200) has no backward here) - detach it")
    flat_pair("depth_pearson_loss", rendered_depth, midas_depth, ("rendered_depth", "midas_depth"))
    loss, branch = _Pearson.apply(rendered_depth, midas_depth, NEG, RECIP200, False)
    return (loss, branch) if return_branch else loss


def pseudo_depth_pearson_loss(rendered_depth, midas_depth):
    """1 - r(depth, -midas), FSGS/train.py:127: the pseudo view's term, differentiable in both (the MiDaS estimate of a
    rendered pseudo view carries gradient in the reference)."""
    flat_pair("pseudo_depth_pearson_loss", rendered_depth, midas_depth, ("rendered_depth", "midas_depth"))
    return _Pearson.apply(rendered_depth, midas_depth, NEG, -1, False)[0]
