"""What DNGaussian's Blender loops (train_blender.py, `training` and `training_sh`) add for a white background, over
libgsplat_hip.so (csrc/gs_dng_blender.hip): the background mask of a ground-truth image with the mono-depth target zeroed under
it (:87, :96-97), and the white rule around a densification (:207-211, :366-370) on a given per-Gaussian colour or on the colour
of the SH rows as render_sh evaluates it (gaussian_renderer/__init__.py:351-355).

Nothing here synchronises with the host: the white rule's boolean-index statements (a gather through a boolean mask is a
nonzero, so a blocking read-back) become counts kept in device memory; the mask and the target are formed once per camera.  fp32 and CUDA(HIP) tensors only, no CPU path."""

import torch

from ._lib import gpu_tensors, hip_api, stream_of


def _ready(what, *tensors):
    gpu_tensors(what, tensors)


def blender_background_mask(gt, threshold, mono=None, return_count=False):
    """train_blender.py:87 on gt [3,H,W]: mask = gt.min(0) > float32(threshold), strictly (a NaN channel leaves its pixel
    unmasked) -> mask bool [1,H,W].
    mono [H,W] (any shape with H W elements; the stored map): also the depth legs' target (:96-97), `255.0 - mono` with the
    masked pixels +0.0, in mono's shape -> (mask, target).
    return_count: the masked count, an int32 tensor [1] on the device, comes last.  New tensors; nothing is edited in place."""
    what = "blender_background_mask"
    if not (gt.dim() == 3 and gt.shape[0] == 3 and gt.shape[1] >= 1 and gt.shape[2] >= 1):
        raise ValueError("%s: gt must be [3,H,W], got shape %s" % (what, tuple(gt.shape)))
    H, W = int(gt.shape[1]), int(gt.shape[2])
    if mono is not None and mono.numel() != H * W:
        raise ValueError("%s: mono has %d elements, the image %d pixels" % (what, mono.numel(), H * W))
    _ready(what, *((gt,) if mono is None else (gt, mono)))
    gt = gt.detach().contiguous()
    api = hip_api()
    mask = torch.empty((1, H, W), dtype=torch.uint8, device=gt.device)
    count = torch.empty((1,), dtype=torch.int32, device=gt.device)
    tmp = torch.empty((int(api.raw("blender_tmp_bytes")(H * W)),), dtype=torch.uint8, device=gt.device)
    target = None
    if mono is not None:
        mono = mono.detach().contiguous()
        target = torch.empty_like(mono)
    api.call("blender_target", gt.data_ptr(), None if mono is None else mono.data_ptr(), H, W, float(threshold), tmp.data_ptr(),
             mask.data_ptr(), count.data_ptr(), None if target is None else target.data_ptr(), stream_of(gt))
    out = (mask.view(torch.bool),) + (() if target is None else (target,)) + ((count,) if return_count else ())
    return out[0] if len(out) == 1 else out


def _rows(what, P, stat, opacity_raw):
    for name, t in (("stat", stat), ("opacity_raw", opacity_raw)):
        if not (t.numel() == P and (t.dim() == 1 or (t.dim() == 2 and t.shape[1] == 1))):
            raise ValueError("%s: %s must be [P] or [P,1] with P = %d, got shape %s" % (what, name, P, tuple(t.shape)))
    _ready(what, stat, opacity_raw)
    for name, t in (("stat", stat), ("opacity_raw", opacity_raw)):
        if not t.is_contiguous():
            raise ValueError("%s: %s is edited in place and must be contiguous" % (what, name))


def white_rule(colour, stat, opacity_raw, threshold, factor=0.1):
    """train_blender.py:207-211 in place, one kernel launch (behind a 4-byte memset of the count): colour [P,3] (render()'s per-Gaussian colour), stat [P] or [P,1]
    (xyz_gradient_accum) and opacity_raw [P] or [P,1] (the model's raw opacity row), the last two contiguous and EDITED.  Where
    min_c colour > float32(threshold), strictly (a NaN colour fires nothing): stat = 0 and
    opacity_raw = inverse_sigmoid(float32(factor) * sigmoid(opacity_raw)), evaluated in double and rounded once.  Optimizer
    moments are not touched.  -> counts, an int32 tensor [1] on the device: the rows that fired."""
    what = "white_rule"
    if not (colour.dim() == 2 and colour.shape[1] == 3 and colour.shape[0] >= 1):
        raise ValueError("%s: colour must be [P,3] with P >= 1, got shape %s" % (what, tuple(colour.shape)))
    P = int(colour.shape[0])
    _ready(what, colour)
    _rows(what, P, stat, opacity_raw)
    cf = colour.detach().contiguous()
    counts = torch.empty((1,), dtype=torch.int32, device=cf.device)
    hip_api().call("dng_white_rule", cf.data_ptr(), stat.data_ptr(), opacity_raw.data_ptr(), P, float(threshold), float(factor),
                   counts.data_ptr(), stream_of(cf))
    return counts


def white_rule_sh(xyz, shs, active_sh_degree, campos, stat, opacity_raw, threshold, factor=0.1, return_colour=False):
    """train_blender.py:366-370 in place, one kernel launch (behind a 4-byte memset of the count): white_rule on the colour render_sh hands back,
    max(eval_sh(active_sh_degree, shs, normalised(xyz - campos)) + 0.5, 0), evaluated in double and rounded once inside the
    kernel.  shs: the packed rows [P,M,3] or the pair (dc [P,1,3], rest [P,M-1,3]); M = 1, 4, 9 or 16, and the coefficients
    above the active degree are not read.  A Gaussian on the camera centre has NaN colours and does not fire (from degree 1 on;
    degree 0 does not use the direction).
    -> counts int32 [1] on the device, or (counts, colour [P,3]) with return_colour."""
    what = "white_rule_sh"
    if not (xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.shape[0] >= 1):
        raise ValueError("%s: xyz must be [P,3] with P >= 1, got shape %s" % (what, tuple(xyz.shape)))
    P = int(xyz.shape[0])
    if isinstance(shs, (tuple, list)):
        dc, rest = shs
        if not (dc.dim() == 3 and tuple(dc.shape) == (P, 1, 3)):
            raise ValueError("%s: dc must be [P,1,3], got shape %s" % (what, tuple(dc.shape)))
        if not (rest.dim() == 3 and rest.shape[0] == P and rest.shape[2] == 3):
            raise ValueError("%s: rest must be [P,M-1,3], got shape %s" % (what, tuple(rest.shape)))
        M = 1 + int(rest.shape[1])
        tensors = (dc, rest)
    else:
        if not (shs.dim() == 3 and shs.shape[0] == P and shs.shape[2] == 3):
            raise ValueError("%s: shs must be [P,M,3], got shape %s" % (what, tuple(shs.shape)))
        M = int(shs.shape[1])
        dc, rest, tensors = None, shs, (shs,)
    if M not in (1, 4, 9, 16):
        raise ValueError("%s: rows of 1, 4, 9 or 16 coefficients, got %d" % (what, M))
    deg = int(active_sh_degree)
    if deg < 0 or (deg + 1) ** 2 > M:
        raise ValueError("%s: active degree %d does not fit rows of %d coefficients" % (what, deg, M))
    if campos.numel() != 3:
        raise ValueError("%s: campos must hold 3 values, got shape %s" % (what, tuple(campos.shape)))
    _ready(what, xyz, campos, *tensors)
    _rows(what, P, stat, opacity_raw)
    xf, cp = xyz.detach().contiguous(), campos.detach().contiguous()
    dcf = None if dc is None else dc.detach().contiguous()
    rf = rest.detach().contiguous()
    counts = torch.empty((1,), dtype=torch.int32, device=xf.device)
    colour = torch.empty((P, 3), dtype=torch.float32, device=xf.device) if return_colour else None
    hip_api().call("dng_white_rule_sh", xf.data_ptr(), None if dcf is None else dcf.data_ptr(), rf.data_ptr() if rf.numel() else None,
                   M, deg, cp.data_ptr(), stat.data_ptr(), opacity_raw.data_ptr(), P, float(threshold), float(factor),
                   None if colour is None else colour.data_ptr(), counts.data_ptr(), stream_of(xf))
    return (counts, colour) if return_colour else counts
