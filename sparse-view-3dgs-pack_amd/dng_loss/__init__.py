"""DNGaussian's depth-normalisation losses on the MI355X kernels - same names and signatures as the reference's
DNGaussian/utils/loss_utils.py (patch_norm_mse_loss, patch_norm_mse_loss_global, patch_norm_l1_loss,
patch_norm_l1_loss_global, loss_depth_smoothness), served by libgsplat_hip.so (csrc/gs_depth_norm.hip), plus
depth_regulariser: a training script's whole `0.1 local + 0.1 smoothness + 1 global` call as one forward and one
backward; and what train_dtu.py puts around those calls (csrc/gs_dng_dtu.hip): dtu_background_mask (:84-94),
masked_mean_fill (:103-105, :136-138) and alpha_penalty (:155-159), one autograd node each; and train_blender.py's
blender_background_mask (:87, :96-97; csrc/gs_dng_blender.hip).  No CPU fallback.

Divergences: batch 1 and one channel only (ValueError otherwise), no gradient to the target, fp32 only.  As in the
reference, an empty mask gives a NaN loss and a zero gradient."""
from gsplat_amd import depth_norm as _dn
from gsplat_amd.depth_norm import depth_regulariser  # noqa: F401
from gsplat_amd.dng_blender import blender_background_mask  # noqa: F401
from gsplat_amd.dng_dtu import alpha_penalty, dtu_background_mask, masked_mean_fill  # noqa: F401

__all__ = ["patch_norm_mse_loss", "patch_norm_mse_loss_global", "patch_norm_l1_loss", "patch_norm_l1_loss_global",
           "loss_depth_smoothness", "depth_regulariser"]
# (the DTU loop's three and the Blender loops' one are importable by name; the star-export stays the reference's loss_utils names)


def patch_norm_mse_loss(input, target, patch_size, margin, return_mask=False):
    return _dn.patch_norm_loss(input, target, patch_size, margin, 0, return_mask)


def patch_norm_mse_loss_global(input, target, patch_size, margin, return_mask=False):
    return _dn.patch_norm_loss(input, target, patch_size, margin, _dn.GLOBAL, return_mask)


def patch_norm_l1_loss_global(input, target, patch_size, margin, return_mask=False):
    return _dn.patch_norm_loss(input, target, patch_size, margin, _dn.GLOBAL | _dn.L1, return_mask)


def patch_norm_l1_loss(input, target, patch_size, margin, return_mask=False):
    return _dn.patch_norm_loss(input, target, patch_size, margin, _dn.L1, return_mask)


def loss_depth_smoothness(depth, img):
    return _dn.depth_smoothness(depth, img)
