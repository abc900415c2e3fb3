"""FSGS's depth-correlation losses on the MI355X kernels (csrc/gs_pearson.hip through gsplat_amd/pearson.py).  No CPU
fallback.

  pearson_corrcoef(preds, target)                    torchmetrics.functional.pearson_corrcoef for one output: the scalar r
  depth_pearson_loss(rendered_depth, midas_depth)    FSGS/train.py:105-108, both forms from one read, min taken on the device
  pseudo_depth_pearson_loss(rendered_depth, midas)   FSGS/train.py:127, 1 - r(depth, -midas), gradients to both
  FsgsCriterion / criterion(**kw)                    the whole loss of an iteration (FSGS/train.py:94-109) as one autograd node
                                                     on the un-clamped render and its depth image (gsplat_amd/fsgs_criterion.py)

A training script changes one import line: `from torchmetrics.functional.regression import pearson_corrcoef` becomes
`from fsgs_loss import pearson_corrcoef` (there is no torchmetrics stand-in package); the two fused functions replace the
expressions around it and remove the host comparison of Python's min.

Divergences: fp32 and one output only; fewer than 2 elements raise ValueError instead of returning NaN; the depth loss
gives no gradient to midas_depth.  A constant sequence gives NaN with a zero gradient."""
from gsplat_amd.fsgs_criterion import FsgsCriterion  # noqa: F401
from gsplat_amd.pearson import depth_pearson_loss, pearson_corrcoef, pseudo_depth_pearson_loss  # noqa: F401

# (the star-import surface stays the three functions a training script's loss lines use; the criterion is imported by name)
__all__ = ["pearson_corrcoef", "depth_pearson_loss", "pseudo_depth_pearson_loss"]


def criterion(**kw):
    """FsgsCriterion on the device library's loss kernels."""
    import lgdwt_loss
    return FsgsCriterion(lgdwt_loss.ops(), **kw)
