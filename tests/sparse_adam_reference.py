"""SparseGaussianAdam's two update rules, restated per element in numpy: the arbiter of tests/test_sparse_gaussian_adam_cpu.py,
tests/test_gpu_sparse_gaussian_adam.py and the loop test of tests/test_gpu_rasterizer_dc.py.

A tensor of a param group has P rows of `row_width` floats; row r is stepped when row_mask[r] is set (no mask: every row).
Rows that are not stepped keep every bit of p, m and v, NaNs included.

  bias_correction=True   torch.optim.Adam's rule.  It IS step_reference.adam_ref (called, not restated again).
  bias_correction=False  the accelerated rasterizer's rule - Adam's moments without bias correction:
                             m = b1 m + (1 - b1) g ;  v = b2 v + ((1 - b2) g) g ;  p = p - lr (m / (sqrt(v) + eps))
                         float64: the arbiter for parameters; float32: one IEEE rounding per operation in that order (the
                         kernel is compiled without contraction), bit-exact for m and v.
"""
import numpy as np

from step_reference import BETA1, BETA2, EPS, adam_ref

WIDTHS = (3, 3, 45, 1, 3, 4)                       # xyz, f_dc, f_rest, opacity, scaling, rotation (gaussian_model.py:183-190)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.025, 0.005, 0.001)


def stepped_elements(P, row_width, row_mask):
    if row_mask is None:
        return np.ones(P * row_width, bool)
    row_mask = np.asarray(row_mask).astype(bool)
    assert row_mask.shape == (P,)
    return np.repeat(row_mask, row_width)


def no_bias_ref(p, g, m, v, lr, stepped, dtype=np.float64, betas=(BETA1, BETA2), eps=EPS):
    """One step of the rule without bias correction per element -> (p, m, v) of `dtype`; p, g, m, v: float32 arrays."""
    stepped = np.asarray(stepped, bool)
    if dtype == np.float64:
        b1, b2, e = float(betas[0]), float(betas[1]), float(eps)
        p, g, m, v = (np.asarray(x, np.float32).astype(np.float64) for x in (p, g, m, v))
        lr = np.float64(lr)
        one_b1, one_b2 = 1.0 - b1, 1.0 - b2
    else:
        assert dtype == np.float32
        f = np.float32
        b1, b2, e = f(betas[0]), f(betas[1]), f(eps)     # (the C ABI takes them as float)
        p, g, m, v = (np.asarray(x, np.float32) for x in (p, g, m, v))
        lr = f(lr)
        one_b1, one_b2 = f(1.0) - b1, f(1.0) - b2
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        m1 = b1 * m + one_b1 * g
        v1 = b2 * v + (one_b2 * g) * g
        p1 = p - lr * (m1 / (np.sqrt(v1) + e))
    for x in (m1, v1, p1):
        assert x.dtype == dtype
    return np.where(stepped, p1, p), np.where(stepped, m1, m), np.where(stepped, v1, v)


def sparse_adam_ref(p, g, m, v, lr, t, row_width, row_mask, bias_correction, dtype=np.float64, betas=(BETA1, BETA2), eps=EPS):
    """One SparseGaussianAdam step of ONE tensor (flat float32 arrays of P * row_width elements, learning rate lr, 1-based step
    count t) -> (p, m, v) of `dtype`."""
    p = np.asarray(p, np.float32)
    P = p.size // row_width
    assert P * row_width == p.size
    stepped = stepped_elements(P, row_width, row_mask)
    if bias_correction:
        with np.errstate(under="ignore", invalid="ignore", over="ignore"):
            return adam_ref(p, g, m, v, np.full(p.size, lr, np.float64), np.full(p.size, int(t), np.int64), stepped, dtype,
                            betas=betas, eps=eps)
    return no_bias_ref(p, g, m, v, lr, stepped, dtype, betas=betas, eps=eps)


def masks(P, seed=0):
    """The row masks of the GPU test: {name: bool [P]}."""
    out = {"none": np.zeros(P, bool), "all": np.ones(P, bool), "every_other": np.arange(P) % 2 == 0,
           "row0": np.arange(P) == 0, "last_row": np.arange(P) == P - 1}
    if P >= 2 * 256 + 1:   # one visible row between runs of >= 256 invisible ones: a whole-wave skip next to a mixed wave
        out["lone_row"] = np.arange(P) == P // 2
    out["random30"] = np.random.default_rng(seed + P).random(P) < 0.3
    return out
