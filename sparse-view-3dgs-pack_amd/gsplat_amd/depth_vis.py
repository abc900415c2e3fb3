"""The coloured depth map of the render stage: DNGaussian/render.py:121,127-130 (spiral.py:114-121) and FSGS's vis_depth
(utils/general_utils.py:157-176), on the device through gs_depth_vis (csrc/gs_depth_vis.hip), on CPU tensors in numpy.

  turbo_table()      matplotlib's 256 x 3 turbo table, float64 (gsplat_amd/_turbo.py holds it as data: matplotlib is no dependency)
  byte_tables()      the two ways the reference turns a table row into bytes, both returned in R, G, B order = file order:
                       "save_image"  torchvision.utils.save_image on the float64 image: mul(255).add(0.5).clamp(0, 255), truncated
                                     (DNGaussian; also used for the identity rule, visualize_cmap's default curve)
                       "trunc"       np.uint8(c * 255): truncation (FSGS).  vis_depth returns c[..., ::-1], B, G, R, and hands it to
                                     cv2.imwrite, which stores R, G, B on disk: the file's bytes are these
  colour_depth()     uint8 [H,W,3] on the input's device
  composite_depth()  render.py:121's image and the grey bytes save_image writes for 1 - d (render.py:124)

The statements matched (numpy 2 promotion: a float32 array with a float64 scalar computes in float64):
  x sorted by np.argsort (NaN last); acc_w = np.cumsum(ones) = 1..n in float32; queries [0.5, 99.5] * float32(n / 100) in
  float64; np.interp(queries, acc_w, x): the first value left of the first node, a node's own value on a node, otherwise
  slope * (q - xp[j]) + fp[j] in double (for n < 200 the low query lies left of the first node)
  lo = lo_auto - eps, hi = hi_auto + eps, eps = float32's epsilon ("dng", "identity") or 1e-10 ("fsgs")
  curve: "dng" -log(x + eps32), "fsgs" 1 / x + 1e-10, "identity" x - on the float32 image in float32, on lo and hi in float64
  v = nan_to_num(clip((curve(x) - min(lo', hi')) / |hi' - lo'|, 0, 1)) in float64; row trunc(256 v), 256 -> 255 (matplotlib)
The device evaluates "dng"'s logarithm of a pixel in double and rounds it to float32 once, where numpy's float32 log is
within a few ulp of that: a pixel whose 256 v lies that close to an integer may take the neighbouring row
(tests/test_gpu_depth_vis.py states the allowance).  The other two rules are IEEE-exact on both sides.  Images of up to 2^24
pixels: beyond, float32's cumulative sum of ones stops counting."""
import numpy as np
import torch

from ._turbo import TURBO

RULES = {"identity": 0, "dng": 1, "fsgs": 2}
_BYTE_RULE = {"identity": "save_image", "dng": "save_image", "fsgs": "trunc"}
EPS32 = np.finfo(np.float32).eps
MAX_PIXELS = 1 << 24
_device_luts = {}


def turbo_table():
    """-> float64 [256,3], matplotlib.colormaps["turbo"](np.arange(256))[:, :3]"""
    return np.array(TURBO, dtype=np.float64)


def byte_tables():
    """-> {"save_image": uint8 [256,3], "trunc": uint8 [256,3]}, both R, G, B"""
    t = turbo_table()
    return {"save_image": np.clip(t * 255 + 0.5, 0, 255).astype(np.uint8), "trunc": np.uint8(t * 255)}


def _plane(t, what):
    if not torch.is_tensor(t):
        raise ValueError("%s: expected a tensor, got %s" % (what, type(t).__name__))
    t = t.detach()
    while t.dim() > 2 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise ValueError("%s: one [H,W] or [1,H,W] image (got shape %s)" % (what, tuple(t.shape)))
    return t.to(torch.float32).contiguous()


def _check(depth, alpha, rule):
    if rule not in RULES:
        raise ValueError("colour_depth: rule is one of %s (got %r)" % (sorted(RULES), rule))
    d = _plane(depth, "depth")
    a = None if alpha is None else _plane(alpha, "alpha")
    if a is not None and (a.shape != d.shape or a.device != d.device):
        raise ValueError("depth %s on %s and alpha %s on %s differ" % (tuple(d.shape), d.device, tuple(a.shape), a.device))
    if d.numel() > MAX_PIXELS:
        raise ValueError("colour_depth: at most 2^24 pixels (got %d x %d)" % tuple(d.shape))
    return d, a


# --------------------------------------------------------------------------------------------------- numpy restatement
def percentile_bounds_numpy(x, eps):
    """x float32 [H,W] -> (lo, hi) np.float64: weighted_percentile(x, ones, [0.5, 99.5]) widened by eps"""
    xs = x.reshape(-1)
    xs = xs[np.argsort(xs)]
    acc_w = np.cumsum(np.ones_like(xs))
    lo_auto, hi_auto = np.interp(np.array([50 - 99. / 2, 50 + 99. / 2]) * (acc_w[-1] / 100), acc_w, xs)
    return lo_auto - eps, hi_auto + eps


def _curve(x, rule):
    if rule == "dng":
        return -np.log(x + EPS32)
    if rule == "fsgs":
        return 1 / x + 1e-10
    return x


def normalise_numpy(x, rule):
    """x float32 [H,W] -> (v float64 [H,W] in [0, 1], lo, hi)"""
    with np.errstate(all="ignore"):
        lo, hi = percentile_bounds_numpy(x, 1e-10 if rule == "fsgs" else EPS32)
        value, clo, chi = _curve(x, rule), _curve(lo, rule), _curve(hi, rule)
        v = np.nan_to_num(np.clip((value - np.minimum(clo, chi)) / np.abs(chi - clo), 0, 1))
    return v, lo, hi


def table_index(v):
    """matplotlib's Colormap.__call__ on floats in [0, 1]: v * N truncated, N itself -> N - 1"""
    xa = np.array(v, dtype=np.float64) * 256
    xa[xa == 256] = 255
    return xa.astype(np.int64)


def composite_numpy(depth, alpha):
    d = torch.from_numpy(depth)
    return ((d - d.min()) / (d.max() - d.min()) + 1 * (1 - torch.from_numpy(alpha))).numpy()   # render.py:121


def colour_depth_numpy(depth, alpha=None, rule="dng"):
    """float32 numpy [H,W] -> (uint8 [H,W,3] R, G, B, lo, hi)"""
    x = np.ascontiguousarray(depth, dtype=np.float32)
    if x.size == 0:
        return np.zeros(x.shape + (3,), dtype=np.uint8), np.float64("nan"), np.float64("nan")
    if alpha is not None:
        x = composite_numpy(x, np.ascontiguousarray(alpha, dtype=np.float32))
    v, lo, hi = normalise_numpy(x, rule)
    return byte_tables()[_BYTE_RULE[rule]][table_index(v)], lo, hi


# --------------------------------------------------------------------------------------------------------------- device
def _lut_on(device, rule):
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, _BYTE_RULE[rule])
    if key not in _device_luts:
        _device_luts[key] = torch.from_numpy(byte_tables()[_BYTE_RULE[rule]].copy()).to(device)
    return _device_luts[key]


def _device_call(d, a, rule, want_composite, want_bounds):
    from ._lib import hip_api, stream_of
    api = hip_api()
    H, W = int(d.shape[0]), int(d.shape[1])
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=d.device)
    grey = torch.empty((H, W, 3), dtype=torch.uint8, device=d.device) if want_composite else None
    comp = torch.empty((H, W), dtype=torch.float32, device=d.device) if want_composite else None
    bounds = torch.empty((2,), dtype=torch.float64, device=d.device) if want_bounds else None
    nb = int(api.raw("depth_vis_tmp_bytes")(H, W))
    tmp = torch.empty((nb,), dtype=torch.uint8, device=d.device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    api.call("depth_vis", d.data_ptr(), ptr(a), H, W, RULES[rule], _lut_on(d.device, rule).data_ptr(), tmp.data_ptr(), nb,
             out.data_ptr(), ptr(grey), ptr(comp), ptr(bounds), stream_of(d))
    return out, grey, comp, bounds


def colour_depth(depth, alpha=None, rule="dng", return_bounds=False):
    """depth (and alpha) [H,W] or [1,H,W] float -> uint8 [H,W,3], R, G, B, on depth's device: what the reference writes as
    depth/color_%05d.png / cdepth_%05d.png ("dng", with the render's alpha) or %05d_depth.png ("fsgs").  With alpha the image
    coloured is render.py:121's composite.  return_bounds: also float64 [2] = (lo, hi) before the curve, on the same device.
    Device tensors: no host synchronisation, no read-back."""
    d, a = _check(depth, alpha, rule)
    if d.is_cuda:
        if d.numel() == 0:
            out, bounds = torch.empty(tuple(d.shape) + (3,), dtype=torch.uint8, device=d.device), None
            if return_bounds:
                bounds = torch.full((2,), float("nan"), dtype=torch.float64, device=d.device)
        else:
            out, _, _, bounds = _device_call(d, a, rule, False, return_bounds)
    else:
        rgb, lo, hi = colour_depth_numpy(d.numpy(), None if a is None else a.numpy(), rule)
        out, bounds = torch.from_numpy(np.ascontiguousarray(rgb)), torch.tensor([float(lo), float(hi)], dtype=torch.float64)
    return (out, bounds) if return_bounds else out


def composite_depth(depth, alpha):
    """-> (d float32 [H,W] = (depth - min) / (max - min) + 1 * (1 - alpha), uint8 [H,W,3] = save_image_bytes(1 - d)), on the
    inputs' device (render.py:121,124)"""
    d, a = _check(depth, alpha, "dng")
    if a is None:
        raise ValueError("composite_depth: alpha is needed")
    if d.is_cuda and d.numel():
        _, grey, comp, _ = _device_call(d, a, "dng", True, False)
        return comp, grey
    from .imageio import save_image_bytes
    comp = (d - d.min()) / (d.max() - d.min()) + 1 * (1 - a) if d.numel() else d.clone()
    return comp, save_image_bytes(1 - comp)


def colour_and_grey(depth, alpha, rule="dng"):
    """-> (colour_depth(depth, alpha, rule), composite_depth(depth, alpha)[1]): on the device both come from one call"""
    d, a = _check(depth, alpha, rule)
    if a is None:
        raise ValueError("colour_and_grey: alpha is needed")
    if d.is_cuda and d.numel():
        out, grey, _, _ = _device_call(d, a, rule, True, False)
        return out, grey
    return colour_depth(d, a, rule), composite_depth(d, a)[1]
