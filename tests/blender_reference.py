"""DNGaussian/train_blender.py's own statements restated in torch, dtype-generic - the yardstick of tests/test_blender_cpu.py,
tests/test_gpu_blender_kernels.py and the Blender trainer tests.

  background_mask   :87 / :286: gt.min(0, keepdim=True).values > threshold
  depth_target      :96-97 / :295-296: depth_mono = 255.0 - depth_mono; depth_mono[bg_mask] = 0
  white_rule        :208-211 / :367-370 on (xyz_gradient_accum, _opacity), in place
  eval_sh           utils/sh_utils.py:59-116, degrees 0..3
  sh_colour         gaussian_renderer/__init__.py:351-355: the "color" of render_sh's package
  white_rule_sh     :366-370: the rule on that colour
and their float64 twins: new_opacity64 (the opacity formula on the fp32 rows, evaluated in float64) and sh_colour64.
"""
import numpy as np
import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def background_mask(gt, threshold=254 / 255):
    """-> mask bool [1,H,W].  `threshold` is a Python float: torch compares a tensor of gt's dtype against it in that dtype."""
    return gt.min(0, keepdim=True).values > threshold


def depth_target(mono, bg_mask):
    """mono as stored, in any shape with the mask's element count -> 255.0 - mono with the masked pixels 0"""
    depth_mono = 255.0 - mono
    depth_mono[bg_mask.reshape(depth_mono.shape)] = 0
    return depth_mono


def white_rule(colour, stat, opacity_raw, threshold=253 / 255, factor=0.1):
    """IN PLACE on stat [P,1] and opacity_raw [P,1] -> the rows that fired"""
    white_mask = colour.min(-1, keepdim=True).values > threshold
    stat[white_mask] = 0
    opacity_raw[white_mask] = inverse_sigmoid(torch.sigmoid(opacity_raw[white_mask]) * factor)
    return int(white_mask.sum())


def target_elementwise(gt, mono, threshold=254 / 255):
    """what gs_blender_target states per pixel, without an index: -> (mask bool [1,H,W], count, target in mono's shape)"""
    thr = torch.tensor(threshold, dtype=gt.dtype)
    nan = gt.isnan().any(0)
    mn = torch.minimum(torch.minimum(gt[0], gt[1]), gt[2])
    mask = (~nan) & (mn > thr)
    target = torch.where(mask.reshape(mono.shape), torch.zeros_like(mono), 255.0 - mono)
    return mask[None], int(mask.sum()), target


def white_rule_elementwise(colour, stat, opacity_raw, threshold=253 / 255, factor=0.1):
    """what gs_dng_white_rule states per row, out of place, the opacity in the rows' own dtype -> (fires bool [P], stat, opacity)"""
    thr = torch.tensor(threshold, dtype=colour.dtype)
    fires = (~colour.isnan().any(-1)) & (colour.min(-1).values > thr)
    f = fires.reshape(stat.shape)
    new = inverse_sigmoid(torch.sigmoid(opacity_raw) * factor)
    return fires, torch.where(f, torch.zeros_like(stat), stat), torch.where(f, new, opacity_raw)


def new_opacity64(opacity_raw, factor=0.1):
    """the formula on fp32 rows evaluated in float64 -> float64.  fp32 torch multiplies by float32(factor) (a Python scalar takes
    the tensor's dtype), so that is the factor here too: 0.1 and float32(0.1) differ by 1.5e-9 relative, which moves the result
    by 1.7e-9 - under a hundredth of the fp32 spacing of a result that is never above log(0.1 / 0.9) = -2.197."""
    f = float(np.float32(factor))
    return inverse_sigmoid(torch.sigmoid(opacity_raw.double()) * f)


def eval_sh(deg, sh, dirs):
    """sh [..., C, (max_deg + 1)^2], dirs [..., 3] -> [..., C]"""
    assert 0 <= deg <= 3
    assert sh.shape[-1] >= (deg + 1) ** 2
    result = C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        result = (result - C1 * y * sh[..., 1] + C1 * z * sh[..., 2] - C1 * x * sh[..., 3])
        if deg > 1:
            xx, yy, zz = x * x, y * y, z * z
            xy, yz, xz = x * y, y * z, x * z
            result = (result + C2[0] * xy * sh[..., 4] + C2[1] * yz * sh[..., 5] + C2[2] * (2.0 * zz - xx - yy) * sh[..., 6] +
                      C2[3] * xz * sh[..., 7] + C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                result = (result + C3[0] * y * (3 * xx - yy) * sh[..., 9] + C3[1] * xy * z * sh[..., 10] +
                          C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12] +
                          C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + C3[5] * z * (xx - yy) * sh[..., 14] +
                          C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return result


def sh_colour(xyz, features, active_sh_degree, campos):
    """features [P,M,3] (get_features) -> colour [P,3], in the inputs' dtype"""
    P, M = features.shape[0], features.shape[1]
    shs_view = features.transpose(1, 2).reshape(-1, 3, M)
    dir_pp = xyz - campos.reshape(1, 3).repeat(P, 1)
    dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
    sh2rgb = eval_sh(active_sh_degree, shs_view, dir_pp_normalized)
    return torch.clamp_min(sh2rgb + 0.5, 0.0)


def sh_colour64(xyz, features, active_sh_degree, campos):
    """the float64 twin: the fp32 inputs widened, every operation in float64"""
    return sh_colour(xyz.double(), features.double(), active_sh_degree, campos.double())


def white_rule_sh(xyz, features, active_sh_degree, campos, stat, opacity_raw, threshold=253 / 255, factor=0.1):
    """-> (rows that fired, colour)"""
    colour = sh_colour(xyz, features, active_sh_degree, campos)
    return white_rule(colour, stat, opacity_raw, threshold, factor), colour


def ulp(v):
    """the spacing of float32 at |v| (a Python float or 0-dim tensor)"""
    t = torch.as_tensor(float(v), dtype=torch.float32).abs()
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)


def spacing(t):
    """float32 spacing at |t| per element (any float tensor in, float64 out); the spacing at 0 is the smallest denormal"""
    a = t.abs().float()
    up = torch.nextafter(a, torch.full_like(a, float("inf")))
    return up.double() - a.double()
