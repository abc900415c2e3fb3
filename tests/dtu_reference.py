"""DNGaussian/train_dtu.py's own statements restated in torch, dtype-generic - the yardstick of tests/test_dtu_cpu.py,
tests/test_gpu_dtu_kernels.py and the DTU trainer tests.

  background_mask       :84-94, the literal loop: 49 shifted in-place products along dim 1 of a [1,H,W] tensor
  background_mask_runs  the same mask stated as a run length going up each column (what the kernel computes)
  masked_mean_fill      :103-105 / :136-138: x[mask] = x[~mask].mean().detach()
  alpha_penalty         :157: (alpha[mask] ** 2).mean()
  colour_rules          :218-230 on (xyz_gradient_accum, _opacity), in place, black before white
"""
import torch


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def reset_value(opacity=0.1):
    """inverse_opacity_activation(ones * 0.1) as torch forms it in fp32: the bits the reference stores"""
    return float(inverse_sigmoid(torch.full((1,), float(opacity), dtype=torch.float32))[0])


def background_mask(gt, threshold, run=50):
    """-> (mask bool [1,H,W], gt zeroed IN PLACE, as the reference does).  `threshold` is a Python float: torch compares a
    tensor of gt's dtype against it in that dtype."""
    bg_mask = gt.max(0, keepdim=True).values < threshold
    bg_mask_clone = bg_mask.clone()
    for i in range(1, run):
        bg_mask[:, i:] *= bg_mask_clone[:, :-i]
    gt[bg_mask.repeat(3, 1, 1)] = 0.
    return bg_mask, gt


def background_mask_runs(gt, threshold, run=50):
    """the run-length statement: masked iff the run of dark pixels ending at (y,x) going up column x is >= min(y + 1, run)"""
    dark = gt.max(0).values < threshold
    H, W = dark.shape
    mask = torch.zeros((H, W), dtype=torch.bool)
    c = torch.zeros((W,), dtype=torch.int64)
    for y in range(H):
        c = torch.where(dark[y], torch.clamp(c + 1, max=run), torch.zeros_like(c))
        mask[y] = c >= min(y + 1, run)
    return mask[None]


def masked_mean_fill(x, mask):
    """out of place (x may require grad): the masked pixels take the detached mean of the others"""
    out = x.clone()
    out[mask] = x[~mask].mean().detach()
    return out


def alpha_penalty(alpha, mask):
    return (alpha[mask] ** 2).mean()


def colour_rules(colour, stat, opacity_raw, black, white, value):
    """IN PLACE on stat [P,1] and opacity_raw [P,1].  black / white = (threshold, divisor, reset) or None; value: the raw
    opacity a reset stores.  -> (rows the black rule fired on, rows the white rule fired on)"""
    nb = nw = 0
    if black is not None:
        thr, div, reset = black
        black_mask = colour.max(-1, keepdim=True).values < thr
        stat[black_mask] /= div
        if reset:
            opacity_raw[black_mask] = value
        nb = int(black_mask.sum())
    if white is not None:
        thr, div, reset = white
        white_mask = colour.min(-1, keepdim=True).values > thr
        stat[white_mask] /= div
        if reset:
            opacity_raw[white_mask] = value
        nw = int(white_mask.sum())
    return nb, nw


def ulp(v):
    """the spacing of float32 at |v| (a Python float or 0-dim tensor)"""
    t = torch.as_tensor(float(v), dtype=torch.float32).abs()
    return float(torch.nextafter(t, torch.tensor(float("inf"))) - t)
