"""Float64 restatement of the test-set metrics of gsplat_amd.evaluate (csrc/gs_eval.hip): the arbiter of the GPU tests.

The three pixel transforms run on the float32 inputs in float32 torch operations, each a single rounding, exactly as the
reference's pipeline applies them (save_image / to_tensor work on float32 tensors, metrics_dtu.py blends float32 tensors):
  clamp      x.clamp(0, 1)
  quantise   x.mul(255).add(0.5).clamp(0, 255).to(uint8)  ->  q.to(float32).div(255)
  mask       x * m + (1 - m)
The transformed images are then promoted and the four metrics evaluated in float64:
  mse / psnr  mean (a - b)^2 over all elements, or over those with m == 1 under the mask; 20 log10(1 / sqrt(mse))
  ssim        the 11-tap sigma-1.5 window built as the reference builds it (float32 exp / sum, float32 outer product), promoted;
              zero padding; mean of the map
  l1          mean |a - b|
"""
from math import exp

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def to_bytes(x):
    """torchvision.utils.save_image's bytes of a float32 tensor"""
    return x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


def transform(x, mask=None, clamp=False, quantise=False):
    """float32 [C,H,W] -> float32, as the metrics see it"""
    assert x.dtype == torch.float32
    if clamp:
        x = x.clamp(0, 1)
    if quantise:
        x = to_bytes(x).to(torch.float32).div(255)
    if mask is not None:
        m = mask.to(torch.float32)[None]
        x = x * m + (1 - m)
    return x


def window64(channels, size=11, sigma=1.5):
    g = torch.Tensor([exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)])
    g = (g / g.sum()).unsqueeze(1)
    w = g.mm(g.t()).float()[None, None]
    return w.expand(channels, 1, size, size).contiguous().double()


def ssim_map(a, b):
    """float64 [1,C,H,W] pair -> the SSIM map"""
    ch = a.shape[1]
    w = window64(ch)
    conv = lambda t: F.conv2d(t, w, padding=5, groups=ch)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    s1 = conv(a * a) - mu1 * mu1
    s2 = conv(b * b) - mu2 * mu2
    s12 = conv(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def metrics(render, gt, mask=None, clamp=False, quantise=False):
    """float32 CPU [C,H,W] images (mask [H,W] float32 or None) -> dict of python floats: mse, psnr, ssim, l1, count"""
    render, gt = render.detach().cpu(), gt.detach().cpu()
    mask = None if mask is None else mask.detach().cpu()
    a = transform(render, mask, clamp, quantise).double()
    b = transform(gt, mask, clamp, quantise).double()
    d = a - b
    if mask is None:
        sel = d.reshape(-1)
    else:
        sel = d[(mask == 1.0)[None].expand_as(d)]
    count = sel.numel()
    mse = (sel * sel).mean() if count else torch.tensor(float("nan"), dtype=torch.float64)
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    return {"mse": float(mse), "psnr": float(psnr), "ssim": float(ssim_map(a[None], b[None]).mean()),
            "l1": float(d.abs().mean()), "count": float(count)}


def seeded_pair(C, H, W, seed, spread=0.0):
    """A float32 render / ground-truth pair: the ground truth uniform in [0, 1], the render that plus noise; spread > 0
    stretches both beyond [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand((C, H, W), generator=g)
    render = gt + 0.1 * torch.randn((C, H, W), generator=g)
    if spread:
        gt = gt * (1 + 2 * spread) - spread
        render = render * (1 + 2 * spread) - spread
    return render.float().contiguous(), gt.float().contiguous()


def seeded_mask(H, W, seed):
    """A grey DTU-like mask: 1 inside a disc, 0 outside, a rim of byte-valued greys k / 255 between."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    r = torch.sqrt(((y - H / 2) / max(H, 1)) ** 2 + ((x - W / 2) / max(W, 1)) ** 2)
    m = ((0.38 - r) * 12).clamp(0, 1)
    m = (m * 255).round() / 255
    flip = torch.rand((H, W), generator=g) < 0.05
    return torch.where(flip, 1 - m, m).float().contiguous()
