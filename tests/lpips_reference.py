"""LPIPS (VGG16, version 0.1) restated in torch for the CPU, in float32 or float64: the arbiter of csrc/gs_lpips.hip's
stages.  tests/golden/lpips.npz (the reference's own lpipsPyTorch module run on the same seeded weights) pins it."""
import torch
import torch.nn.functional as F

from lpips_cases import BLOCK_CONVS, CONV_INDEX

MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


def z_score(x, dtype):
    """x [N,3,H,W] in [0, 1]; the buffers are fp32 tensors (torch.Tensor([...])), widened when the module runs in float64"""
    mean = torch.tensor(MEAN, dtype=torch.float32)[None, :, None, None].to(device=x.device, dtype=dtype)
    std = torch.tensor(STD, dtype=torch.float32)[None, :, None, None].to(device=x.device, dtype=dtype)
    return (x.to(dtype) - mean) / std


def conv3x3_relu(x, w, b):
    return F.relu(F.conv2d(x, w, b, padding=1))


def tap_features(x, vgg_sd, dtype):
    """the five tap activations of z-scored x [N,3,H,W]"""
    taps, layer = [], 0
    for blk, n in enumerate(BLOCK_CONVS):
        if blk:
            x = F.max_pool2d(x, 2, 2)
        for _ in range(n):
            i = CONV_INDEX[layer]
            x = conv3x3_relu(x, vgg_sd["features.%d.weight" % i].to(dtype), vgg_sd["features.%d.bias" % i].to(dtype))
            layer += 1
        taps.append(x)
    return taps


def distance(fx, fy, lin, dtype=torch.float64, return_terms=False):
    """one tap: fx, fy [C,H,W], lin [C] -> the mean over the pixels of sum_c lin_c (x_c / (|x| + eps) - y_c / (|y| + eps))^2"""
    fx, fy, lin = fx.to(dtype)[None], fy.to(dtype)[None], lin.reshape(1, -1, 1, 1).to(dtype)
    nx = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
    ny = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
    terms = lin * (nx - ny) ** 2
    val = terms.sum(dim=1, keepdim=True).mean((2, 3))[0, 0]
    return (val, terms) if return_terms else val


def lin_vectors(lin_sd):
    out = []
    for k in range(5):
        for key in ("lin%d.model.1.weight" % k, "%d.1.weight" % k):
            if key in lin_sd:
                out.append(lin_sd[key].reshape(-1))
                break
    return out


def lpips(render, gt, vgg_sd, lin_sd, dtype):
    """render, gt [3,H,W] fp32 in [0, 1] -> (total, [5] per-tap terms) in dtype"""
    x = z_score(torch.stack([render, gt]), dtype)
    taps = tap_features(x, vgg_sd, dtype)
    vals = torch.stack([distance(t[0], t[1], lin, dtype) for t, lin in zip(taps, lin_vectors(lin_sd))])
    return vals.sum(), vals


def transform(x, mask=None, clamp=False, quantise=False):
    """the evaluation's pixel transform in torch (gs_eval_px.h): clamp, 8-bit round trip, blend to white"""
    if clamp:
        x = x.clamp(0, 1)
    if quantise:
        x = x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).to(torch.float32).div(255.0)
    if mask is not None:
        x = x * mask + (1.0 - mask)
    return x
