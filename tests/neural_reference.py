"""DNGaussian's two neural heads restated in torch from their formulas (no code shared with the package):

    sigma_net  enc_x [B,32] -> 64 -> 64 -> 65, bias-free, ReLU between; column 0 = sigma, columns 1..64 = geo_feat
    color_net  [enc_d [B,16] | geo_feat] -> 64 -> 3, color = sigmoid(.) * 1.002 - 0.001

heads_ref evaluates them in float64 (the arbiter of the GPU tests), torch_chain in fp32 with the statements a user of the
encoders wrote before the fused node existed (torch.nn.functional.linear, cat, slices, sigmoid).  run() drives either through
a backward with given output gradients and returns every output and gradient tensor."""
import math

import torch
import torch.nn.functional as F

NAMES = ("w_s0", "w_s1", "w_s2", "w_c0", "w_c1")
SHAPES = ((64, 32), (64, 64), (65, 64), (64, 80), (3, 64))


def heads_ref(enc_x, enc_d, w):
    """float64 tensors -> (sigma [B], color [B,3]); enc_d None: (sigma, None)."""
    h = torch.relu(enc_x @ w[0].t())
    h = torch.relu(h @ w[1].t())
    out = h @ w[2].t()
    sigma, geo = out[:, 0], out[:, 1:]
    if enc_d is None:
        return sigma, None
    hc = torch.relu(torch.cat([enc_d, geo], dim=1) @ w[3].t())
    pre = hc @ w[4].t()
    return sigma, 1.002 / (1.0 + torch.exp(-pre)) - 0.001


def torch_chain(enc_x, enc_d, w):
    """The fp32 statements of tests/test_gpu_encoding.py's neural chain, on given weights."""
    x = enc_x
    for l in range(3):
        x = F.linear(x, w[l])
        if l != 2:
            x = F.relu(x)
    sigma, geo = x[:, 0], x[:, 1:]
    if enc_d is None:
        return sigma, None
    h = F.relu(F.linear(torch.cat([enc_d, geo], dim=-1), w[3]))
    return sigma, torch.sigmoid(F.linear(h, w[4])) * (1 + 2 * 0.001) - 0.001


def make_inputs(B, seed, device="cpu"):
    """randn activations, weights uniform in +-1/sqrt(fan_in), non-zero random output gradients."""
    g = torch.Generator().manual_seed(seed)
    t = {"enc_x": torch.randn((B, 32), generator=g), "enc_d": torch.randn((B, 16), generator=g)}
    for n, s in zip(NAMES, SHAPES):
        t[n] = (torch.rand(s, generator=g) * 2 - 1) / math.sqrt(s[1])
    t["g_sigma"] = torch.randn((B,), generator=g)
    t["g_color"] = torch.randn((B, 3), generator=g)
    return {k: v.to(device) for k, v in t.items()}


def run(fn, t, dtype, g_sigma=True, g_color=True):
    """fn(enc_x, enc_d, [w]) on leaves of `dtype` made from the dict t -> dict of sigma, color, g_enc_x, g_enc_d, g_w_*."""
    leaf = {k: t[k].detach().to(dtype).requires_grad_(True) for k in ("enc_x", "enc_d") + NAMES}
    sigma, color = fn(leaf["enc_x"], leaf["enc_d"], [leaf[n] for n in NAMES])
    outs, grads = [], []
    if g_sigma:
        outs.append(sigma); grads.append(t["g_sigma"].to(dtype))
    if g_color:
        outs.append(color); grads.append(t["g_color"].to(dtype))
    torch.autograd.backward(outs, grads)
    res = {"sigma": sigma.detach(), "color": color.detach()}
    for k in ("enc_x", "enc_d") + NAMES:
        res["g_" + k] = leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])
    return res
