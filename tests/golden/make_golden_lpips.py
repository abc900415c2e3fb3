"""Generates tests/golden/lpips.npz by IMPORTING the reference's own lpipsPyTorch package (LGDWT-GS/lpipsPyTorch) and running
its LPIPS('vgg') on the CPU in float32 and in float64 (the reference tree is no part of this repository, so the outputs are
committed; GS_REFERENCE_ROOT names it).  Fixtures are data only: the uint8 images, the seeds, the results.  No weights are
stored (59 MB): tests/lpips_cases.make_state_dicts regenerates them from the seed.

What the package needs and this machine lacks is supplied, not fetched:
  * torchvision is not installed: a stand-in module whose models.vgg16(...).features is an nn.Sequential in torchvision's
    layout (the thirteen convolutions at their indices, ReLU, MaxPool2d(2, 2)) filled from the seeded weights;
  * get_state_dict (a download on every call) is replaced by the seeded lin weights under its renamed keys;
  * torch.hub.load_state_dict_from_url raises, so nothing can reach the network.
The per-tap terms are read with forward hooks on the package's own lin layers (their output's mean over the pixels).

  python tests/golden/make_golden_lpips.py"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("GS_REFERENCE_ROOT", "/root/reference/fs3dgs_benchmark")

import lpips_cases as cases  # noqa: E402


def _no_network(*a, **k):
    raise RuntimeError("make_golden_lpips: nothing is fetched")


def install_stand_ins(vgg_sd, lin_sd_renamed):
    torch.hub.load_state_dict_from_url = _no_network

    def vgg16(*a, **k):
        cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
        layers, cin = [], 3
        for v in cfg:
            if v == "M":
                layers.append(nn.MaxPool2d(2, 2))
            else:
                layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        net = nn.Module()
        net.features = nn.Sequential(*layers)
        net.load_state_dict(vgg_sd)
        return net

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = vgg16
    tv.models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
    sys.path.insert(0, os.path.join(REF, "LGDWT-GS"))
    import lpipsPyTorch.modules.lpips as ref_lpips
    ref_lpips.get_state_dict = lambda *a, **k: lin_sd_renamed
    return ref_lpips


def run(crit, render, gt, dtype):
    taps, hooks = [], []
    for layer in crit.lin:
        hooks.append(layer.register_forward_hook(lambda m, i, o: taps.append(float(o.mean((2, 3)).reshape(())))))
    with torch.no_grad():
        val = crit(render[None].to(dtype), gt[None].to(dtype))
    for h in hooks:
        h.remove()
    assert tuple(val.shape) == (1, 1, 1, 1) and len(taps) == 5
    return float(val.reshape(())), taps


def main():
    vgg_sd, _ = cases.make_state_dicts()
    _, lin_renamed = cases.make_state_dicts(renamed=True)
    ref_lpips = install_stand_ins(vgg_sd, lin_renamed)
    crit32 = ref_lpips.LPIPS("vgg").eval()
    crit64 = ref_lpips.LPIPS("vgg").double().eval()
    out = {"weight_seed": np.int64(cases.WEIGHT_SEED), "names": np.array([c[0] for c in cases.WHOLE_CASES])}
    for name, H, W, seed in cases.WHOLE_CASES:
        r8, g8 = cases.whole_images(H, W, seed)
        render, gt = cases.planar(r8), cases.planar(g8)
        v32, t32 = run(crit32, render, gt, torch.float32)
        v64, t64 = run(crit64, render, gt, torch.float64)
        rel = abs(v32 - v64) / abs(v64)
        print("%-10s lpips f64 %.12g  f32 %.9g  rel %.3g  taps %s" % (name, v64, v32, rel, ["%.3g" % t for t in t64]))
        out[name + "/render_u8"], out[name + "/gt_u8"] = r8, g8
        out[name + "/seed"] = np.int64(seed)
        out[name + "/lpips_f64"], out[name + "/lpips_f32"] = np.float64(v64), np.float32(v32)
        out[name + "/taps_f64"], out[name + "/taps_f32"] = np.array(t64, dtype=np.float64), np.array(t32, dtype=np.float32)
        out[name + "/rel_f32_f64"] = np.float64(rel)
    np.savez_compressed(os.path.join(HERE, "lpips.npz"), **out)


if __name__ == "__main__":
    main()
