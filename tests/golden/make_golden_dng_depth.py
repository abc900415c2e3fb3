"""Generator of tests/golden/dng_depth.npz (run by hand, never by the suite):

    python tests/golden/make_golden_dng_depth.py /path/to/DNGaussian/utils/loss_utils.py

It loads DNGaussian's own loss_utils.py from the given path and EXECUTES its patch_norm_{mse,l1}_loss[_global] and
loss_depth_smoothness in float64 on a seeded depth / target pair.  Only arrays are kept: the inputs (float32), and per
case the loss, the mask, the input gradient, for some the normalised difference d - nothing of the reference's text.

The image is 64 x 80 so that the file stays well inside the committed-file limit with float64 gradients.  Patch sizes
5 (remainder in H only), 8 (divides both) and 17 (remainder in both); margins 0.00025, 0.01, 0.2 rotated over the
(patch size, loss) grid so that every patch size and every loss meets every margin; one empty-mask case."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dng_depth_reference as restatement  # noqa: E402  (the seeded scene only)

H, W = 64, 80
PATCHES = (5, 8, 17)
MARGINS = (0.00025, 0.01, 0.2)
LOSSES = ("mse", "mse_global", "l1", "l1_global")
REF_NAME = {"mse": "patch_norm_mse_loss", "mse_global": "patch_norm_mse_loss_global", "l1": "patch_norm_l1_loss",
            "l1_global": "patch_norm_l1_loss_global"}


def main():
    spec = importlib.util.spec_from_file_location("dng_loss_utils", sys.argv[1])
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    depth, mono = restatement.scene(H, W, seed=11)
    out = {"depth": depth.float().numpy(), "mono": mono.float().numpy()}
    cases = []

    def run(name, p, margin):
        x = depth.clone().requires_grad_(True)
        loss, mask = getattr(ref, REF_NAME[name])(x, mono, p, margin, return_mask=True)
        loss.backward()
        return loss.detach(), mask, x.grad

    for i, p in enumerate(PATCHES):
        for j, name in enumerate(LOSSES):
            margin = MARGINS[(i + j) % 3]
            loss, mask, grad = run(name, p, margin)
            k = "c%02d" % len(cases)
            cases.append({"key": k, "loss": name, "p": p, "margin": margin})
            out[k + "_loss"] = loss.numpy()
            out[k + "_mask"] = mask.numpy()
            out[k + "_grad"] = grad.numpy()
            assert 0 < int(mask.sum()) < mask.numel() or margin < 1e-3, (name, p, margin, int(mask.sum()))
        # the normalised difference itself, one form per patch size (what the mask thresholds)
        glob = i % 2 == 1
        std = {"std": depth.std().detach()} if glob else {}
        stdt = {"std": mono.std().detach()} if glob else {}
        d = ref.normalize(ref.patchify(depth, p), **std) - ref.normalize(ref.patchify(mono, p), **stdt)
        out["d_p%d_%s" % (p, "global" if glob else "local")] = d.numpy()
    # the empty mask: NaN loss, zero gradient
    loss, mask, grad = run("mse", 8, 1e9)
    assert not bool(mask.any()) and bool(torch.isnan(loss)) and float(grad.abs().max()) == 0.0
    cases.append({"key": "empty", "loss": "mse", "p": 8, "margin": 1e9})
    out["empty_loss"], out["empty_mask"], out["empty_grad"] = loss.numpy(), mask.numpy(), grad.numpy()
    # smoothness, guided by the target as the training scripts do, and by a 3-channel image
    g = torch.Generator().manual_seed(12)
    rgb = torch.rand((1, 3, H, W), generator=g, dtype=torch.float64).float().double()
    out["rgb"] = rgb.float().numpy()
    for tag, img in (("smooth_mono", mono), ("smooth_rgb", rgb)):
        x = depth.clone().requires_grad_(True)
        loss = ref.loss_depth_smoothness(x, img)
        loss.backward()
        out[tag + "_loss"], out[tag + "_grad"] = loss.detach().numpy(), x.grad.numpy()
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "dng_depth.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
