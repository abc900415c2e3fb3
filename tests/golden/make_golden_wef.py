"""Generates tests/golden/wef_maps.npz by IMPORTING the reference's own LGDWT-GS/utils/loss_utils.py and running it on the
CPU (the reference tree is no part of this repository, so the outputs are committed; GS_REFERENCE_ROOT names it, default as
in make_golden.py).  Arrays only.

Run:  python tests/golden/make_golden_wef.py

The module's `from pytorch_wavelets import DWTForward` is satisfied as in make_golden.py: tests/torch_loss_reference.DWTForward,
an independent F.conv2d statement of that package's published Haar step, is registered under that name while the module loads.
For every case of tests/wef_cases.FIXTURE_CASES (inputs from the case table's seeds, stored as well so that a drift of the
generator shows):
  maps32_<case>_<l2|all>, maps64_...   compute_wef_maps / compute_wef_all_subbands in float32 and on the same inputs in float64,
                                       stacked in key order [K + 1,H,W]
  grid_<case>_<l2|all>                 the bytes of make_wef_grid_image(float32 maps, keys, tile_cols=3) (Pillow), not for the
                                       NaN case (a NaN has no byte)
  grid4_<case>_all                     the same with tile_cols=4 (more keys than one row, unused tiles)
heat_in / heat_out                     make_heatmap_rgb on a ramp that leaves [0, 1] on both sides
ch_<i>_*                               charbonnier_loss (default epsilon, and 0.05) with autograd gradients to both arguments,
                                       float32 and float64"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("GS_REFERENCE_ROOT", "/root/reference/fs3dgs_benchmark")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import torch_loss_reference as tlr  # noqa: E402
import wef_cases  # noqa: E402

CH_SHAPES = ((1,), (7,), (3, 5, 7), (2, 3, 4, 5))


def charbonnier_inputs(i):
    g = torch.Generator().manual_seed(100 + i)
    shape = CH_SHAPES[i]
    pred = torch.rand(shape, generator=g)
    target = torch.rand(shape, generator=g)
    if pred.numel() >= 7:
        target.reshape(-1)[3] = pred.reshape(-1)[3]   # d = 0: the term is epsilon, the gradient 0
    return pred, target


def load_reference():
    stub = types.ModuleType("pytorch_wavelets")
    stub.DWTForward = tlr.DWTForward
    sys.modules["pytorch_wavelets"] = stub
    try:
        spec = importlib.util.spec_from_file_location("ref_lgdwt_loss_utils_wef", REF + "/LGDWT-GS/utils/loss_utils.py")
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        del sys.modules["pytorch_wavelets"]
    return m


def main():
    ref = load_reference()
    out = {}
    for c in wef_cases.FIXTURE_CASES:
        pred, gt = wef_cases.inputs(c)
        out["pred_" + c.name], out["gt_" + c.name] = pred.numpy(), gt.numpy()
        for tag, fn, keys in (("l2", ref.compute_wef_maps, wef_cases.LEVEL2_KEYS),
                              ("all", ref.compute_wef_all_subbands, wef_cases.ALL_KEYS)):
            m32 = fn(pred[None], gt[None])
            m64 = fn(pred[None].double(), gt[None].double())
            assert tuple(m32) == keys
            out["maps32_%s_%s" % (c.name, tag)] = torch.cat([m32[k][0] for k in keys]).numpy()
            out["maps64_%s_%s" % (c.name, tag)] = torch.cat([m64[k][0] for k in keys]).numpy()
            if c.kind != "nan":
                out["grid_%s_%s" % (c.name, tag)] = np.array(ref.make_wef_grid_image(m32, list(keys), 3))
                if tag == "all":
                    out["grid4_%s_all" % c.name] = np.array(ref.make_wef_grid_image(m32, list(keys), 4))
    x = torch.linspace(-0.25, 1.25, 97).reshape(1, 1, 1, 97)
    out["heat_in"], out["heat_out"] = x.numpy(), ref.make_heatmap_rgb(x).numpy()
    for i in range(len(CH_SHAPES)):
        for eps_tag, eps in (("d", None), ("e", 0.05)):
            for dt_tag, dt in (("32", torch.float32), ("64", torch.float64)):
                pred, target = (t.to(dt).requires_grad_(True) for t in charbonnier_inputs(i))
                loss = ref.charbonnier_loss(pred, target) if eps is None else ref.charbonnier_loss(pred, target, eps)
                loss.backward()
                pre = "ch_%d_%s_%s_" % (i, eps_tag, dt_tag)
                out[pre + "loss"] = loss.detach().numpy()
                out[pre + "dpred"], out[pre + "dtarget"] = pred.grad.numpy(), target.grad.numpy()
    path = os.path.join(HERE, "wef_maps.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
