"""The evaluation's files: render.py's folders written, metrics.py / metrics_dtu.py read back and scored on the device.

  write_render_set    <model_path>/<name>/ours_<iteration>/renders/%05d.png and gt/%05d.png (LGDWT-GS/render.py:45-46,
                      DNGaussian/render.py:122-123), and for views that carry `depth` and `alpha` DNGaussian's two grey images
                      depth/%05d.png and depth/alpha_%05d.png (render.py:121,124-125)
  evaluate_dir        every method folder under <model_path>/<name>: the PNG pairs read back, to_tensor, first three channels,
                      scored by gs_eval_metrics (metrics.py:28-38,79-82).  With mask_dir it is metrics_dtu.py:28-46,93-95: the
                      mask resized to a quarter (size // 4), render and ground truth resized to the mask's size - PIL's
                      Image.resize restated in csrc/gs_eval_files.hip - to_tensor, the blend to white, PSNR over mask == 1.

The renders/ and gt/ folders are also the hand-off to LPIPS, which this package does not compute, and the way to compare a
run of the reference image by image.  Divergences, raised or stated here:
  * depth/color_%05d.png, the turbo-coloured depth, is not written: it needs matplotlib's colour table.
  * the DTU mask is one plane (gsplat_amd/evaluate.py): a mask file of several channels must hold equal colour channels; the
    first is used.  Files with an alpha channel cannot take the DTU leg: Pillow resizes them premultiplied, not restated here.
  * views are scored in sorted file order (the reference in os.listdir's order; the means do not depend on it).
  * results.json / per_view.json are written through io.write_results_json as it stands: one method per file, so with
    several method folders the files hold the last one in sorted order; the returned dictionary holds all of them.
  * no LPIPS key; L1 is added (evaluate.py)."""
import os

import numpy as np
import torch

from . import evaluate
from .imageio import read_png, resize_u8, save_image_bytes, to_planar, write_png
from .io import write_results_json


def _get(view, key):
    if isinstance(view, dict):
        return view.get(key)
    return getattr(view, key, None)


def write_render_set(model_path, name, iteration, views):
    """views: an iterable of mappings (or objects) with `render` and `gt` - [C,H,W] float tensors, the ground truth's first
    three channels are written as render.py:120 takes them - and optionally `depth` and `alpha` ([1,H,W] or [H,W]).
    -> the method folder.  Files are numbered in the order of `views`."""
    base = os.path.join(model_path, name, "ours_{}".format(iteration))
    render_path, gts_path, depth_path = (os.path.join(base, d) for d in ("renders", "gt", "depth"))
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    with torch.no_grad():
        for idx, view in enumerate(views):
            render, gt = _get(view, "render"), _get(view, "gt")
            if render is None or gt is None:
                raise ValueError("write_render_set: view %d carries no `render` / `gt`" % idx)
            fname = "{0:05d}.png".format(idx)
            write_png(os.path.join(render_path, fname), save_image_bytes(render))
            write_png(os.path.join(gts_path, fname), save_image_bytes(gt[0:3] if gt.dim() == 3 else gt))
            depth, alpha = _get(view, "depth"), _get(view, "alpha")
            if depth is not None and alpha is not None:
                os.makedirs(depth_path, exist_ok=True)
                d = (depth - depth.min()) / (depth.max() - depth.min()) + 1 * (1 - alpha)   # render.py:121
                write_png(os.path.join(depth_path, fname), save_image_bytes(1 - d))
                write_png(os.path.join(depth_path, "alpha_" + fname), save_image_bytes(alpha))
    return base


def _planar(u8, fname, device):
    """to_tensor(file)[:3] on the device: uint8 [H,W,C] on the host -> fp32 [min(C, 3),H,W] = byte / 255"""
    if u8.shape[2] == 2:
        raise ValueError("evaluate_dir: %s is grey + alpha - grey, RGB and RGBA files only" % fname)
    return to_planar(torch.from_numpy(np.ascontiguousarray(u8[:, :, :3])).to(device))


def _mask_plane(path):
    m = read_png(path)
    if m.shape[2] in (2, 4):
        raise ValueError("evaluate_dir: mask %s has an alpha channel - Pillow resizes such files premultiplied, which is not "
                         "restated here" % path)
    if m.shape[2] == 3 and not (np.array_equal(m[:, :, 0], m[:, :, 1]) and np.array_equal(m[:, :, 0], m[:, :, 2])):
        raise ValueError("evaluate_dir: mask %s is not grey - the DTU mask is one plane here" % path)
    return np.ascontiguousarray(m[:, :, :1])


def evaluate_dir(model_path, name="test", mask_dir=None, ssim_sk=False, device="cuda"):
    """-> {method: Evaluator.result(names)} for every method folder (ours_<iteration>) under <model_path>/<name>, and
    results.json / per_view.json under model_path.  One read-back per method folder.  All views of a method share one size."""
    device = torch.device(device)
    test_dir = os.path.join(model_path, name)
    out = {}
    for method in sorted(os.listdir(test_dir)):
        method_dir = os.path.join(test_dir, method)
        renders_dir, gt_dir = os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt")
        if not os.path.isdir(renders_dir):
            continue
        names = sorted(f for f in os.listdir(renders_dir) if f.lower().endswith(".png"))
        if not names:
            raise ValueError("evaluate_dir: no PNG files under %s" % renders_dir)
        ev = None
        for i, fname in enumerate(names):
            render, gt = read_png(os.path.join(renders_dir, fname)), read_png(os.path.join(gt_dir, fname))
            mask = None
            if mask_dir is None:
                r, g = _planar(render, fname, device), _planar(gt, fname, device)
            else:
                if render.shape[2] in (2, 4) or gt.shape[2] in (2, 4):
                    raise ValueError("evaluate_dir: %s has an alpha channel - Pillow resizes such files premultiplied, which "
                                     "is not restated here" % fname)
                m8 = torch.from_numpy(_mask_plane(os.path.join(mask_dir, fname))).to(device)
                size = (m8.shape[1] // 4, m8.shape[0] // 4)   # PIL's (width, height)
                mask = resize_u8(m8, size, return_planar=True)[1][0]
                r = resize_u8(torch.from_numpy(render).to(device), size, return_planar=True)[1]
                g = resize_u8(torch.from_numpy(gt).to(device), size, return_planar=True)[1]
            if r.shape != g.shape:
                raise ValueError("evaluate_dir: %s: render %s and gt %s differ in shape" % (fname, tuple(r.shape), tuple(g.shape)))
            if ev is None:
                ev = evaluate.Evaluator(len(names), r.shape[0], r.shape[1], r.shape[2], device, ssim_sk=ssim_sk)
            ev.add(i, r, g, mask=mask)   # (the files' values are bytes / 255 already: no clamp, no second quantisation)
        out[method] = ev.result(names)
        write_results_json(model_path, method, out[method])
    if not out:
        raise ValueError("evaluate_dir: no method folder with renders/ under %s" % test_dir)
    return out
