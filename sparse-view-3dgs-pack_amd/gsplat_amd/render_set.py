"""The render stage's files: render.py's folders and the camera-path frames written, metrics.py / metrics_dtu.py read back and
scored on the device.

  write_render_set    <model_path>/<name>/ours_<iteration>/renders/%05d.png and gt/%05d.png (LGDWT-GS/render.py:45-46,
                      DNGaussian/render.py:122-123), and for views that carry `depth` and `alpha` DNGaussian's two grey images
                      depth/%05d.png and depth/alpha_%05d.png (render.py:121,124-125); with colour_depth=True also
                      depth/color_%05d.png, the turbo-coloured depth (render.py:127-130, gsplat_amd/depth_vis.py)
  write_path_frames   the frames of a camera path (gsplat_amd/paths.py): DNGaussian/spiral.py:99-121's render/ours_N/ with
                      %05d.png, depth_%05d.png, cdepth_%05d.png, or FSGS/render.py:55-81's video/ours_N/%05d.png; and
                      FSGS/render.py:48-51's _depth.png / _depth.npy beside a render set's files
  prune_for_path      spiral.py:104-108: the Gaussians within `near` of any path camera leave the model
  evaluate_dir        every method folder under <model_path>/<name>: the PNG pairs read back, to_tensor, first three channels,
                      scored by gs_eval_metrics (metrics.py:28-38,79-82).  With mask_dir it is metrics_dtu.py:28-46,93-95: the
                      mask resized to a quarter (size // 4), render and ground truth resized to the mask's size - PIL's
                      Image.resize restated in csrc/gs_eval_files.hip - to_tensor, the blend to white, PSNR over mask == 1.

With lpips = the LpipsWeights (gsplat_amd/lpips.py) evaluate_dir adds the LPIPS key, metrics.py:74,83-86's
lpips(render, gt, net_type='vgg'); with mask_dir it is the LPIPS of the pair blended to white (metrics_dtu.py:42-43,98).  The
renders/ and gt/ folders remain the way to compare a run of the reference image by image.  Divergences, raised or stated here:
  * no video container is written (spiral.py:123-125's ffmpeg calls, render.py:66-81's cv2.VideoWriter): neither ffmpeg nor
    cv2 is a dependency; the numbered frames are what both would encode.
  * FSGS names a render set's files by view.image_name; here they are numbered in the order given unless a frame carries
    `image_name`.
  * the DTU mask is one plane (gsplat_amd/evaluate.py): a mask file of several channels must hold equal colour channels; the
    first is used.  Files with an alpha channel cannot take the DTU leg: Pillow resizes them premultiplied, not restated here.
  * views are scored in sorted file order (the reference in os.listdir's order; the means do not depend on it).
  * results.json / per_view.json are written through io.write_results_json as it stands: one method per file, so with
    several method folders the files hold the last one in sorted order; the returned dictionary holds all of them.
  * the LPIPS key only on request (its weights are the user's files); L1 is added (evaluate.py)."""
import os

import numpy as np
import torch

from . import evaluate
from .depth_vis import colour_depth as _colour_depth
from .depth_vis import colour_and_grey
from .imageio import read_png, resize_u8, save_image_bytes, to_planar, write_png
from .io import write_results_json


def _get(view, key):
    if isinstance(view, dict):
        return view.get(key)
    return getattr(view, key, None)


def write_render_set(model_path, name, iteration, views, colour_depth=False):
    """views: an iterable of mappings (or objects) with `render` and `gt` - [C,H,W] float tensors, the ground truth's first
    three channels are written as render.py:120 takes them - and optionally `depth` and `alpha` ([1,H,W] or [H,W]).
    colour_depth: views with depth and alpha also get depth/color_%05d.png (render.py:127-130); the default writes exactly
    the files listed above.  -> the method folder.  Files are numbered in the order of `views`."""
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
                if colour_depth:
                    write_png(os.path.join(depth_path, "color_" + fname), _colour_depth(depth, alpha, rule="dng"))
    return base


PATH_LAYOUTS = ("dng_spiral", "fsgs_video")


def write_path_frames(model_path, frames, layout="dng_spiral", iteration=0, fsgs_depth=False, name="test"):
    """frames: an iterable of mappings (or objects) with `render` [3,H,W] and, per layout, `depth` and `alpha`.
      "dng_spiral"  <model_path>/render/ours_<iteration>/%05d.png (the render as it is), depth_%05d.png (save_image of 1 - d, d
                    the composite of render.py:121) and cdepth_%05d.png (d turbo-coloured): spiral.py:99-121; needs depth, alpha
      "fsgs_video"  <model_path>/video/ours_<iteration>/%05d.png, the render clamped to [0, 1]: render.py:55-77
    fsgs_depth: every frame that carries `depth` also leaves <model_path>/<name>/ours_<iteration>/renders/<stem>_depth.png
    (vis_depth's colours) and <stem>_depth.npy (the float32 depth), stem = the frame's `image_name` or its %05d number:
    render.py:48-51.  -> the layout's folder.  Tensors on the device are coloured there; only the bytes are read back."""
    if layout not in PATH_LAYOUTS:
        raise ValueError("write_path_frames: layout is one of %s (got %r)" % (PATH_LAYOUTS, layout))
    base = os.path.join(model_path, "render" if layout == "dng_spiral" else "video", "ours_{}".format(iteration))
    os.makedirs(base, exist_ok=True)
    set_path = os.path.join(model_path, name, "ours_{}".format(iteration), "renders")
    with torch.no_grad():
        for idx, frame in enumerate(frames):
            render = _get(frame, "render")
            if render is None:
                raise ValueError("write_path_frames: frame %d carries no `render`" % idx)
            fname = "{0:05d}.png".format(idx)
            depth, alpha = _get(frame, "depth"), _get(frame, "alpha")
            if layout == "dng_spiral":
                if depth is None or alpha is None:
                    raise ValueError("write_path_frames: frame %d carries no `depth` / `alpha` (layout 'dng_spiral')" % idx)
                write_png(os.path.join(base, fname), save_image_bytes(render))
                colour, grey = colour_and_grey(depth, alpha, rule="dng")
                write_png(os.path.join(base, "depth_" + fname), grey)
                write_png(os.path.join(base, "cdepth_" + fname), colour)
            else:
                write_png(os.path.join(base, fname), save_image_bytes(torch.clamp(render, min=0., max=1.)))
            if fsgs_depth and depth is not None:
                os.makedirs(set_path, exist_ok=True)
                stem = _get(frame, "image_name") or "{0:05d}".format(idx)
                plane = depth[0] if depth.dim() == 3 else depth
                write_png(os.path.join(set_path, stem + "_depth.png"), _colour_depth(plane, rule="fsgs"))
                np.save(os.path.join(set_path, stem + "_depth.npy"), plane.detach().cpu().numpy())
    return base


def prune_for_path(model, centres, near):
    """spiral.py:104-108 (render.py:110-115 with --near): remove the Gaussians closer than `near` to any of the path's camera
    centres [K,3] (paths.path_centres).  The mask is dng_reg.near_camera_mask on a device model, the same norm test in torch on
    a CPU one; the rows leave through the model's prune_points.  -> the bool mask [P] of the rows removed."""
    xyz = model.get_xyz.detach()
    centres = torch.as_tensor(centres, dtype=torch.float32).reshape(-1, 3).to(xyz.device)
    if xyz.is_cuda:
        from .dng_reg import near_camera_mask
        mask = near_camera_mask(xyz, centres, float(near))
    else:
        mask = torch.zeros((xyz.shape[0],), dtype=torch.bool)
        for c in centres:
            mask |= (xyz - c[None].repeat(xyz.shape[0], 1)).norm(dim=1) < near
    model.prune_points(mask)
    return mask


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


def evaluate_dir(model_path, name="test", mask_dir=None, ssim_sk=False, device="cuda", lpips=None):
    """-> {method: Evaluator.result(names)} for every method folder (ours_<iteration>) under <model_path>/<name>, and
    results.json / per_view.json under model_path.  One read-back per method folder.  All views of a method share one size.
    lpips: the LpipsWeights; results.json and per_view.json then carry the LPIPS key."""
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
                ev = evaluate.Evaluator(len(names), r.shape[0], r.shape[1], r.shape[2], device, ssim_sk=ssim_sk, lpips=lpips)
            ev.add(i, r, g, mask=mask)   # (the files' values are bytes / 255 already: no clamp, no second quantisation)
        out[method] = ev.result(names)
        write_results_json(model_path, method, out[method])
    if not out:
        raise ValueError("evaluate_dir: no method folder with renders/ under %s" % test_dir)
    return out
