"""Generator of tests/golden/camera_paths.npz and tests/golden/depth_vis.npz (run by hand, never by the suite):

    python tests/golden/make_golden_paths.py /path/to/fs3dgs_benchmark

It EXECUTES the reference's own functions on the CPU and keeps arrays only - inputs, poses, bounds, normalised images, bytes:
  FSGS/utils/pose_utils.py (with its utils.stepfun import)   generate_spiral_path, generate_ellipse_path,
                                                             generate_random_poses_llff, generate_random_poses_360
  DNGaussian/utils/pose_utils.py                             recenter / backcenter / the two spirals / convert_poses
  DNGaussian/scene/dataset_readers.py                        CreateLLFFSpiral, CreateDTUSpiral, generateLLFFCameras: the three
                                                             definitions are pulled out with `ast` when this runs (the module
                                                             imports the whole scene stack) and executed on a temporary
                                                             poses_bounds.npy; none of their text is kept
  FSGS/utils/general_utils.py                                vis_depth, weighted_percentile
  DNGaussian/render.py                                       weighted_percentile, visualize_cmap, depth_curve_fn - pulled out
                                                             with `ast` too (the script imports torchvision)
Modules the reference imports but these functions never call (cv2, imageio, skimage) are replaced by empty stand-ins.
matplotlib 3.10 has no cm.get_cmap: visualize_cmap is handed matplotlib.colormaps["turbo"], vis_depth's module a `cm` whose
get_cmap returns it.  The composite in front of DNGaussian's colouring (render.py:121) and save_image's byte rule behind it
are the stated torch operations (torchvision is absent): mul(255).add_(0.5).clamp_(0, 255) on the float64 image, truncated."""
import ast
import importlib.util
import os
import sys
import tempfile
import types

import matplotlib
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import depth_vis_cases  # noqa: E402


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pull(path, names, ns):
    """Execute the named top-level definitions / assignments of a file in ns"""
    tree = ast.parse(open(path).read())
    keep = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            keep.append(node)
        elif isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in node.targets):
            keep.append(node)
    assert {getattr(n, "name", None) or n.targets[0].id for n in keep} == set(names), names
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


# ------------------------------------------------------------------------------------------------------- inputs
def seeded_views(n, seed):
    """n cameras on an arc around the origin, looking near it: R (camera-to-world, as the reference stores it), T, bounds"""
    rng = np.random.RandomState(seed)
    Rs, Ts, bounds = [], [], []
    for i in range(n):
        az = 0.5 * (i - (n - 1) / 2) + 0.05 * rng.randn()
        eye = np.array([4.0 * np.sin(az), 0.4 * rng.randn(), -4.0 * np.cos(az)]) + 0.1 * rng.randn(3)
        fwd = 0.2 * rng.randn(3) - eye
        fwd /= np.linalg.norm(fwd)
        right = np.cross(np.array([0.0, -1.0, 0.0]) + 0.05 * rng.randn(3), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        c2w = np.stack([right, down, fwd], axis=1)
        Rs.append(c2w)
        Ts.append(-c2w.T @ eye)
        bounds.append(np.array([2.0 + rng.rand(), 9.0 + 3 * rng.rand()]))
    return np.stack(Rs), np.stack(Ts), np.stack(bounds)


def seeded_poses_bounds(n, seed):
    """[n,17] in the LLFF file layout: 3 x 5 (columns -y, x, z, position, hwf) and two depth bounds"""
    R, T, bounds = seeded_views(n, seed)
    rows = []
    for i in range(n):
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = R[i], -R[i] @ T[i]
        m = np.concatenate([c2w[:3, 1:2], c2w[:3, 0:1], -c2w[:3, 2:3], c2w[:3, 3:4], np.array([[378.0], [504.0], [420.0]])], 1)
        rows.append(np.concatenate([m.ravel(), bounds[i]]))
    return np.stack(rows)


def gen_paths(ref):
    for name in ("cv2", "imageio", "skimage", "skimage.transform"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, os.path.join(ref, "FSGS"))
    import utils.pose_utils as fsgs   # (its `from utils.stepfun import sample_np` resolves beside it)
    dng = load(os.path.join(ref, "DNGaussian", "utils", "pose_utils.py"), "ref_dng_pose_utils")
    graphics = load(os.path.join(ref, "DNGaussian", "utils", "graphics_utils.py"), "ref_dng_graphics_utils")
    captured = {}
    ns = dict(np=np, os=os, sys=types.SimpleNamespace(stdout=types.SimpleNamespace(write=lambda s: None, flush=lambda: None)),
              pose_utils=dng, focal2fov=graphics.focal2fov,
              CameraInfo=lambda **kw: types.SimpleNamespace(**kw), getNerfppNorm=lambda cams: None,
              SceneInfo=lambda **kw: captured.update(kw) or kw)
    pull(os.path.join(ref, "DNGaussian", "scene", "dataset_readers.py"), ("generateLLFFCameras", "CreateLLFFSpiral", "CreateDTUSpiral"), ns)
    out = {}
    for n in (3, 5):
        R, T, bounds = seeded_views(n, 40 + n)
        pb = seeded_poses_bounds(n, 50 + n)
        out["views%d_R" % n], out["views%d_T" % n], out["views%d_bounds" % n], out["pb%d" % n] = R, T, bounds, pb
        views = [types.SimpleNamespace(R=R[i].copy(), T=T[i].copy(), bounds=bounds[i].copy()) for i in range(n)]
        for nf in (4, 7):
            out["spiral_%d_%d" % (n, nf)] = fsgs.generate_spiral_path(pb.copy(), n_frames=nf)
            out["ellipse_%d_%d" % (n, nf)] = np.stack(fsgs.generate_ellipse_path(views, n_frames=nf))
            out["ellipse_z_%d_%d" % (n, nf)] = np.stack(fsgs.generate_ellipse_path(views, n_frames=nf, const_speed=False,
                                                                                   z_variation=0.3, z_phase=0.25))
            poses = pb[:, :-2].reshape([-1, 3, 5])[:, :3, :4] @ np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]],
                                                                         dtype=np.float32)
            rec = dng.recenter_poses(poses)
            out["dng_recenter_%d" % n] = rec
            out["dng_spiral_%d_%d" % (n, nf)] = dng.generate_spiral_path(rec, pb[:, -2:], n_frames=nf)
            unit = rec.copy()
            unit[:, :3, -1] /= np.max(np.abs(unit[:, :3, -1]))
            out["dng_spiral_dtu_%d_%d" % (n, nf)] = dng.generate_spiral_path_dtu(unit, n_frames=nf)
            out["dng_backcenter_%d_%d" % (n, nf)] = dng.backcenter_poses(out["dng_spiral_%d_%d" % (n, nf)], poses)
        for seed in (0, 1):
            np.random.seed(seed)
            out["random_llff_%d_s%d" % (n, seed)] = fsgs.generate_random_poses_llff(views)[:6]   # (it draws 10 000; rand(3) each)
            np.random.seed(seed)
            out["random_360_%d_s%d" % (n, seed)] = np.stack(fsgs.generate_random_poses_360(views, n_frames=7))
        with tempfile.TemporaryDirectory() as tmp:
            np.save(os.path.join(tmp, "poses_bounds.npy"), pb)
            for tag, fn in (("llff", "CreateLLFFSpiral"), ("dtu", "CreateDTUSpiral")):
                captured.clear()
                ns[fn](tmp)
                cams = captured["test_cameras"]
                assert len(cams) == 180
                out["create_%s_%d_R" % (tag, n)] = np.stack([c.R for c in cams])
                out["create_%s_%d_T" % (tag, n)] = np.stack([c.T for c in cams])
                out["create_%s_%d_hwf" % (tag, n)] = np.array([cams[0].height, cams[0].width, cams[0].FovX, cams[0].FovY])
    return out


# ------------------------------------------------------------------------------------------------------- depth
def gen_depth_vis(ref):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    turbo = matplotlib.colormaps["turbo"]
    general = load(os.path.join(ref, "FSGS", "utils", "general_utils.py"), "ref_fsgs_general_utils")
    general.cm = types.SimpleNamespace(get_cmap=lambda name: matplotlib.colormaps[name])
    dng = pull(os.path.join(ref, "DNGaussian", "render.py"), ("weighted_percentile", "visualize_cmap", "depth_curve_fn"), dict(np=np))
    out = {"turbo": turbo(np.arange(256))[:, :3]}
    for name, (depth, alpha, rules) in depth_vis_cases.cases().items():
        out[name + "_depth"] = depth
        x = depth
        if alpha is not None:
            out[name + "_alpha"] = alpha
            d, a = torch.from_numpy(depth), torch.from_numpy(alpha)
            x = ((d - d.min()) / (d.max() - d.min()) + 1 * (1 - a)).numpy()   # render.py:121
            out[name + "_composite"] = x
        for rule in rules:
            with np.errstate(all="ignore"):
                if rule == "fsgs":
                    lo_auto, hi_auto = general.weighted_percentile(x, np.ones_like(x), [50 - 99 / 2, 50 + 99 / 2])
                    lo, hi = lo_auto - 1e-10, hi_auto + 1e-10
                    bgr = general.vis_depth(x.copy())
                    rgb = bgr[..., ::-1]
                    curve = lambda v: 1 / v + 1e-10  # noqa: E731  (only to record the normalised image)
                else:
                    curve = dng["depth_curve_fn"] if rule == "dng" else (lambda v: v)
                    lo_auto, hi_auto = dng["weighted_percentile"](x, np.ones_like(x), [50 - 99. / 2, 50 + 99. / 2])
                    eps = np.finfo(np.float32).eps
                    lo, hi = lo_auto - eps, hi_auto + eps
                    kw = dict(curve_fn=curve) if rule == "dng" else {}
                    col = dng["visualize_cmap"](x.copy(), np.ones_like(x), turbo, **kw).copy()
                    t = torch.as_tensor(col).permute(2, 0, 1)   # render.py:129, then save_image's statement on float64
                    rgb = t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
                # the normalised image: the statements above restated once, then checked below to give the reference's bytes
                clo, chi = curve(lo), curve(hi)
                v = np.nan_to_num(np.clip((curve(x) - np.minimum(clo, chi)) / np.abs(chi - clo), 0, 1))
            key = "%s_%s" % (name, rule)
            out[key + "_bounds"] = np.array([lo, hi], dtype=np.float64)
            if rule == "dng" or x.size < 20000:   # (the largest case keeps only the image the DNGaussian allowance reads)
                out[key + "_v"] = v.astype(np.float64)
            out[key + "_rgb"] = np.ascontiguousarray(rgb)
            # the recorded normalised image is the one the reference coloured: same table rows
            idx = np.array(v, dtype=np.float64) * 256
            idx[idx == 256] = 255
            rows = turbo(np.arange(256))[:, :3][idx.astype(int)]
            want = np.uint8(rows * 255) if rule == "fsgs" else np.clip(rows * 255 + 0.5, 0, 255).astype(np.uint8)
            assert np.array_equal(want, rgb), key
    return out


if __name__ == "__main__":
    ref = sys.argv[1]
    paths = gen_paths(ref)
    np.savez_compressed(os.path.join(HERE, "camera_paths.npz"), **paths)
    vis = gen_depth_vis(ref)
    np.savez_compressed(os.path.join(HERE, "depth_vis.npz"), **vis)
    for f in ("camera_paths.npz", "depth_vis.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
