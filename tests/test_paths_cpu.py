"""Camera paths (gsplat_amd/paths.py) and the render stage's new files (gsplat_amd/render_set.py) without a GPU: every generator
against tests/golden/camera_paths.npz - what the reference's own functions gave on the same seeded inputs
(tests/golden/make_golden_paths.py) - at rtol 1e-12: the operations are the same float64 ones in the same order, so the two
differ by nothing or by the last bits of a LAPACK call (atol 1e-12 on entries that are zero up to rounding); camera_from_pose
against a torch restatement of FSGS/render.py:71-73; the files of write_render_set / write_path_frames on CPU tensors."""
import os
import types

import numpy as np
import pytest
import torch

import depth_vis_cases as dc
from gsplat_amd import depth_vis as dv
from gsplat_amd import paths, render_set, synthetic
from gsplat_amd.imageio import read_png, save_image_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_paths.npz")
RTOL, ATOL = 1e-12, 1e-12


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def views_of(z, n):
    return [types.SimpleNamespace(R=z["views%d_R" % n][i].copy(), T=z["views%d_T" % n][i].copy()) for i in range(n)]


def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == np.float64
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("nf", (4, 7))
def test_fsgs_spiral_and_ellipse(z, n, nf):
    pb = z["pb%d" % n].copy()
    close(paths.generate_spiral_path(pb, n_frames=nf), z["spiral_%d_%d" % (n, nf)])
    assert np.array_equal(pb, z["pb%d" % n]), "the input rows are left alone"
    got = paths.generate_ellipse_path(views_of(z, n), n_frames=nf)
    assert isinstance(got, list) and len(got) == nf
    close(np.stack(got), z["ellipse_%d_%d" % (n, nf)])
    close(np.stack(paths.generate_ellipse_path(views_of(z, n), n_frames=nf, const_speed=False, z_variation=0.3, z_phase=0.25)),
          z["ellipse_z_%d_%d" % (n, nf)])


@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("seed", (0, 1))
def test_random_generators_reproduce_the_reference_draws(z, n, seed):
    got = paths.generate_random_poses_llff(views_of(z, n), z["views%d_bounds" % n], np.random.RandomState(seed), n_poses=6)
    close(got, z["random_llff_%d_s%d" % (n, seed)])
    got = paths.generate_random_poses_360(views_of(z, n), np.random.RandomState(seed), n_frames=7)
    assert len(got) == 6          # the reference drops its last draw
    close(np.stack(got), z["random_360_%d_s%d" % (n, seed)])
    other = paths.generate_random_poses_360(views_of(z, n), np.random.RandomState(seed + 7), n_frames=7)
    assert not np.allclose(np.stack(other), np.stack(got))


@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("nf", (4, 7))
def test_dng_spirals(z, n, nf):
    pb = z["pb%d" % n]
    poses = pb[:, :-2].reshape([-1, 3, 5])[:, :3, :4] @ paths._FIX_ROTATION
    rec = paths.recenter_poses(poses)[0]
    close(rec, z["dng_recenter_%d" % n])
    sp = paths.spiral_path_dng(rec, pb[:, -2:], n_frames=nf)
    close(sp, z["dng_spiral_%d_%d" % (n, nf)])
    close(paths.backcenter_poses(sp, poses), z["dng_backcenter_%d_%d" % (n, nf)])
    unit = rec.copy()
    unit[:, :3, -1] /= np.max(np.abs(unit[:, :3, -1]))
    close(paths.generate_spiral_path_dtu(unit, n_frames=nf), z["dng_spiral_dtu_%d_%d" % (n, nf)])


@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("tag", ("llff", "dtu"))
def test_create_spirals_are_the_reference_cameras(z, n, tag):
    cams = (paths.create_llff_spiral if tag == "llff" else paths.create_dtu_spiral)(z["pb%d" % n])
    assert cams["R"].shape == (180, 3, 3) and cams["T"].shape == (180, 3)
    close(cams["R"], z["create_%s_%d_R" % (tag, n)])
    close(cams["T"], z["create_%s_%d_T" % (tag, n)])
    close(np.array([cams["height"], cams["width"], cams["FovX"], cams["FovY"]]), z["create_%s_%d_hwf" % (tag, n)])
    cam = paths.camera_from_rt(synthetic.look_at_camera((3.0, 0.0, 0.0), 48, 64), cams["R"][0], cams["T"][0])
    w2c = cam.world_view_transform.T.numpy()
    np.testing.assert_allclose(w2c[:3, :3], cams["R"][0].T, atol=1e-6)
    np.testing.assert_allclose(w2c[:3, 3], cams["T"][0], atol=1e-5)


def test_camera_from_pose_is_render_py_71_73(z):
    template = synthetic.look_at_camera((3.0, 0.5, 0.2), 48, 64)
    proj = synthetic.perspective(0.01, 100.0, template.FoVx, template.FoVy).transpose(0, 1)
    for pose in z["spiral_3_4"]:
        # getWorld2View2(R, t) with R = pose[:3, :3].T, zero translation, unit scale - restated in torch, float64 then float32
        Rt = torch.zeros((4, 4), dtype=torch.float64)
        Rt[:3, :3] = torch.from_numpy(pose[:3, :3].T.copy()).T
        Rt[:3, 3] = torch.from_numpy(pose[:3, 3].copy())
        Rt[3, 3] = 1.0
        w2v = torch.linalg.inv(torch.linalg.inv(Rt)).to(torch.float32)
        wvt = w2v.transpose(0, 1)
        full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
        centre = wvt.inverse()[3, :3]
        cam = paths.camera_from_pose(template, pose)
        assert isinstance(cam, synthetic.Camera)
        assert (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy) == (64, 48, template.FoVx, template.FoVy)
        assert torch.allclose(cam.world_view_transform, wvt, rtol=1e-6, atol=1e-6)     # float32 results of two float64 inversions
        assert torch.allclose(cam.full_proj_transform, full, rtol=1e-5, atol=1e-5)
        assert torch.allclose(cam.camera_center, centre, rtol=1e-5, atol=1e-5)
        assert torch.allclose(cam.camera_center.double(), torch.from_numpy(np.linalg.inv(pose)[:3, 3]), atol=1e-5)


def test_pseudo_cameras_and_path_centres(z):
    cams = synthetic.orbit_cameras(32, 24, n_azimuth=4, elevations_deg=(10.0,))
    ps = paths.pseudo_cameras(cams, "360", np.random.RandomState(0), n_poses=5)
    assert len(ps) == 4 and all(isinstance(c, synthetic.Camera) and c.image_width == 32 for c in ps)
    bounds = np.tile(np.array([[2.0, 9.0]]), (4, 1))
    pl = paths.pseudo_cameras(cams, "llff", np.random.RandomState(0), bounds=bounds, n_poses=3)
    assert len(pl) == 3
    with pytest.raises(ValueError):
        paths.pseudo_cameras(cams, "llff", np.random.RandomState(0))
    with pytest.raises(ValueError):
        paths.pseudo_cameras(cams, "blender", np.random.RandomState(0))
    c = paths.path_centres(ps)
    assert c.shape == (4, 3) and c.dtype == torch.float32 and torch.equal(c[1], ps[1].camera_center)
    assert paths.path_centres([]).shape == (0, 3)
    # a package camera gives the generators the pose its matrices hold
    R, T = paths._rt(cams[0])
    np.testing.assert_allclose(R.T, cams[0].world_view_transform.T.numpy()[:3, :3])
    np.testing.assert_allclose(T, cams[0].world_view_transform.T.numpy()[:3, 3])


# ----------------------------------------------------------------------------------------------------------- files
def frames_cpu(n=2):
    g = torch.Generator().manual_seed(5)
    depth, alpha, _ = dc.cases()["plain_alpha_64x48"]
    out = []
    for i in range(n):
        out.append(dict(render=torch.rand((3, 64, 48), generator=g) * 1.2 - 0.1, gt=torch.rand((3, 64, 48), generator=g),
                        depth=torch.from_numpy(depth)[None] + 0.1 * i, alpha=torch.from_numpy(alpha)[None]))
    return out


def listing(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_write_render_set_default_is_unchanged_and_colour_depth_adds_one_file_per_view(tmp_path):
    frames = frames_cpu()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    render_set.write_render_set(a, "test", 7, frames)
    want = sorted(os.path.join("test", "ours_7", d, f) for d, fs in (("renders", ("00000.png", "00001.png")), ("gt", ("00000.png", "00001.png")),
                                                                    ("depth", ("00000.png", "00001.png", "alpha_00000.png", "alpha_00001.png")))
                  for f in fs)
    assert listing(a) == want                                           # exactly today's files
    render_set.write_render_set(b, "test", 7, frames, colour_depth=True)
    extra = [os.path.join("test", "ours_7", "depth", "color_%05d.png" % i) for i in range(2)]
    assert listing(b) == sorted(want + extra)
    for f in want:                                                      # and today's bytes
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read()
    for i, fr in enumerate(frames):
        got = read_png(os.path.join(b, extra[i]))
        assert np.array_equal(got, dv.colour_depth(fr["depth"], fr["alpha"], rule="dng").numpy())
    # a view without depth gets no colour file
    c = str(tmp_path / "c")
    render_set.write_render_set(c, "test", 7, [dict(render=frames[0]["render"], gt=frames[0]["gt"])], colour_depth=True)
    assert listing(c) == sorted(os.path.join("test", "ours_7", d, "00000.png") for d in ("renders", "gt"))


def test_write_path_frames_layouts(tmp_path):
    frames = frames_cpu()
    root = str(tmp_path / "m")
    base = render_set.write_path_frames(root, frames, layout="dng_spiral", iteration=3)
    assert base == os.path.join(root, "render", "ours_3")
    assert listing(root) == sorted(os.path.join("render", "ours_3", p + "%05d.png" % i) for i in range(2) for p in ("", "depth_", "cdepth_"))
    for i, fr in enumerate(frames):
        d = (fr["depth"] - fr["depth"].min()) / (fr["depth"].max() - fr["depth"].min()) + 1 * (1 - fr["alpha"])
        assert np.array_equal(read_png(os.path.join(base, "%05d.png" % i)), save_image_bytes(fr["render"]).numpy())
        assert np.array_equal(read_png(os.path.join(base, "depth_%05d.png" % i)), save_image_bytes(1 - d).numpy())
        assert np.array_equal(read_png(os.path.join(base, "cdepth_%05d.png" % i)), dv.colour_depth(fr["depth"], fr["alpha"], rule="dng").numpy())
    root2 = str(tmp_path / "v")
    base2 = render_set.write_path_frames(root2, frames, layout="fsgs_video", iteration=3, fsgs_depth=True, name="test")
    sets = os.path.join("test", "ours_3", "renders")
    assert listing(root2) == sorted([os.path.join("video", "ours_3", "%05d.png" % i) for i in range(2)] +
                                    [os.path.join(sets, "%05d_depth.%s" % (i, e)) for i in range(2) for e in ("png", "npy")])
    for i, fr in enumerate(frames):
        assert np.array_equal(read_png(os.path.join(base2, "%05d.png" % i)), save_image_bytes(fr["render"].clamp(0, 1)).numpy())
        assert np.array_equal(read_png(os.path.join(root2, sets, "%05d_depth.png" % i)), dv.colour_depth(fr["depth"], rule="fsgs").numpy())
        assert np.array_equal(np.load(os.path.join(root2, sets, "%05d_depth.npy" % i)), fr["depth"][0].numpy())
    with pytest.raises(ValueError):
        render_set.write_path_frames(root, frames, layout="mp4")
    with pytest.raises(ValueError):
        render_set.write_path_frames(root, [dict(render=frames[0]["render"])], layout="dng_spiral")


def test_render_set_docstring_no_longer_lists_the_coloured_depth_as_missing():
    assert "is not written" not in render_set.__doc__ and "color_%05d.png" in render_set.__doc__
    assert "no video container" in render_set.__doc__
