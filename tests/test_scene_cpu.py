"""gsplat_amd/scene.py without a GPU: loadCam's size rule, the image reader, readColmapSceneInfo / readNerfSyntheticInfo over
tests/golden/colmap and a written transforms scene, and a Scene on the CPU (host ingest, torch Adam)."""
import argparse
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from gsplat_amd import imageio, scene
from gsplat_amd import io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLMAP = os.path.join(ROOT, "tests", "golden", "colmap")
NAMES = ["img_%02d.png" % i for i in range(6)]


# values of the reference's expressions (utils/camera_utils.py:42-61), recorded from them: (orig_w, orig_h, resolution,
# resolution_scale) -> (width, height)
RESOLUTIONS = (((1001, 667, 2, 1.0), (500, 334)),      # round() ties: 500.5 -> 500 (to even), 333.5 -> 334
               ((1601, 1000, -1, 1.0), (1599, 999)),   # 1601 / (1601 / 1600) falls just below 1600 in double: int() truncates
               ((4946, 3286, -1, 1.0), (1600, 1063)),
               ((1600, 1200, -1, 1.0), (1600, 1200)), ((800, 800, -1, 1.0), (800, 800)),
               ((4946, 3286, 1000, 1.0), (1000, 664)),  # an explicit width
               ((1000, 750, 300, 1.0), (300, 225)),
               ((1001, 667, 2, 2.0), (250, 167)), ((779, 519, 4, 1.0), (195, 130)), ((1957, 1091, 8, 1.0), (245, 136)),
               ((4946, 3286, 1, 1.0), (4946, 3286)), ((5187, 3361, -1, 2.0), (800, 518)), ((802, 803, 2, 1.0), (401, 402)))


@pytest.mark.parametrize("args,want", RESOLUTIONS)
def test_image_resolution_is_loadcams_rule(args, want):
    got = scene.image_resolution(*args)
    assert got == want and all(isinstance(v, int) for v in got)


def write_images(folder, names, W=40, H=30, channels=3, seed=0):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = {}
    for n in names:
        out[n] = rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)
        imageio.write_png(os.path.join(folder, n), out[n])
    return out


def colmap_source(tmp_path, images=True, **kw):
    src = tmp_path / "scene"
    os.makedirs(src / "sparse" / "0")
    for f in os.listdir(COLMAP):
        shutil.copy(os.path.join(COLMAP, f), src / "sparse" / "0" / f)
    pixels = write_images(str(src / "images"), NAMES, **kw) if images else {}
    return str(src), pixels


def listing(folder):
    return sorted(os.path.relpath(os.path.join(d, f), folder) for d, _, fs in os.walk(folder) for f in fs)


def test_read_image(tmp_path, monkeypatch):
    px = write_images(str(tmp_path), ["rgb.png"], channels=3)
    px.update(write_images(str(tmp_path), ["rgba.png"], channels=4))
    assert np.array_equal(scene.read_image(str(tmp_path / "rgb.png")), px["rgb.png"])
    assert np.array_equal(scene.read_image(str(tmp_path / "rgba.png")), px["rgba.png"])
    for name, ch in (("grey.png", 1), ("la.png", 2)):
        write_images(str(tmp_path), [name], channels=ch)
        with pytest.raises(ValueError, match="grey"):
            scene.read_image(str(tmp_path / name))
    # Pillow stays optional: without it a file the PNG reader cannot take raises an error that names the file and Pillow
    monkeypatch.setitem(sys.modules, "PIL", None)
    (tmp_path / "photo.jpg").write_bytes(b"\xff\xd8\xff\xe0 not decoded here")
    with pytest.raises(RuntimeError, match=r"photo\.jpg needs Pillow"):
        scene.read_image(str(tmp_path / "photo.jpg"))
    imageio.write_png16(str(tmp_path / "deep.png"), np.zeros((4, 4, 3), dtype=np.uint16))
    with pytest.raises(RuntimeError, match=r"deep\.png needs Pillow"):
        scene.read_image(str(tmp_path / "deep.png"))


def test_read_scene_info_colmap_splits(tmp_path):
    src, _ = colmap_source(tmp_path, images=False)
    before = listing(src)
    info = scene.read_scene_info(src)
    assert [c.image_name for c in info.train_cameras] == NAMES and info.test_cameras == [] and not info.is_nerf_synthetic
    assert all(c.image_path == os.path.join(src, "images", c.image_name) for c in info.train_cameras)
    ev = scene.read_scene_info(src, eval=True)
    assert [c.image_name for c in ev.test_cameras] == ["img_00.png"] and [c.image_name for c in ev.train_cameras] == NAMES[1:]
    assert all(c.is_test for c in ev.test_cameras) and not any(c.is_test for c in ev.train_cameras)
    ev2 = scene.read_scene_info(src, eval=True, llffhold=2)
    assert [c.image_name for c in ev2.test_cameras] == NAMES[0::2] and [c.image_name for c in ev2.train_cameras] == NAMES[1::2]
    # train_test_exp keeps the test views in the training set too, marked
    tte = scene.read_scene_info(src, eval=True, llffhold=2, train_test_exp=True)
    assert [c.image_name for c in tte.train_cameras] == NAMES and [c.is_test for c in tte.train_cameras] == [True, False] * 3
    # n_views: np.linspace(0, n - 1, n_views, dtype=int) over the training cameras; the point cloud is then looked for under
    # <n>_views/ (dense: a file that is not there -> no cloud; sparse: sparse/0)
    nv = scene.read_scene_info(src, eval=True, n_views=2)
    assert [c.image_name for c in nv.train_cameras] == [NAMES[1], NAMES[5]] and nv.point_cloud is None
    assert nv.ply_path == os.path.join(src, "2_views/dense/fused.ply")
    nvs = scene.read_scene_info(src, eval=True, n_views=3, point_cloud_type="sparse")
    assert [c.image_name for c in nvs.train_cameras] == [NAMES[1], NAMES[3], NAMES[5]] and nvs.point_cloud is not None
    # "360" in the path forces llffhold 8; llffhold 0 reads sparse/0/test.txt
    os.rename(src, src + "_360")
    assert [c.image_name for c in scene.read_scene_info(src + "_360", eval=True, llffhold=2).test_cameras] == ["img_00.png"]
    os.rename(src + "_360", src)
    with open(os.path.join(src, "sparse/0/test.txt"), "w") as fp:
        fp.write("img_03.png\nimg_04.png\n")
    assert [c.image_name for c in scene.read_scene_info(src, eval=True, llffhold=0).test_cameras] == ["img_03.png", "img_04.png"]
    os.remove(os.path.join(src, "sparse/0/test.txt"))
    # the normalisation runs over the TRAINING cameras; the cloud is points3D.bin as fetchPly would read it back from storePly's file
    assert info.nerf_normalization["radius"] == gio.nerfpp_norm(info.train_cameras)["radius"]
    assert ev.nerf_normalization["radius"] == gio.nerfpp_norm(ev.train_cameras)["radius"] != info.nerf_normalization["radius"]
    xyz, rgb, _ = gio.read_points3D_binary(os.path.join(src, "sparse/0/points3D.bin"))
    assert info.point_cloud.points.dtype == np.float32 and np.array_equal(info.point_cloud.points, xyz.astype(np.float32))
    assert np.array_equal(info.point_cloud.colors, rgb.astype(np.uint8) / 255.0)
    assert listing(src) == before, "nothing is written into the source directory"
    # text files when the binary ones are missing
    for f in ("images.bin", "cameras.bin", "points3D.bin"):
        os.remove(os.path.join(src, "sparse/0", f))
    with open(os.path.join(src, "sparse/0/cameras.txt"), "w") as fp:
        fp.write("".join("%d PINHOLE 656 488 734.0 886.7 328.0 244.0\n" % i for i in (1, 2, 3, 4)))
    txt = scene.read_scene_info(src)
    assert [c.image_name for c in txt.train_cameras] == NAMES and np.array_equal(txt.point_cloud.points, info.point_cloud.points)


def params(src, model, **kw):
    base = dict(sh_degree=3, source_path=src, model_path=model, images="images", depths="", resolution=-1, white_background=False,
                train_test_exp=False, data_device="cpu", eval=False, n_views=0, point_cloud_type="dense")
    base.update(kw)
    return argparse.Namespace(**base)


def test_scene_on_the_cpu(tmp_path):
    src, pixels = colmap_source(tmp_path)
    before = listing(src)
    model = str(tmp_path / "model")
    sc = scene.Scene(params(src, model, eval=True, resolution=2, images="images"), "cpu", ingest="host")
    assert listing(src) == before, "nothing is written into the source directory"
    assert sorted(os.listdir(model)) == ["cameras.json", "input.ply"]
    cams = json.load(open(os.path.join(model, "cameras.json")))
    assert [c["img_name"] for c in cams] == ["img_00.png"] + NAMES[1:], "test cameras first"
    assert [c["id"] for c in cams] == list(range(6)) and cams[0]["width"] == 656
    assert sc.train_names == NAMES[1:] and sc.test_names == ["img_00.png"]
    assert sc.cameras_extent == sc.info.nerf_normalization["radius"] and not sc.masked
    cam, gt, mask = sc.train_cameras[1.0][0], sc.gt_images[1.0][0], sc.alpha_masks[1.0][0]
    assert (cam.image_width, cam.image_height) == (20, 15) and tuple(gt.shape) == (3, 15, 20) and tuple(mask.shape) == (1, 15, 20)
    want = imageio.resize_u8_numpy(pixels[NAMES[1]], (20, 15)).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(gt.numpy(), want) and float(mask.min()) == 1.0
    info = sc.info.train_cameras[0]
    assert cam.FoVx == info.FovX and cam.FoVy == info.FovY
    # input.ply is the cloud the model starts from
    pts = gio.fetch_ply(os.path.join(model, "input.ply"))
    assert np.array_equal(pts.points, sc.info.point_cloud.points) and np.array_equal(pts.colors, sc.info.point_cloud.colors)
    assert sc.model.P == pts.points.shape[0] and sc.model.active_sh_degree == 0
    assert torch.equal(sc.model.params["xyz"].detach(), torch.from_numpy(pts.points))
    # save, then a second Scene loads the highest iteration and writes nothing else
    sc.save(7)
    sc.save(30)
    assert os.path.exists(os.path.join(model, "point_cloud/iteration_30/point_cloud.ply")) and not os.path.exists(os.path.join(model, "exposure.json"))
    os.remove(os.path.join(model, "cameras.json"))
    again = scene.Scene(params(src, model, eval=True, resolution=2), "cpu", load_iteration=-1, ingest="host")
    assert again.loaded_iter == 30 and not os.path.exists(os.path.join(model, "cameras.json"))
    assert torch.equal(again.model.params["xyz"].detach(), sc.model.params["xyz"].detach()) and again.model.active_sh_degree == 3
    with pytest.raises(RuntimeError, match="CUDA"):
        scene.Scene(params(src, model), "cpu", ingest="device")
    # RGBA images: the alpha channel is the mask, and train_test_exp halves the test views' masks in both sets
    shutil.rmtree(os.path.join(src, "images"))
    rgba = write_images(os.path.join(src, "images"), NAMES, channels=4, seed=3)
    sc4 = scene.Scene(params(src, str(tmp_path / "m4"), eval=True, train_test_exp=True, resolution=1), "cpu", ingest="host")
    assert sc4.masked and sc4.train_names == NAMES
    a = torch.from_numpy(rgba["img_00.png"][:, :, 3].astype(np.float32) / np.float32(255))
    assert torch.equal(sc4.alpha_masks[1.0][0][0, :, :20], a[:, :20]) and float(sc4.alpha_masks[1.0][0][0, :, 20:].abs().max()) == 0
    assert torch.equal(sc4.test_alpha_masks[1.0][0][0, :, 20:], a[:, 20:]) and float(sc4.test_alpha_masks[1.0][0][0, :, :20].abs().max()) == 0
    b = torch.from_numpy(rgba["img_01.png"][:, :, 3].astype(np.float32) / np.float32(255))
    assert torch.equal(sc4.alpha_masks[1.0][1][0], b)


def test_read_scene_info_blender(tmp_path):
    src = str(tmp_path / "lego")
    frames = lambda names: {"camera_angle_x": 0.69, "frames": [  # noqa: E731
        {"file_path": "./" + n, "transform_matrix": [[1, 0, 0, 0.1 * i], [0, 1, 0, 0.2], [0, 0, 1, 4.0 + i], [0, 0, 0, 1]]}
        for i, n in enumerate(names)]}
    os.makedirs(src)
    rgba = write_images(src, ["train_0.png", "train_1.png", "test_0.png"], W=24, H=16, channels=4, seed=9)
    json.dump(frames(["train_0", "train_1"]), open(os.path.join(src, "transforms_train.json"), "w"))
    json.dump(frames(["test_0"]), open(os.path.join(src, "transforms_test.json"), "w"))
    before = listing(src)
    merged = scene.read_scene_info(src)
    assert merged.is_nerf_synthetic and [c.image_name for c in merged.train_cameras] == ["train_0", "train_1", "test_0"]
    assert merged.test_cameras == [] and (merged.train_cameras[0].width, merged.train_cameras[0].height) == (24, 16)
    ev = scene.read_scene_info(src, eval=True)
    assert [c.image_name for c in ev.train_cameras] == ["train_0", "train_1"] and [c.image_name for c in ev.test_cameras] == ["test_0"]
    # no points3d.ply: 100 000 seeded points in [-1.3, 1.3]^3, kept in memory
    assert merged.point_cloud.points.shape == (100_000, 3) and float(np.abs(merged.point_cloud.points).max()) <= 1.3
    assert np.array_equal(merged.point_cloud.points, ev.point_cloud.points)
    assert not np.array_equal(scene.read_scene_info(src, seed=1).point_cloud.points, merged.point_cloud.points)
    assert listing(src) == before, "nothing is written into the source directory"
    # the composite of the reference's reader happens at ingest: the same values
    u8 = scene.read_image(os.path.join(src, "train_0.png"))
    image, mask = imageio.ingest_image(u8, (24, 16), white_background=True)
    assert np.array_equal(image, gio.composite_rgba(rgba["train_0.png"], True)) and float(mask.min()) == 1.0
    with pytest.raises(ValueError, match="could not recognize"):
        scene.read_scene_info(str(tmp_path))
