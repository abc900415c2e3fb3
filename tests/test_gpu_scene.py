"""A scene on disk, end to end on the device: gsplat_amd/scene.py and gsplat_amd/cli.py.

The scene is written by the test: 6 orbit cameras at 96 x 64 as a COLMAP binary model, ground truth rendered from a seeded
Gaussian set and saved as PNG (RGB, and an RGBA variant loaded at -r 2).  Scene(ingest="device") must equal
Scene(ingest="host") bit for bit.  `cli train` must end with the very parameters of a Trainer assembled by hand from the same
Scene tensors, options and seed - every kernel of the step is deterministic, so any difference is a wiring fault - and
`cli render` / `cli metrics` must give the numbers of evaluate_dir called directly."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gsplat_amd import cli, imageio, render_set, scene, synthetic
from gsplat_amd import io as gio

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sparse-view-3dgs-pack_amd")
W, H, N_CAMS = 96, 64, 6
TRAIN_FLAGS = ["--eval", "--iterations", "60", "--densify_from_iter", "20", "--densification_interval", "10", "--patch_size", "32",
               "--test_iterations", "60", "--save_iterations", "60", "--seed", "3", "--quiet"]


def write_colmap(folder, cams, names, points, colours):
    cameras = {1: gio.ColmapCamera(1, "PINHOLE", W, H, [synthetic.fov2focal(cams[0].FoVx, W), synthetic.fov2focal(cams[0].FoVy, H),
                                                          W / 2.0, H / 2.0])}
    images = {}
    for i, (cam, name) in enumerate(zip(cams, names)):
        w2c = cam.world_view_transform.t().double().numpy()
        images[i + 1] = gio.ColmapImage(i + 1, gio.rotmat2qvec(w2c[:3, :3]), w2c[:3, 3], 1, name, np.zeros((0, 2)), np.zeros((0,), dtype=np.int64))
    gio.write_colmap_binary(folder, cameras, images, (points, colours, np.zeros((len(points), 1))))


@pytest.fixture(scope="module")
def written(hip, tmp_path_factory):
    """-> dict(rgb=source dir with RGB PNGs, rgba=source dir with RGBA PNGs, pixels=...)"""
    import diff_gaussian_rasterization as dgr
    from gsplat_amd.trainer import GaussianModelLite, camera_to, render
    base = tmp_path_factory.mktemp("scene")
    sc = synthetic.trained_like(2000, seed=0, scale_mult=1.5)
    target = GaussianModelLite(sc, DEV, api=hip.api)
    cams = synthetic.orbit_cameras(W, H, n_azimuth=N_CAMS, elevations_deg=(20.0,))
    bg = torch.zeros(3, device=DEV)
    names = ["view_%02d.png" % i for i in range(N_CAMS)]
    g = torch.Generator().manual_seed(4)
    keep = torch.randperm(2000, generator=g)[:600]
    points = sc["means3D"][keep].double().numpy()
    colours = (sc["shs"][keep, 0, :] * synthetic.C0 + 0.5).clamp(0, 1).mul(255).round().numpy()
    out = {"names": names, "pixels": {}}
    for kind in ("rgb", "rgba"):
        src = str(base / kind)
        os.makedirs(os.path.join(src, "images"))
        write_colmap(os.path.join(src, "sparse", "0"), cams, names, points, colours)
        out[kind] = src
    with torch.no_grad():
        for cam, name in zip(cams, names):
            pkg = render(camera_to(cam, DEV), target, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg)
            rgb = imageio.save_image_bytes(pkg["render"]).cpu().numpy()
            alpha = torch.randint(0, 256, (H, W, 1), generator=g, dtype=torch.uint8).numpy()
            alpha[:, : W // 3] = 255
            alpha[: H // 4] = 0
            imageio.write_png(os.path.join(out["rgb"], "images", name), rgb)
            imageio.write_png(os.path.join(out["rgba"], "images", name), np.concatenate((rgb, alpha), axis=2))
            out["pixels"][name] = rgb
    assert float(np.mean([p.mean() for p in out["pixels"].values()])) > 5, "the ground truth shows something"
    return out


def params(src, model, **kw):
    base = dict(sh_degree=3, source_path=src, model_path=model, images="images", depths="", resolution=-1, white_background=False,
                train_test_exp=False, data_device="cuda", eval=True, n_views=0, point_cloud_type="dense")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("kind,resolution,extra", [("rgb", 1, {}), ("rgb", 2, {}), ("rgba", 2, {}), ("rgba", 1, {}),
                                                    ("rgba", 2, dict(train_test_exp=True)), ("rgb", 50, dict(train_test_exp=True))])
def test_device_ingest_equals_host_ingest(hip, written, tmp_path, kind, resolution, extra):
    scenes = [scene.Scene(params(written[kind], str(tmp_path / how), resolution=resolution, **extra), DEV, api=hip.api, ingest=how)
              for how in ("host", "device")]
    host, dev = scenes
    assert host.ingest == "host" and dev.ingest == "device" and host.masked == dev.masked == (kind == "rgba" or bool(extra))
    size = scene.image_resolution(W, H, resolution)
    n_train = N_CAMS if extra else N_CAMS - 1
    assert len(host.gt_images[1.0]) == n_train and len(host.test_gt_images[1.0]) == 1
    for a, b in ((host.gt_images, dev.gt_images), (host.alpha_masks, dev.alpha_masks), (host.test_gt_images, dev.test_gt_images),
                 (host.test_alpha_masks, dev.test_alpha_masks)):
        for x, y in zip(a[1.0], b[1.0]):
            assert x.is_cuda and y.is_cuda and x.shape[-2:] == (size[1], size[0]) and torch.equal(x, y)
    if kind == "rgb" and resolution == 1:
        want = torch.from_numpy(written["pixels"]["view_01.png"]).permute(2, 0, 1).to(torch.float32).div(255)
        assert torch.equal(dev.gt_images[1.0][0].cpu(), want), "the same size keeps the file's bytes"
    assert torch.equal(host.model.flat, dev.model.flat)
    assert json.load(open(os.path.join(dev.model_path, "cameras.json")))[0]["img_name"] == "view_00.png"


@pytest.fixture(scope="module")
def trained(hip, written, tmp_path_factory):
    model_path = str(tmp_path_factory.mktemp("model"))
    res = cli.main(["train", "-s", written["rgb"], "-m", model_path] + TRAIN_FLAGS)
    return model_path, res


def test_cli_train_is_the_trainer_assembled_by_hand(hip, written, trained, tmp_path):
    import diff_gaussian_rasterization as dgr
    import lgdwt_loss
    from gsplat_amd.trainer import TrainOptions, Trainer
    model_path, res = trained
    assert sorted(os.listdir(model_path)) == ["cameras.json", "cfg_args", "input.ply", "point_cloud"]
    assert os.path.exists(os.path.join(model_path, "point_cloud/iteration_60/point_cloud.ply"))
    cfg = cli.parse_cfg_args(open(os.path.join(model_path, "cfg_args")).read())
    assert cfg.source_path == os.path.abspath(written["rgb"]) and cfg.eval is True and cfg.model_path == model_path
    assert list(vars(cfg)) == [f[0] for f in cli.MODEL_FLAGS]
    # by hand: the same Scene tensors, the reference's defaults spelled out, the flags of TRAIN_FLAGS
    sc = scene.Scene(params(written["rgb"], str(tmp_path / "hand"), seed=3), DEV, api=hip.api)
    crit = lgdwt_loss.criterion(lambda_dssim=0.2, dwt_enable=True, patch_dwt_enable=True, patch_size=32)
    opt = TrainOptions(iterations=60, densify_from_iter=20, densification_interval=10, seed=3, cameras_extent=sc.cameras_extent)
    tr = Trainer(sc.model, sc.train_cameras[1.0], sc.gt_images[1.0], crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings,
                 torch.zeros(3, device=DEV))
    densified = 0
    for it in range(1, 61):
        densified += tr.train_iteration(it, opt)["densified"] is not None
    tr.sync()
    got = res["trainer"].model
    assert densified == 4 and got.P == sc.model.P != 600, "iterations 30, 40, 50 and ... densify: the model changed size"
    assert torch.equal(got.flat, sc.model.flat), "cli train and the hand-made Trainer differ: a wiring fault"
    saved = gio.load_gaussians_ply(os.path.join(model_path, "point_cloud/iteration_60/point_cloud.ply"))
    assert np.array_equal(saved["xyz"], got.params["xyz"].detach().cpu().numpy())
    # training_report's figures are Trainer.evaluate's
    lines = cli.report(res["trainer"], res["scene"], 60, out=lambda s: None)
    ev = res["trainer"].evaluate(res["scene"].test_cameras[1.0], res["scene"].test_gt_images[1.0], quantise=False, clamp=True)
    assert lines[0] == "\n[ITER 60] Evaluating test: L1 {} PSNR {}".format(ev["L1"], ev["PSNR"]) and lines[1].startswith("\n[ITER 60] Evaluating train")


def test_cli_render_and_metrics_give_evaluate_dirs_numbers(hip, written, trained):
    model_path, res = trained
    out = cli.main(["render", "-m", model_path, "--quiet"])
    assert out == {k: os.path.join(model_path, k, "ours_60") for k in ("train", "test")}
    assert sorted(os.listdir(os.path.join(out["train"], "renders"))) == ["%05d.png" % i for i in range(N_CAMS - 1)]
    assert np.array_equal(imageio.read_png(os.path.join(out["test"], "gt", "00000.png")), written["pixels"]["view_00.png"])
    # the render of the loaded PLY is the trained model's
    import diff_gaussian_rasterization as dgr
    from gsplat_amd.trainer import render
    m = res["trainer"].model
    with torch.no_grad():
        img = render(res["scene"].test_cameras[1.0][0], m, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings,
                     torch.zeros(3, device=DEV), clamp=False)["render"]
    assert np.array_equal(imageio.read_png(os.path.join(out["test"], "renders", "00000.png")), imageio.save_image_bytes(img).cpu().numpy())
    got = cli.main(["metrics", "-m", model_path])[model_path]
    want = render_set.evaluate_dir(model_path, "test")
    assert got == want and list(got) == ["ours_60"] and got["ours_60"]["PSNR"] > 10
    results = json.load(open(os.path.join(model_path, "results.json")))
    assert results == {"ours_60": {k: want["ours_60"][k] for k in ("SSIM", "PSNR", "L1")}}
    # once through `python -m`, as a fresh child process
    os.remove(os.path.join(model_path, "results.json"))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    child = subprocess.run([sys.executable, "-m", "gsplat_amd.cli", "metrics", "-m", model_path], env=env, capture_output=True,
                           text=True, timeout=300)
    assert child.returncode == 0, child.stderr[-2000:]
    assert json.load(open(os.path.join(model_path, "results.json"))) == results and "PSNR" in child.stdout


def test_cli_refuses_what_it_cannot_honour(hip, written, tmp_path):
    with pytest.raises(cli.UnsupportedFlag, match="data_device"):
        cli.main(["train", "-s", written["rgb"], "-m", str(tmp_path / "m"), "--data_device", "cpu"])
    with pytest.raises(cli.UnsupportedFlag, match="opacity_lr"):
        cli.main(["train", "-s", written["rgb"], "-m", str(tmp_path / "m"), "--opacity_lr", "0.05"])
    assert not os.path.exists(str(tmp_path / "m")), "refused before anything is written"


def test_jpeg_images_through_pillow(hip, written, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    src = str(tmp_path / "jpeg")
    os.makedirs(os.path.join(src, "images"))
    names = [n.replace(".png", ".jpg") for n in written["names"]]
    cams = synthetic.orbit_cameras(W, H, n_azimuth=N_CAMS, elevations_deg=(20.0,))
    write_colmap(os.path.join(src, "sparse", "0"), cams, names, np.zeros((8, 3)) + np.arange(8)[:, None], np.full((8, 3), 128.0))
    for n, png in zip(names, written["names"]):
        Image.fromarray(written["pixels"][png], "RGB").save(os.path.join(src, "images", n), quality=90)
    sc = scene.Scene(params(src, str(tmp_path / "m"), resolution=2, eval=False), DEV, api=hip.api, ingest="device")
    decoded = np.asarray(Image.open(os.path.join(src, "images", names[2])))
    want = imageio.resize_u8_numpy(decoded, (W // 2, H // 2)).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert sc.train_names == names and np.array_equal(sc.gt_images[1.0][2].cpu().numpy(), want)
