"""From a dataset directory to what the trainers take: cameras, ground-truth images and alpha masks on the device, the scene's
extent and the initial model.  Counterparts of

  Scene                        LGDWT-GS/scene/__init__.py
  image_resolution             LGDWT-GS/utils/camera_utils.py:42-61 (loadCam's target size)
  the images                   LGDWT-GS/scene/cameras.py:42-56 through gsplat_amd.imageio.ingest_image
  read_scene_info              LGDWT-GS/scene/dataset_readers.py:188-421 (readColmapSceneInfo, readNerfSyntheticInfo) over the
                               readers of gsplat_amd/io.py

Divergences, on purpose:
  * Nothing is ever written into the source directory.  Where the reference converts points3D.bin to a .ply beside it (or
    stores NeRF-synthetic's random points3d.ply) the first time a scene is opened, the point cloud stays in memory here - with
    the values the reference reads back from the file it wrote (float32 positions, colours through a byte) - and only
    <model_path>/input.ply is written.
  * Cameras keep the readers' order: by image name for COLMAP, the transforms files' order for NeRF-synthetic.  The reference's
    random.shuffle of both lists is not reproduced: the Trainer draws its own cameras (Trainer.draw_cameras).
  * NeRF-synthetic's composite happens where the image is ingested, not in the reader; the bytes are the reference's.
  * NeRF-synthetic's random points come from a generator seeded by `seed`, not from numpy's global state.
Image files: 8-bit PNG through gsplat_amd.imageio.read_png; anything that reader refuses, and every other format (JPEG), through
Pillow when it is importable - it stays optional."""
import collections
import json
import os
import struct

import numpy as np
import torch

from . import imageio
from . import io as gio
from . import synthetic

SceneInfo = collections.namedtuple("SceneInfo", ["point_cloud", "train_cameras", "test_cameras", "nerf_normalization",
                                                 "ply_path", "is_nerf_synthetic"])


def image_resolution(orig_w, orig_h, resolution, resolution_scale=1.0):
    """loadCam's rule (camera_utils.py:42-61) -> (width, height).  resolution 1, 2, 4, 8: a divisor, rounded by Python's round()
    (half to even).  -1: down to width 1600 when the image is wider, else unchanged.  Any other number: the target width.  Those
    two go through int()."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def _read_with_pillow(path, why):
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("read_image: %s needs Pillow, which is not installed (%s); 8-bit non-interlaced PNG files are read "
                           "without it" % (path, why))
    with Image.open(path) as im:
        if im.mode in ("L", "LA", "1", "I", "I;16", "F"):
            raise ValueError("read_image: %s is a grey image (mode %s): the ground truth takes three colour channels" % (path, im.mode))
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "transparency" in im.info else "RGB")
        return np.array(im)   # (a copy: what asarray hands out is read-only)


def read_image(path):
    """-> uint8 numpy [H,W,3] or [H,W,4].  8-bit PNG: read_png.  What that reader refuses (16-bit, palette, interlaced) and
    every other extension go through Pillow if it is importable; without it the error names the file and says so.  Grey and
    grey + alpha images raise: the reference's gt_image[:3] of such a file is one channel."""
    if os.path.splitext(path)[1].lower() == ".png":
        try:
            u8 = imageio.read_png(path)
        except ValueError as e:
            if not os.path.exists(path):
                raise
            u8 = _read_with_pillow(path, str(e))
    else:
        u8 = _read_with_pillow(path, "not a PNG file")
    if u8.ndim != 3 or u8.shape[2] not in (3, 4):
        raise ValueError("read_image: %s is a grey image (%d channel(s)): the ground truth takes three colour channels"
                         % (path, 1 if u8.ndim == 2 else u8.shape[2]))
    return u8


def _image_size(path):
    """(width, height) of an image file: the PNG header, else the decoded image"""
    with open(path, "rb") as fp:
        head = fp.read(24)
    if head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR":
        return struct.unpack(">II", head[16:24])
    u8 = read_image(path)
    return u8.shape[1], u8.shape[0]


def _stored_cloud(xyz, rgb):
    """What fetchPly reads back from the file storePly writes: float32 positions, colours through a byte, zero normals"""
    pts = np.asarray(xyz).astype(np.float32)
    col = np.asarray(rgb).astype(np.uint8) / 255.0
    return gio.BasicPointCloud(points=pts, colors=col, normals=np.zeros_like(pts))


def _points3d(folder):
    try:
        xyz, rgb, _ = gio.read_points3D_binary(os.path.join(folder, "points3D.bin"))
    except (OSError, ValueError, struct.error):
        xyz, rgb, _ = gio.read_points3D_text(os.path.join(folder, "points3D.txt"))
    return _stored_cloud(xyz, rgb)


def _thin(train, n_views):
    if n_views > 0 and len(train) > n_views:
        return [train[i] for i in np.linspace(0, len(train) - 1, n_views, dtype=int)]
    return train


def _read_colmap(path, images, eval, train_test_exp, llffhold, n_views, point_cloud_type):
    sparse = os.path.join(path, "sparse/0")
    try:
        ext = gio.read_extrinsics_binary(os.path.join(sparse, "images.bin"))
        intr = gio.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    except (OSError, ValueError, KeyError, struct.error):
        ext = gio.read_extrinsics_text(os.path.join(sparse, "images.txt"))
        intr = gio.read_intrinsics_text(os.path.join(sparse, "cameras.txt"))
    test_names = []
    if eval:
        if "360" in path:
            llffhold = 8
        if llffhold:
            names = sorted(ext[k].name for k in ext)
            test_names = [n for i, n in enumerate(names) if i % llffhold == 0]
        else:
            with open(os.path.join(sparse, "test.txt"), "r") as fp:
                test_names = [line.strip() for line in fp]
    cams = gio.read_colmap_cameras(ext, intr, os.path.join(path, "sorghum_rgb" if images is None else images), set(test_names))
    train = _thin([c for c in cams if train_test_exp or not c.is_test], n_views)
    test = [c for c in cams if c.is_test]
    # dataset_readers.py:264-313: which point cloud
    if n_views > 0 and point_cloud_type == "dense":
        ply_path = os.path.join(path, "%d_views/dense/fused.ply" % n_views)
    elif n_views > 0 and point_cloud_type == "triangulated":
        ply_path = os.path.join(path, "%d_views/triangulated/points3D.ply" % n_views)
    else:
        ply_path = os.path.join(sparse, "points3D.ply")
    pcd = None
    if os.path.exists(ply_path):
        try:
            pcd = gio.fetch_ply(ply_path)
        except (OSError, ValueError, KeyError):
            pcd = None   # (as the reference: a scene without a readable cloud has none)
    elif "triangulated" in ply_path or "sparse" in ply_path:
        pcd = _points3d(os.path.dirname(ply_path))   # the reference's one-time conversion, kept in memory
    return SceneInfo(pcd, train, test, gio.nerfpp_norm(train), ply_path, False)


def _read_blender(path, eval, n_views, seed, extension=".png"):
    def cams_of(name, is_test):
        if not os.path.exists(os.path.join(path, name)):
            return []
        out = []
        for c in gio.read_cameras_from_transforms(path, name, is_test=is_test, extension=extension):
            w, h = _image_size(c.image_path)
            out.append(c._replace(width=w, height=h, FovY=synthetic.focal2fov(synthetic.fov2focal(c.FovX, w), h)))
        return out
    train, test = cams_of("transforms_train.json", False), cams_of("transforms_test.json", True)
    if not eval:
        train, test = train + test, []
    train = _thin(train, n_views)
    ply_path = os.path.join(path, "points3d.ply")
    if os.path.exists(ply_path):
        pcd = gio.fetch_ply(ply_path)
    else:   # dataset_readers.py:399-409: no COLMAP data, random points inside the synthetic scenes' bounds
        rng = np.random.RandomState(seed)
        xyz = rng.random_sample((100_000, 3)) * 2.6 - 1.3
        shs = rng.random_sample((100_000, 3)) / 255.0
        pcd = _stored_cloud(xyz, (shs * synthetic.C0 + 0.5) * 255)
    return SceneInfo(pcd, train, test, gio.nerfpp_norm(train), ply_path, True)


def read_scene_info(source_path, images="images", depths="", eval=False, train_test_exp=False, llffhold=8, n_views=0,
                    point_cloud_type="dense", white_background=False, seed=0):
    """sceneLoadTypeCallbacks (scene/__init__.py:43-50): a folder with sparse/ is a COLMAP scene, one with
    transforms_train.json NeRF-synthetic -> SceneInfo(point_cloud, train_cameras, test_cameras, nerf_normalization, ply_path,
    is_nerf_synthetic), the cameras as gsplat_amd.io.CameraInfo.  ply_path is where the reference reads - and, when the file
    is missing, writes - the point cloud; here a missing file leaves the cloud in memory.  depths and white_background take part
    where the images are ingested (Scene); they are accepted here so that the call reads like the reference's."""
    if os.path.exists(os.path.join(source_path, "sparse")):
        return _read_colmap(source_path, images, eval, train_test_exp, llffhold, n_views, point_cloud_type)
    if os.path.exists(os.path.join(source_path, "transforms_train.json")):
        return _read_blender(source_path, eval, n_views, seed)
    raise ValueError("%s: could not recognize the scene type (neither sparse/ nor transforms_train.json)" % source_path)


def search_for_max_iteration(folder):
    """utils/system_utils.py:searchForMaxIteration: the largest N among iteration_N"""
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


# What ingest="auto" means is a measurement (tests/tools/scene_load_timing.py, profiles/scene_load_timing.txt): the device call
# only where it is faster than the host path of the same commit by more than the windows' spread.  On one MI355X it is, at both
# image shapes (1458 against 1.26 ms, 16.1 against 0.11 ms per image) and for a whole 24-frame Scene (568 against 308 ms, spreads
# 149 and 14): "auto" is the device path on a GPU.  A CPU device has no kernel path and takes the host one.
AUTO_INGEST = "device"


class Scene:
    """scene/__init__.py: the cameras of a dataset at every resolution scale, the extent, the model.

    params: the ModelParams fields (source_path, model_path, images, depths, resolution, white_background, train_test_exp,
    eval, n_views, point_cloud_type; optionally llffhold and seed), as a Namespace or anything with those attributes.
    train_cameras / test_cameras [scale]: synthetic.Camera tuples at the resized size, tensors on `device`;
    gt_images / alpha_masks [scale] and test_gt_images / test_alpha_masks [scale]: what Camera.original_image and
    Camera.alpha_mask hold, on `device`; train_names / test_names: the image names.  masked: some training mask is not all ones
    (else a Trainer needs no alpha_masks: multiplying by ones changes no bit).
    ingest: "host" (numpy), "device" (gs_image_ingest) or "auto" (AUTO_INGEST on a GPU, the host path on a CPU device)."""

    def __init__(self, params, device, api=None, load_iteration=None, resolution_scales=(1.0,), ingest="auto"):
        if ingest not in ("auto", "host", "device"):
            raise ValueError("ingest must be 'auto', 'host' or 'device'")
        self.device = torch.device(device)
        if ingest == "auto":
            ingest = AUTO_INGEST if self.device.type == "cuda" else "host"
        if ingest == "device" and self.device.type != "cuda":
            raise RuntimeError("ingest='device' needs a CUDA(HIP) device - there is no CPU kernel path")
        self.ingest = ingest
        self.params = params
        self.model_path = params.model_path
        self.loaded_iter = None
        if load_iteration:
            self.loaded_iter = search_for_max_iteration(os.path.join(self.model_path, "point_cloud")) \
                if load_iteration == -1 else load_iteration
        info = read_scene_info(params.source_path, params.images, params.depths, params.eval, params.train_test_exp,
                               llffhold=getattr(params, "llffhold", 8), n_views=params.n_views,
                               point_cloud_type=params.point_cloud_type, white_background=params.white_background,
                               seed=getattr(params, "seed", 0))
        self.info = info
        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            dest = os.path.join(self.model_path, "input.ply")
            if os.path.exists(info.ply_path):
                with open(info.ply_path, "rb") as src, open(dest, "wb") as dst:
                    dst.write(src.read())
            elif info.point_cloud is not None:
                gio.store_ply(dest, info.point_cloud.points, np.rint(info.point_cloud.colors * 255.0))
            gio.write_cameras_json(os.path.join(self.model_path, "cameras.json"), list(info.test_cameras) + list(info.train_cameras))
        self.cameras_extent = info.nerf_normalization["radius"]
        self.train_names = [c.image_name for c in info.train_cameras]
        self.test_names = [c.image_name for c in info.test_cameras]
        self.train_cameras, self.gt_images, self.alpha_masks = {}, {}, {}
        self.test_cameras, self.test_gt_images, self.test_alpha_masks = {}, {}, {}
        for scale in resolution_scales:
            self.train_cameras[scale], self.gt_images[scale], self.alpha_masks[scale] = self._load(info.train_cameras, scale, False)
            self.test_cameras[scale], self.test_gt_images[scale], self.test_alpha_masks[scale] = self._load(info.test_cameras, scale, True)
        self.masked = any(bool((m != 1).any()) for masks in self.alpha_masks.values() for m in masks)
        self.model = self._model(info, api)

    def _load(self, cam_infos, scale, is_test_dataset):
        from .trainer import camera_to
        p = self.params
        cams, gts, masks = [], [], []
        wb = bool(p.white_background) if self.info.is_nerf_synthetic else None
        for c in cam_infos:
            u8 = read_image(c.image_path)
            size = image_resolution(u8.shape[1], u8.shape[0], p.resolution, scale)
            kw = dict(white_background=wb, train_test_exp=bool(p.train_test_exp), is_test_view=bool(c.is_test),
                      is_test_dataset=is_test_dataset)
            if self.ingest == "device":
                image, mask = imageio.ingest_image(torch.from_numpy(u8).to(self.device), size, **kw)
            else:
                image, mask = (torch.from_numpy(a).to(self.device) for a in imageio.ingest_image(u8, size, **kw))
            cams.append(camera_to(synthetic.make_camera(c.R, c.T, c.FovX, c.FovY, size[0], size[1]), self.device))
            gts.append(image)
            masks.append(mask)
        return cams, gts, masks

    def _model(self, info, api):
        from .trainer import GaussianModelLite
        knn = None   # (a CPU device: create_from_pcd's float64 brute force)
        if self.device.type == "cuda":
            from simple_knn._C import distCUDA2
            knn = lambda x: distCUDA2(x.to(self.device)).cpu()  # noqa: E731
        if self.loaded_iter:
            seed_pts, seed_col = np.zeros((4, 3), dtype=np.float32) + np.arange(4, dtype=np.float32)[:, None], np.full((4, 3), 0.5)
            model = GaussianModelLite.create_from_pcd(seed_pts, seed_col, self.device, spatial_lr_scale=self.cameras_extent, api=api,
                                                      knn=None, spatial_order=False)
            model.load_ply(os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter), "point_cloud.ply"))
            return model
        if info.point_cloud is None:
            raise ValueError("%s: no point cloud to start from (looked for %s)" % (self.params.source_path, info.ply_path))
        return GaussianModelLite.create_from_pcd(info.point_cloud.points, info.point_cloud.colors, self.device,
                                                 spatial_lr_scale=self.cameras_extent, api=api, knn=knn)

    def save(self, iteration):
        """scene/__init__.py:86-95: point_cloud/iteration_N/point_cloud.ply, and exposure.json when the model trains exposures"""
        self.model.save_ply(os.path.join(self.model_path, "point_cloud/iteration_{}".format(iteration), "point_cloud.ply"))
        if self.model.exposure is not None:
            exposure = self.model.exposure.detach().cpu().numpy()
            with open(os.path.join(self.model_path, "exposure.json"), "w") as fp:
                json.dump({name: exposure[i].tolist() for i, name in enumerate(self.train_names)}, fp, indent=2)

    def load_depth_priors(self, trainer, scale=1.0):
        """params.depths != "": the training cameras' inverse-depth maps through Trainer.load_depth_priors (depth_params.json of
        a COLMAP scene beside its sparse model)"""
        from .depth_priors import image_key, read_depth_params
        p = self.params
        if not p.depths:
            return None
        dp = None if self.info.is_nerf_synthetic else read_depth_params(os.path.join(p.source_path, "sparse/0", "depth_params.json"))
        keys = [n if self.info.is_nerf_synthetic else image_key(n) for n in self.train_names]
        return trainer.load_depth_priors(keys, os.path.join(p.source_path, p.depths), depth_params=dp,
                                         nerf_synthetic=self.info.is_nerf_synthetic)
