"""Depth priors from files: from a COLMAP directory and a folder of 16-bit mono inverse-depth PNGs to the list
Trainer.depth_priors takes (gaussian-splatting / LGDWT-GS, `-d depths`).

  depth_scales        utils/make_depth_scale.py:8-64 (get_scales) for every image: the scale and offset between the mono map's
                      inverse depth and COLMAP's, by medians and mean absolute deviations
  make_depth_params   that script's __main__: sparse/0 + depths_dir -> sparse/0/depth_params.json
  read_depth_params   scene/dataset_readers.py:157-170: the JSON with med_scale added to every entry
  prepare_invdepth    scene/cameras.py:60-78: resize to the camera, negatives to zero, the reliability rule, scale and offset
  load_depth_priors   utils/camera_utils.py:23-28 + the above, per camera: None, or (invdepth [1,H,W], None)

The host numpy path is the default and the arbiter; on_device=True (depth_scales) or a CUDA tensor / device= (prepare_invdepth)
goes through gs_depth_scales / gs_invdepth_prepare (csrc/gs_depth_priors.hip).  cv2 is no dependency: its two calls are restated.

get_scales restated, statement by statement (numpy 2 promotion; a Python float beside a float32 array compares in float32):
  used   = (id >= 0) * (id < len(table)); the dense table's rows that no point fills are zeros and ARE used, as in the script
  z      = ((X r20 + Y r21) + Z r22) + t2 in float64, one rounding per operation.  The script forms all of np.dot(pts, R.T) + tvec
           and reads column 2 alone; BLAS's summation order inside that product is not specified, this one is
  inv    = 1 / z;  s = map rows / camera height;  maps = (xys * s).astype(float32)
  valid  = (mx >= 0) * (my >= 0) * (mx < width * s) * (my < height * s) * (inv > 0)
  valid.sum() > 10 and inv.max() - inv.min() > 1e-3 (over the USED observations; NaN fails the test), else scale = offset = 0
  mono   = the map / 2**16 sampled at maps (below); np.median and np.mean(np.abs(. - median)) of both, mono's in float32
  scale  = s_colmap / s_mono, offset = t_colmap - t_mono * scale
The sample (cv2.remap, INTER_LINEAR, BORDER_REPLICATE, as OpenCV documents it - DESIGN.md 4.8.4 says what is unverified): each
coordinate rounded half-to-even to 1 / 32 pixel, i = rint(32 x), cell = i >> 5, f = (i & 31) / 32; weights (1 - fy)(1 - fx),
(1 - fy) fx, fy (1 - fx), fy fx (exact in fp32); ((w00 v00 + w01 v01) + w10 v10) + w11 v11, every multiply and add rounded to
fp32; cell indices clamped to the map.  coord_bits=None keeps the float32 coordinate: cell = floor(x), f = x - cell.
The resize (cv2.resize's INTER_LINEAR on a float image, as documented): fx = float32((dx + 0.5) * (W / W2) - 0.5), sx = floor(fx),
fx -= sx, sx < 0 -> (0, 0), sx >= W - 1 -> (W - 1, 0); rows first, a0 S0 + a1 S1 with a0 = 1 - fx, then columns the same way,
every operation rounded to fp32; equal sizes copy.
Named divergences: a depth file with more than one channel raises ValueError (the script takes cv2's channel 0, which is the
file's LAST colour channel - an order this package cannot check); the device's mean absolute deviations are float64 sums where
numpy's mono one is a float32 pairwise sum (the tests state the distance)."""
import json
import os

import numpy as np
import torch

from . import io as gio
from .imageio import read_png16

COORD_BITS = 5            # cv2.remap's INTER_BITS
MAP_U16, MAP_F32 = 0, 1   # GS_DEPTH_MAP_*
STAT_KEYS = ("scale", "offset", "n_valid", "t_colmap", "s_colmap", "t_mono", "s_mono")


def image_key(name):
    """image_meta.name[:-n_remove]: the name without its last extension"""
    return name[:-(len(name.split(".")[-1]) + 1)]


def dense_point_table(points_xyz, points_ids):
    """points3d_ordered of the script's __main__: float64 zeros [max id + 1, 3] with every point at the row of its id"""
    ids = np.asarray(points_ids, dtype=np.int64)
    table = np.zeros([int(ids.max()) + 1 if ids.size else 0, 3])
    if ids.size:
        table[ids] = np.asarray(points_xyz, dtype=np.float64)
    return table


def _map_f32(m):
    m = np.asarray(m)
    if m.ndim != 2 or m.dtype not in (np.uint16, np.float32) or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("a mono map is uint16 or float32 [h,w] (got %s %s)" % (m.dtype, m.shape))
    return m.astype(np.float32) / (2 ** 16)


# --------------------------------------------------------------------------------------------------- the sample
def _cells(x, n, coord_bits):
    if coord_bits is None:
        fl = np.floor(x)
        cell, f = fl.astype(np.int64), x - fl
    else:
        q = np.float32(1 << coord_bits)
        i = np.rint(x * q).astype(np.int64)
        cell, f = i >> coord_bits, (i & ((1 << coord_bits) - 1)).astype(np.float32) / q
    return np.clip(cell, 0, n - 1), np.clip(cell + 1, 0, n - 1), f


def sample_bilinear(mono_map, x, y, coord_bits=COORD_BITS):
    """mono_map float32 [h,w], x / y float32 [n] -> float32 [n]: the stated rule of the module's docstring"""
    mono_map, x, y = np.asarray(mono_map, np.float32), np.asarray(x, np.float32), np.asarray(y, np.float32)
    h, w = mono_map.shape
    x0, x1, fx = _cells(x, w, coord_bits)
    y0, y1, fy = _cells(y, h, coord_bits)
    one = np.float32(1)
    gx, gy = one - fx, one - fy
    acc = (gy * gx) * mono_map[y0, x0]
    acc = acc + (gy * fx) * mono_map[y0, x1]
    acc = acc + (fy * gx) * mono_map[y1, x0]
    acc = acc + (fy * fx) * mono_map[y1, x1]
    return acc


# --------------------------------------------------------------------------------------------------- the fit, host
def _zero_stats(n_valid=0):
    return dict(scale=0, offset=0, n_valid=int(n_valid), t_colmap=0.0, s_colmap=0.0, t_mono=0.0, s_mono=0.0)


def fit_image_numpy(image, cam, table, mono, coord_bits=COORD_BITS):
    """get_scales for one image whose map is there -> the STAT_KEYS dict (scale = offset = 0 where the gate fails)"""
    ids = np.asarray(image.point3D_ids, dtype=np.int64)
    used = ids >= 0
    used = used * (ids < len(table))
    ids, xys = ids[used], np.asarray(image.xys, dtype=np.float64).reshape(-1, 2)[used]
    if len(ids) == 0:    # (the script's stand-in point: no observation is valid)
        return _zero_stats()
    R, t = gio.qvec2rotmat(image.qvec), np.asarray(image.tvec, dtype=np.float64)
    pts = table[ids]
    mono_map = _map_f32(mono)
    width, height = int(cam.width), int(cam.height)
    with np.errstate(all="ignore"):
        z = ((pts[:, 0] * R[2, 0] + pts[:, 1] * R[2, 1]) + pts[:, 2] * R[2, 2]) + t[2]
        inv = 1. / z
        s = mono_map.shape[0] / height
        maps = (xys * s).astype(np.float32)
        valid = ((maps[..., 0] >= 0) * (maps[..., 1] >= 0) * (maps[..., 0] < width * s) * (maps[..., 1] < height * s) * (inv > 0))
        n_valid = int(valid.sum())
        if not (n_valid > 10 and (inv.max() - inv.min()) > 1e-3):
            return _zero_stats(n_valid)
        maps, inv = maps[valid, :], inv[valid]
        sampled = sample_bilinear(mono_map, maps[..., 0], maps[..., 1], coord_bits)
        t_colmap = np.median(inv)
        s_colmap = np.mean(np.abs(inv - t_colmap))
        t_mono = np.median(sampled)
        s_mono = np.mean(np.abs(sampled - t_mono))
        scale = s_colmap / s_mono
        offset = t_colmap - t_mono * scale
    return dict(scale=float(scale), offset=float(offset), n_valid=n_valid, t_colmap=float(t_colmap), s_colmap=float(s_colmap),
                t_mono=float(t_mono), s_mono=float(s_mono))


# --------------------------------------------------------------------------------------------------- the fit, device
def _as_device_map(m, device, as_f32):
    m = np.ascontiguousarray(m)
    if as_f32:
        return torch.from_numpy(m.astype(np.float32)).to(device)
    return torch.from_numpy(m.view(np.int16)).to(device)   # (the uint16 bits)


def pack_device_inputs(items, table, device):
    """items: [(image, cam, map)] -> (the device tensors gs_depth_scales reads, n_obs, map dtype).  The dict also keeps the
    maps alive: the pointer array refers to them."""
    n = len(items)
    as_f32 = any(np.asarray(m).dtype != np.uint16 for _, _, m in items)
    ids, xys, seg, cams, hw, keep = [], [], [0], np.zeros((n, 8)), np.zeros((n, 2), dtype=np.int32), []
    for k, (image, cam, m) in enumerate(items):
        m = np.asarray(m)
        if m.ndim != 2 or m.dtype not in (np.uint16, np.float32) or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError("a mono map is uint16 or float32 [h,w] (got %s %s)" % (m.dtype, m.shape))
        i = np.asarray(image.point3D_ids, dtype=np.int64).reshape(-1)
        ids.append(i)
        xys.append(np.asarray(image.xys, dtype=np.float64).reshape(-1, 2))
        seg.append(seg[-1] + i.shape[0])
        R, s = gio.qvec2rotmat(image.qvec), m.shape[0] / int(cam.height)
        cams[k] = (R[2, 0], R[2, 1], R[2, 2], float(image.tvec[2]), s, np.float32(int(cam.width) * s),
                   np.float32(int(cam.height) * s), 0.0)
        hw[k] = m.shape
        keep.append(_as_device_map(m, device, as_f32))
    n_obs = seg[-1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    t = dict(ids=dev(np.concatenate(ids) if n_obs else np.zeros((1,), dtype=np.int64)),
             xys=dev(np.concatenate(xys) if n_obs else np.zeros((1, 2))),
             table=dev(np.asarray(table, dtype=np.float64) if len(table) else np.zeros((1, 3))),
             seg=dev(np.array(seg, dtype=np.int64)), cams=dev(cams), hw=dev(hw), maps=keep,
             ptrs=dev(np.array([m.data_ptr() for m in keep], dtype=np.int64)))
    return t, n_obs, MAP_F32 if as_f32 else MAP_U16


def fit_images_device(items, table, coord_bits=COORD_BITS, device="cuda"):
    """items: [(image, cam, map)] -> [STAT_KEYS dict], one gs_depth_scales launch for all of them"""
    from ._lib import hip_api
    api = hip_api()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("depth_scales(on_device=True) needs a GPU device - the host numpy path is on_device=False")
    n = len(items)
    if n == 0:
        return []
    if coord_bits is not None and not 0 <= int(coord_bits) <= 10:
        raise ValueError("coord_bits: None or 0..10 (got %r)" % (coord_bits,))
    t, n_obs, dtype = pack_device_inputs(items, table, device)
    nb = int(api.raw("depth_scales_tmp_bytes")(n_obs))
    tmp = torch.empty((nb,), dtype=torch.uint8, device=device)
    out = torch.empty((n, 8), dtype=torch.float64, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    api.call("depth_scales", t["table"].data_ptr(), len(table), t["ids"].data_ptr(), t["xys"].data_ptr(), n_obs,
             t["seg"].data_ptr(), t["cams"].data_ptr(), t["ptrs"].data_ptr(), t["hw"].data_ptr(), dtype,
             -1 if coord_bits is None else int(coord_bits), n, tmp.data_ptr(), nb, out.data_ptr(), stream)
    res = out.cpu().numpy()   # (the read-back waits for the launch; the inputs above stay alive until here)
    stats = []
    for row in res:
        d = dict(zip(STAT_KEYS, (float(v) for v in row[:7])))
        d["n_valid"] = int(row[2])
        if d["scale"] == 0 and d["offset"] == 0 and d["s_mono"] == 0:   # the gate failed: the script's integer zeros
            d["scale"], d["offset"] = 0, 0
        stats.append(d)
    return stats


# --------------------------------------------------------------------------------------------------- public
def depth_scales(images, intrinsics, points_xyz, points_ids, maps, on_device=False, coord_bits=COORD_BITS,
                 return_stats=False, device="cuda"):
    """images / intrinsics: what io.read_extrinsics_* / read_intrinsics_* return; points_xyz [N,3], points_ids [N]: the model's
    points and their ids (io.read_points3D_*(with_ids=True)); maps: {key: uint16 or float32 [h,w] map, or None} with
    key = the image's name without its extension.  A uint16 map holds the file's samples, a float32 one the same values as
    floats: both are divided by 2**16.  -> {key: {"scale": ..., "offset": ...}} in the images' order; an image whose map is
    None or missing is left out, as the script's `return None` does.  return_stats: every entry also holds n_valid, both
    medians and both deviations."""
    table = dense_point_table(points_xyz, points_ids)
    todo = []
    for image_id in images:
        image = images[image_id]
        key = image_key(image.name)
        if maps.get(key) is not None:
            todo.append((key, image, intrinsics[image.camera_id], maps[key]))
    if on_device:
        stats = fit_images_device([(i, c, m) for _, i, c, m in todo], table, coord_bits, device)
    else:
        stats = [fit_image_numpy(i, c, table, m, coord_bits) for _, i, c, m in todo]
    keys = STAT_KEYS if return_stats else ("scale", "offset")
    return {key: {k: st[k] for k in keys} for (key, _, _, _), st in zip(todo, stats)}


def make_depth_params(base_dir, depths_dir, model_type="bin", on_device=False, device="cuda"):
    """The script's __main__: reads base_dir/sparse/0 (model_type "bin" or "txt") and depths_dir/<image key>.png, writes
    base_dir/sparse/0/depth_params.json (indent=2) and returns its dict."""
    sparse = os.path.join(base_dir, "sparse", "0")
    if model_type == "bin":
        cams = gio.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
        images = gio.read_extrinsics_binary(os.path.join(sparse, "images.bin"))
        xyz, _, _, ids = gio.read_points3D_binary(os.path.join(sparse, "points3D.bin"), with_ids=True)
    elif model_type == "txt":
        cams = gio.read_intrinsics_text(os.path.join(sparse, "cameras.txt"))
        images = gio.read_extrinsics_text(os.path.join(sparse, "images.txt"))
        xyz, _, _, ids = gio.read_points3D_text(os.path.join(sparse, "points3D.txt"), with_ids=True)
    else:
        raise ValueError("make_depth_params: model_type is \"bin\" or \"txt\" (got %r)" % (model_type,))
    maps = {}
    for image in images.values():
        key = image_key(image.name)
        path = os.path.join(depths_dir, key + ".png")
        maps[key] = _read_depth_file(path) if os.path.exists(path) else None
    params = depth_scales(images, cams, xyz, ids, maps, on_device=on_device, device=device)
    with open(os.path.join(sparse, "depth_params.json"), "w") as f:
        json.dump(params, f, indent=2)
    return params


def _read_depth_file(path):
    m = read_png16(path)
    if m.ndim != 2:
        raise ValueError("%s has %d channels - a depth file is one grey channel (cv2 would take its channel 0, the file's last "
                         "colour channel: an order that is not restated here)" % (path, m.shape[2]))
    return m


def read_depth_params(path):
    """dataset_readers.py:157-170: depth_params.json with med_scale = the median of the positive scales (0 when there are
    none) added to every entry"""
    with open(path, "r") as f:
        params = json.load(f)
    all_scales = np.array([params[key]["scale"] for key in params])
    med_scale = float(np.median(all_scales[all_scales > 0])) if (all_scales > 0).sum() else 0
    for key in params:
        params[key]["med_scale"] = med_scale
    return params


# --------------------------------------------------------------------------------------------------- the camera's map
def _axis(n_in, n_out):
    d = np.arange(n_out, dtype=np.float64)
    f = ((d + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    fl = np.floor(f)
    s, f = fl.astype(np.int64), f - fl
    low, high = s < 0, s >= n_in - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), np.float32(1) - f, f


def resize_bilinear_numpy(src, size):
    """src float32 [H,W] -> float32 [H2,W2], size = (W2, H2): the stated rule of the module's docstring"""
    src = np.asarray(src, dtype=np.float32)
    W2, H2 = int(size[0]), int(size[1])
    H, W = src.shape
    if (H2, W2) == (H, W):
        return src.copy()
    x0, x1, a0, a1 = _axis(W, W2)
    y0, y1, b0, b1 = _axis(H, H2)
    rows = a0[None, :] * src[:, x0] + a1[None, :] * src[:, x1]
    return b0[:, None] * rows[y0] + b1[:, None] * rows[y1]


def reliability(depth_params):
    """-> (reliable, apply): cameras.py:68-74's two tests on a depth_params entry (None: reliable, nothing applied)"""
    if depth_params is None:
        return True, False
    scale, med = depth_params["scale"], depth_params["med_scale"]
    return not (scale < 0.2 * med or scale > 5 * med), bool(scale > 0)


def prepare_invdepth(map, resolution, depth_params=None, divisor=65536.0, device=None):
    """map: uint16 or float32 [H,W] samples (numpy array or tensor); resolution = (W2, H2); depth_params: the camera's entry
    of read_depth_params, or None -> (invdepth float32 [1,H2,W2], depth_mask float32 [1,H2,W2], reliable) as
    scene/cameras.py:60-78 leaves them.  A CUDA tensor (or device="cuda") goes through gs_invdepth_prepare and stays on the
    device; everything else takes the numpy path and returns CPU tensors."""
    W2, H2 = int(resolution[0]), int(resolution[1])
    if W2 < 1 or H2 < 1:
        raise ValueError("prepare_invdepth: resolution = (W2, H2) with both >= 1 (got %r)" % (resolution,))
    reliable, apply = reliability(depth_params)
    scale = np.float32(depth_params["scale"]) if apply else np.float32(1)
    offset = np.float32(depth_params["offset"]) if apply else np.float32(0)
    on_gpu = (torch.is_tensor(map) and map.is_cuda) or (device is not None and torch.device(device).type == "cuda")
    if on_gpu:
        if not torch.is_tensor(map):
            m = np.ascontiguousarray(map)
            if m.dtype not in (np.uint16, np.float32) or m.ndim != 2:
                raise ValueError("prepare_invdepth: uint16 or float32 [H,W] (got %s %s)" % (m.dtype, m.shape))
            is_u16 = m.dtype == np.uint16
            map = torch.from_numpy(m.view(np.int16) if is_u16 else m).to(device)
        else:
            is_u16 = map.dtype in (torch.int16, getattr(torch, "uint16", torch.int16))
            if (not is_u16 and map.dtype != torch.float32) or map.dim() != 2:
                raise ValueError("prepare_invdepth: uint16 or float32 [H,W] (got %s %s)" % (map.dtype, tuple(map.shape)))
            map = map.contiguous()
        from ._lib import hip_api
        H, W = int(map.shape[0]), int(map.shape[1])
        inv = torch.empty((1, H2, W2), dtype=torch.float32, device=map.device)
        mask = torch.empty((1, H2, W2), dtype=torch.float32, device=map.device)
        stream = torch.cuda.current_stream(map.device).cuda_stream
        hip_api().call("invdepth_prepare", map.data_ptr(), MAP_U16 if is_u16 else MAP_F32, H, W, H2, W2, float(divisor),
                       int(apply), float(scale), float(offset), 1.0 if reliable else 0.0, inv.data_ptr(), mask.data_ptr(), stream)
        return inv, mask, reliable
    m = map.numpy() if torch.is_tensor(map) else np.asarray(map)
    if m.dtype == np.int16:
        m = m.view(np.uint16)
    if m.dtype not in (np.uint16, np.float32) or m.ndim != 2:
        raise ValueError("prepare_invdepth: uint16 or float32 [H,W] (got %s %s)" % (m.dtype, m.shape))
    x = resize_bilinear_numpy(m.astype(np.float32) / np.float32(divisor), (W2, H2))
    x[x < 0] = 0
    if apply:
        x = x * scale + offset
    mask = np.ones((1, H2, W2), dtype=np.float32)
    if not reliable:
        mask *= 0
    return torch.from_numpy(np.ascontiguousarray(x[None])), torch.from_numpy(mask), reliable


def load_depth_priors(keys, depths_dir, depth_params, resolutions, nerf_synthetic=False, device="cpu"):
    """keys: per camera the image's name without extension; resolutions: per camera (W, H); depth_params: read_depth_params'
    dict or None -> the list Trainer.depth_priors takes: None where depths_dir/<key>.png is absent or the camera is not
    depth_reliable (train.py:206), else (invdepth [1,H,W] on `device`, None) - the mask of a reliable camera is all ones, which
    the trainer takes as None.  nerf_synthetic: the samples are divided by 512 instead of 2**16 (camera_utils.py:26)."""
    device = torch.device(device)
    out = []
    for key, res in zip(keys, resolutions):
        path = os.path.join(depths_dir, key + ".png")
        if not os.path.exists(path):
            out.append(None)
            continue
        entry = None if depth_params is None else depth_params.get(key)
        inv, _, reliable = prepare_invdepth(_read_depth_file(path), res, entry, 512.0 if nerf_synthetic else 65536.0,
                                            device=device if device.type == "cuda" else None)
        out.append((inv.to(device), None) if reliable else None)
    return out
