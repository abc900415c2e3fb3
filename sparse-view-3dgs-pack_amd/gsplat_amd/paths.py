"""Camera paths for novel-view rendering and pseudo views: host, numpy, float64, operation for operation what the reference
computes (tests/golden/camera_paths.npz pins every generator to the reference's own functions at rtol 1e-12).

  FSGS/utils/pose_utils.py                 generate_spiral_path (LLFF poses_bounds rows), generate_ellipse_path,
                                           generate_random_poses_llff, generate_random_poses_360
  DNGaussian/utils/pose_utils.py           spiral_path_dng (its generate_spiral_path), generate_spiral_path_dtu, recenter_poses /
                                           backcenter_poses, convert_poses
  DNGaussian/scene/dataset_readers.py      create_llff_spiral / create_dtu_spiral = CreateLLFFSpiral / CreateDTUSpiral (:401-488)
                                           from the poses_bounds array instead of its file; -> (R, T, height, width, focal) as
                                           generateLLFFCameras (:374-395) reads them
  FSGS/render.py:71-73                     camera_from_pose
  pseudo_cameras / path_centres            what TrainerFSGS(pseudo_cameras=...) and TrainerDNG(near_centers=...) take

`views` are objects with R (camera-to-world rotation, as the reference stores it) and T (world-to-camera translation), or this
package's cameras (gsplat_amd.synthetic.Camera), whose world_view_transform holds both.  The random generators take an
np.random.RandomState: one seeded as np.random.seed(s) was reproduces the reference's draws (rand(3) per pose for LLFF, one
rand(n_frames) for 360).  The two FSGS look-at helpers differ from DNGaussian's only in the sign of subtract_position's
difference; both are kept."""
import numpy as np
import torch

from . import synthetic

_FIX_ROTATION = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
EPS32 = np.finfo(np.float32).eps


# ------------------------------------------------------------------------------------------------------ pose helpers
def normalize(x):
    return x / np.linalg.norm(x)


def viewmatrix(lookdir, up, position, subtract_position=False, dng=False):
    """Look-at matrix [3,4] with columns (x, y, z, position).  subtract_position: z along lookdir - position (FSGS) or
    position - lookdir (DNGaussian, dng=True)."""
    if subtract_position:
        lookdir = (position - lookdir) if dng else (lookdir - position)
    vec2 = normalize(lookdir)
    vec0 = normalize(np.cross(up, vec2))
    vec1 = normalize(np.cross(vec2, vec0))
    return np.stack([vec0, vec1, vec2, position], axis=1)


def poses_avg(poses):
    """The pose at the mean position with the mean z axis and the mean up vector"""
    return viewmatrix(poses[:, :3, 2].mean(0), poses[:, :3, 1].mean(0), poses[:, :3, 3].mean(0))


def pad_poses(p):
    bottom = np.broadcast_to([0, 0, 0, 1.], p[..., :1, :4].shape)
    return np.concatenate([p[..., :3, :4], bottom], axis=-2)


def unpad_poses(p):
    return p[..., :3, :4]


def recenter_poses(poses):
    """-> (poses in the frame of poses_avg, the 4 x 4 transform applied)"""
    transform = np.linalg.inv(pad_poses(poses_avg(poses)))
    return unpad_poses(transform @ pad_poses(poses)), transform


def backcenter_poses(poses, pose_ref):
    return unpad_poses(pad_poses(poses_avg(pose_ref)) @ pad_poses(poses))


def focus_point_fn(poses):
    """The point nearest to all the poses' optical axes"""
    directions, origins = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - directions * np.transpose(directions, [0, 2, 1])
    mt_m = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mt_m.mean(0)) @ (mt_m @ origins).mean(0)[:, 0]


def transform_poses_pca(poses):
    """Poses [N,3,4] with their positions' principal axes on x, y, z, inside the unit cube -> (poses, 4 x 4 transform)"""
    t = poses[:, :3, 3]
    t_mean = t.mean(axis=0)
    t = t - t_mean
    eigval, eigvec = np.linalg.eig(t.T @ t)
    eigvec = eigvec[:, np.argsort(eigval)[::-1]]
    rot = eigvec.T
    if np.linalg.det(rot) < 0:
        rot = np.diag(np.array([1, 1, -1])) @ rot
    transform = np.concatenate([rot, rot @ -t_mean[:, None]], -1)
    recentred = unpad_poses(transform @ pad_poses(poses))
    transform = np.concatenate([transform, np.eye(4)[3:]], axis=0)
    if recentred.mean(axis=0)[2, 1] < 0:
        recentred = np.diag(np.array([1, -1, -1])) @ recentred
        transform = np.diag(np.array([1, -1, -1, 1])) @ transform
    scale_factor = 1. / np.max(np.abs(recentred[:, :3, 3]))
    recentred[:, :3, 3] *= scale_factor
    transform = np.diag(np.array([scale_factor] * 3 + [1])) @ transform
    return recentred, transform


def _rt(view):
    if hasattr(view, "R") and hasattr(view, "T"):
        return np.asarray(view.R), np.asarray(view.T)
    w2c = np.asarray(view.world_view_transform.detach().cpu().numpy(), dtype=np.float64).T
    return w2c[:3, :3].T, w2c[:3, 3]


def view_poses(views):
    """[N,4,4] camera-to-world in the y-up / z-back convention the path generators work in"""
    poses = []
    for view in views:
        R, T = _rt(view)
        m = np.eye(4)
        m[:3] = np.concatenate([R.T, T[:, None]], 1)
        m = np.linalg.inv(m)
        m[:, 1:3] *= -1
        poses.append(m)
    return np.stack(poses, 0)


def _focus_depth(bounds):
    close_depth, inf_depth = bounds.min() * .9, bounds.max() * 5.
    dt = .75
    return 1 / (((1 - dt) / close_depth + dt / inf_depth))


def _to_world(pose34, transform, scale=None):
    """a path pose in the generator's frame -> the reference's render pose: world-to-camera, y down / z forward"""
    m = np.eye(4)
    m[:3] = pose34
    m = np.linalg.inv(transform) @ m
    m[:3, 1:3] *= -1
    if scale is not None:
        m[:3, 3] /= scale
    return np.linalg.inv(m)


# ------------------------------------------------------------------------------------------------------ FSGS generators
def _llff_frame(poses, bounds):
    scale = 1. / (bounds.min() * .75)
    poses[:, :3, 3] *= scale
    bounds = bounds * scale
    poses, transform = recenter_poses(poses)
    return poses, bounds, transform, scale


def generate_spiral_path(poses_arr, n_frames=180, n_rots=2, zrate=.5):
    """poses_arr: the rows of an LLFF poses_bounds.npy [N,17] -> world-to-camera poses [n_frames,4,4] (render.py --video on
    llff scenes).  The input is not modified."""
    poses_arr = np.array(poses_arr, copy=True)
    poses = poses_arr[:, :-2].reshape([-1, 3, 5])
    poses = poses[:, :3, :4] @ _FIX_ROTATION
    poses, bounds, transform, scale = _llff_frame(poses, poses_arr[:, -2:])
    focal = _focus_depth(bounds)
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 90, 0), [1.]])
    cam2world = poses_avg(poses)
    up = poses[:, :3, 1].mean(0)
    out = []
    for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
        position = cam2world @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
        lookat = cam2world @ [0, 0, -focal, 1.]
        out.append(_to_world(viewmatrix(position - lookat, up, position), transform, scale))
    return np.stack(out, axis=0)


def _ellipse(poses, z_variation, z_phase):
    center = focus_point_fn(poses)
    offset = np.array([center[0], center[1], 0])
    sc = np.percentile(np.abs(poses[:, :3, 3] - offset), 90, axis=0)
    low, high = -sc + offset, sc + offset
    z_low = np.percentile((poses[:, :3, 3]), 10, axis=0)
    z_high = np.percentile((poses[:, :3, 3]), 90, axis=0)

    def get_positions(theta):
        return np.stack([(low[0] + (high - low)[0] * (np.cos(theta) * .5 + .5)),
                         (low[1] + (high - low)[1] * (np.sin(theta) * .5 + .5)),
                         z_variation * (z_low[2] + (z_high - z_low)[2] * (np.cos(theta + 2 * np.pi * z_phase) * .5 + .5))], -1)
    avg_up = poses[:, :3, 1].mean(0)
    avg_up = avg_up / np.linalg.norm(avg_up)
    ind_up = np.argmax(np.abs(avg_up))
    up = np.eye(3)[ind_up] * np.sign(avg_up[ind_up])
    return center, up, get_positions


def _resample_const_speed(theta, lengths, n):
    """FSGS/utils/stepfun.py's sample_np(None, theta, log(lengths), n): n points spaced evenly in arc length"""
    w_logits = np.log(lengths)
    u = np.linspace(0, 1. - EPS32, n)
    w = np.exp(w_logits) / np.exp(w_logits).sum(axis=-1, keepdims=True)
    cw = np.minimum(1, np.cumsum(w[..., :-1], axis=-1))
    cw0 = np.concatenate([np.zeros(cw.shape[:-1] + (1,)), cw, np.ones(cw.shape[:-1] + (1,))], axis=-1)
    return np.interp(u, cw0, theta)


def generate_ellipse_path(views, n_frames=600, const_speed=True, z_variation=0., z_phase=0.):
    """-> list of n_frames world-to-camera poses [4,4] on an ellipse around the views' focus point (render.py --video on 360
    scenes)"""
    poses, transform = transform_poses_pca(view_poses(views))
    center, up, get_positions = _ellipse(poses, z_variation, z_phase)
    theta = np.linspace(0, 2. * np.pi, n_frames + 1, endpoint=True)
    positions = get_positions(theta)
    if const_speed:
        lengths = np.linalg.norm(positions[1:] - positions[:-1], axis=-1)
        positions = get_positions(_resample_const_speed(theta, lengths, n_frames + 1))
    return [_to_world(viewmatrix(p - center, up, p), transform) for p in positions[:-1]]


def generate_random_poses_llff(views, bounds, rng, n_poses=10000):
    """views with their depth bounds [N,2] -> [n_poses,4,4] world-to-camera poses in the box the training cameras span.
    rng: np.random.RandomState, three uniform draws per pose."""
    poses, bounds, transform, scale = _llff_frame(view_poses(views), np.array(bounds, dtype=np.float64))
    focal = _focus_depth(bounds)
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 100, 0), [1.]])
    cam2world = poses_avg(poses)
    up = poses[:, :3, 1].mean(0)
    out = []
    for _ in range(n_poses):
        position = cam2world @ (radii * np.concatenate([2 * rng.rand(3) - 1., [1, ]]))
        lookat = cam2world @ [0, 0, -focal, 1.]
        out.append(_to_world(viewmatrix(position - lookat, up, position), transform, scale))
    return np.stack(out, axis=0)


def generate_random_poses_360(views, rng, n_frames=10000, z_variation=0.1, z_phase=0):
    """-> list of n_frames - 1 world-to-camera poses at random angles of generate_ellipse_path's ellipse (the reference drops
    the last draw).  rng: np.random.RandomState, one draw of n_frames."""
    poses, transform = transform_poses_pca(view_poses(views))
    center, up, get_positions = _ellipse(poses, z_variation, z_phase)
    positions = get_positions(rng.rand(n_frames) * 2. * np.pi)[:-1]
    return [_to_world(viewmatrix(p - center, up, p), transform) for p in positions]


# ------------------------------------------------------------------------------------------------ DNGaussian generators
def spiral_path_dng(poses, bounds, n_frames=120, n_rots=2, zrate=.5):
    """DNGaussian's generate_spiral_path: recentred poses [N,3,4] and bounds -> camera-to-world [n_frames,3,4]"""
    focal = _focus_depth(bounds)
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 90, 0), [1.]])
    cam2world = poses_avg(poses)
    up = poses[:, :3, 1].mean(0)
    out = []
    for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
        position = cam2world @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
        lookat = cam2world @ [0, 0, -focal, 1.]
        out.append(viewmatrix(position - lookat, up, position))
    return np.stack(out, axis=0)


def generate_spiral_path_dtu(poses, n_frames=120, n_rots=2, zrate=.5, perc=60):
    """Recentred, unit-scaled poses [N,3,4] -> camera-to-world [n_frames,3,4] looking at the poses' focus point"""
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), perc, 0), [1.]])
    cam2world = poses_avg(poses)
    up = poses[:, :3, 1].mean(0)
    z_axis = focus_point_fn(poses)
    out = []
    for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
        position = cam2world @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
        out.append(viewmatrix(z_axis, up, position, True, dng=True))
    return np.stack(out, axis=0)


def convert_poses(poses):
    """LLFF-layout poses [3,5,N] -> (Rs [N,3,3] world-to-camera, tvecs [N,3], H, W, focal)"""
    poses = np.concatenate([poses[:, 1:2], poses[:, 0:1], -poses[:, 2:3], poses[:, 3:4], poses[:, 4:5]], 1).transpose(2, 0, 1)
    bottom = np.tile(np.array([0, 0, 0, 1.]).reshape([1, 1, 4]), (poses.shape[0], 1, 1))
    H, W, fl = poses[0, :, -1]
    poses = np.linalg.inv(np.concatenate([poses[..., :4], bottom], 1))
    return poses[:, :3, :3], poses[:, :3, -1], H, W, fl


def _spiral_cameras(render_poses, poses_o):
    inv_rotation = np.linalg.inv(_FIX_ROTATION)
    render_poses = render_poses @ inv_rotation
    render_poses = np.concatenate([render_poses, np.tile(poses_o[:1, :3, 4:], (render_poses.shape[0], 1, 1))], -1)
    Rs, tvecs, height, width, focal = convert_poses(render_poses.transpose([1, 2, 0]))
    return dict(R=np.stack([np.transpose(r) for r in Rs]), T=tvecs, height=height, width=width, focal=focal,
                FovY=synthetic.focal2fov(focal, height), FovX=synthetic.focal2fov(focal, width))


def create_llff_spiral(poses_arr, n_frames=180):
    """CreateLLFFSpiral on the poses_bounds array [N,17] -> dict(R [n,3,3] as the reference stores it (transposed), T [n,3],
    height, width, focal, FovX, FovY): spiral.py's render cameras on LLFF scenes"""
    poses_arr = np.asarray(poses_arr)
    poses_o = poses_arr[:, :-2].reshape([-1, 3, 5])
    poses = poses_o[:, :3, :4] @ _FIX_ROTATION
    render_poses = spiral_path_dng(recenter_poses(poses)[0], poses_arr[:, -2:], n_frames=n_frames)
    return _spiral_cameras(backcenter_poses(render_poses, poses), poses_o)


def create_dtu_spiral(poses_arr, n_frames=180):
    """CreateDTUSpiral on the poses_bounds array [N,17]; returns as create_llff_spiral"""
    poses_arr = np.asarray(poses_arr)
    poses_o = poses_arr[:, :-2].reshape([-1, 3, 5])
    poses = poses_o[:, :3, :4] @ _FIX_ROTATION
    render_poses = recenter_poses(poses)[0]
    s = np.max(np.abs(render_poses[:, :3, -1]))
    render_poses[:, :3, -1] /= s
    render_poses = generate_spiral_path_dtu(render_poses, n_frames=n_frames)
    render_poses[:, :3, -1] *= s
    return _spiral_cameras(backcenter_poses(render_poses, poses), poses_o)


# ------------------------------------------------------------------------------------------------------------ cameras
def world_to_view(R, t, translate=np.array([.0, .0, .0]), scale=1.0):
    """The reference's getWorld2View2 (utils/graphics_utils.py): [R^T | t] with the camera centre moved by (c + translate) *
    scale, through its two inversions, as float32"""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = np.asarray(R).transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    C2W[:3, 3] = (C2W[:3, 3] + translate) * scale
    return np.float32(np.linalg.inv(C2W))


def camera_from_pose(template, pose, trans=np.array([.0, .0, .0]), scale=1.0, znear=0.01, zfar=100.0):
    """FSGS/render.py:71-73: the template camera moved to a world-to-camera `pose` [4,4] (a generator's output): world-view
    transform, full projection and centre from the pose, size and field of view from the template -> synthetic.Camera"""
    pose = np.asarray(pose)
    wvt = torch.tensor(world_to_view(pose[:3, :3].T, pose[:3, 3], trans, scale)).transpose(0, 1)
    proj = synthetic.perspective(znear, zfar, template.FoVx, template.FoVy).transpose(0, 1)
    full = (wvt.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
    center = wvt.inverse()[3, :3]
    return synthetic.Camera(int(template.image_height), int(template.image_width), float(template.FoVx), float(template.FoVy),
                            wvt.contiguous(), full.contiguous(), center.contiguous())


def camera_from_rt(template, R, T, FoVx=None, FoVy=None):
    """A create_*_spiral entry (R stored transposed, T) -> synthetic.Camera of the template's size"""
    return synthetic.make_camera(R, T, template.FoVx if FoVx is None else FoVx, template.FoVy if FoVy is None else FoVy,
                                 template.image_width, template.image_height)


def pseudo_cameras(train_cameras, kind, rng, bounds=None, n_poses=10000):
    """The pseudo views FSGS's scene builds beside the training cameras (scene/__init__.py): kind "llff" (needs the views'
    depth bounds [N,2]) or "360".  -> list of cameras for TrainerFSGS(pseudo_cameras=...), intrinsics of the first camera."""
    if kind == "llff":
        if bounds is None:
            raise ValueError("pseudo_cameras: kind 'llff' needs the training views' depth bounds")
        poses = generate_random_poses_llff(train_cameras, bounds, rng, n_poses=n_poses)
    elif kind == "360":
        poses = generate_random_poses_360(train_cameras, rng, n_frames=n_poses)
    else:
        raise ValueError("pseudo_cameras: kind is 'llff' or '360' (got %r)" % (kind,))
    return [camera_from_pose(train_cameras[0], p) for p in poses]


def path_centres(cameras):
    """-> float32 [K,3], the cameras' centres: TrainerDNG(near_centers=...) and render_set.prune_for_path"""
    if len(cameras) == 0:
        return torch.zeros((0, 3), dtype=torch.float32)
    return torch.stack([torch.as_tensor(c.camera_center, dtype=torch.float32).reshape(3).cpu() for c in cameras])
