"""The `dc=` / `shs=` rasterizer call against the concatenated call on the same numbers: shared by
tests/test_sparse_gaussian_adam_cpu.py (fall-back path, CPU checker) and tests/test_gpu_rasterizer_dc.py (gs_backward_split)."""
import torch

from gsplat_amd import synthetic
from helpers import settings_for

GEOMETRY = ("means3D", "means2D", "opacities", "scales", "rotations", "cov3D_precomp")


def inside_camera(W, H):
    """A camera INSIDE the scene's cube (synthetic._points: +-1.3): a share of the Gaussians lies behind it."""
    return synthetic.look_at_camera((0.1, -0.2, 0.15), W, H, target=(1.3, 0.3, 0.0))


def scene_rows(P, K, seed=0, max_degree=3):
    """trained_like's activated tensors with the SH rows cut to 1 + K coefficients."""
    n = max(P, 16)   # (the synthetic scales come from three nearest neighbours: a tiny model is cut out of a larger one)
    sc = synthetic.trained_like(n, seed=seed, sh_degree=max_degree)
    if n != P:       # ... its rows furthest along +x, where inside_camera looks
        rows = torch.argsort(sc["means3D"][:, 0], descending=True)[:P]
        sc = {k: (v[rows].contiguous() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == n else v) for k, v in sc.items()}
    sc["shs"] = sc["shs"][:, :1 + K, :].contiguous()
    return sc


def covariances(sc):
    """[P,6] upper triangles of R S S^T R^T (what the rasterizer builds from scales and rotations)."""
    q = torch.nn.functional.normalize(sc["rotations"].double())
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * sc["scales"].double()[:, None, :]
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()


def run(Rasterizer, Settings, sc, cam, device, degree, split, antialiasing=False, use_depth=False, camera_key=None,
        precomputed_cov=False, visits=1):
    """Render and backpropagate a fixed image gradient.  split: the call is rasterizer(dc=shs[:, :1], shs=shs[:, 1:], ...),
    else rasterizer(shs=shs, ...).  Returns dict(color, radii, invdepth, grads{...}) of the LAST visit, with the SH gradient
    as grads["dc"], grads["rest"] in both forms."""
    out = None
    for _ in range(visits):
        p = {k: sc[k].detach().clone().to(device).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
        cov = covariances(sc).to(device).requires_grad_(True) if precomputed_cov else None
        means2D = torch.zeros_like(p["means3D"], requires_grad=True)
        rs = settings_for(Settings, cam, torch.tensor([0.1, 0.2, 0.3]), degree, device, antialiasing)
        rast = Rasterizer(raster_settings=rs)
        if camera_key is not None:
            rast.camera_key = camera_key
        geometry = dict(means3D=p["means3D"], means2D=means2D, opacities=p["opacities"], colors_precomp=None,
                        scales=None if precomputed_cov else p["scales"], rotations=None if precomputed_cov else p["rotations"],
                        cov3D_precomp=cov)
        if split:
            dc = sc["shs"][:, :1, :].detach().clone().contiguous().to(device).requires_grad_(True)
            rest = sc["shs"][:, 1:, :].detach().clone().contiguous().to(device).requires_grad_(True)
            color, radii, invdepth = rast(dc=dc, shs=rest, **geometry)
        else:
            shs = sc["shs"].detach().clone().to(device).requires_grad_(True)
            color, radii, invdepth = rast(shs=shs, **geometry)
        H, W = cam.image_height, cam.image_width
        g = torch.Generator().manual_seed(99)
        loss = (color * torch.randn((3, H, W), generator=g).to(device)).sum()
        if use_depth:
            loss = loss + (invdepth * torch.randn((1, H, W), generator=g).to(device)).sum()
        loss.backward()
        grads = {"means2D": means2D.grad, "cov3D_precomp": None if cov is None else cov.grad}
        grads.update({k: v.grad for k, v in p.items()})
        if split:
            grads["dc"], grads["rest"] = dc.grad, rest.grad
        else:
            grads["dc"], grads["rest"] = shs.grad[:, :1, :], shs.grad[:, 1:, :]
        out = dict(color=color.detach().cpu(), radii=radii.detach().cpu(), invdepth=invdepth.detach().cpu(),
                   grads={k: (None if v is None else v.detach().cpu()) for k, v in grads.items()})
    return out


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape:
        return False
    if a.dtype.is_floating_point:
        return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))
    return bool(torch.equal(a, b))


def assert_same(split, cat, what, precomputed_cov=False):
    """Image, radii, inverse depth and every gradient of the split call are the concatenated call's bit for bit."""
    for k in ("color", "radii", "invdepth"):
        assert same_bits(split[k], cat[k]), "%s: %s differs" % (what, k)
    names = ["dc", "rest", "means3D", "means2D", "opacities"] + (["cov3D_precomp"] if precomputed_cov else ["scales", "rotations"])
    for k in names:
        a, b = split["grads"][k], cat["grads"][k]
        if a is None and b is not None and b.numel() == 0:   # (a [P,0,3] tensor takes no gradient)
            continue
        assert a is not None and b is not None, "%s: no gradient for %s" % (what, k)
        assert same_bits(a, b), "%s: dL/d%s differs at %d of %d elements" % (
            what, k, int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum()) if a.shape == b.shape else -1,
            a.numel())
