"""gs_depth_vis (csrc/gs_depth_vis.hip) on the GPU against tests/golden/depth_vis.npz - what the reference's own visualize_cmap
and vis_depth gave on the CPU (tests/golden/make_golden_paths.py) - and against the torch statements of render.py:121,124.

  bounds    lo and hi equal the fixture's float64 BITS on every case: the select is exact and the interpolation the same double
            operations.  One reading of "bits": a NaN bound compares as NaN - IEEE 754 leaves the sign and payload of a
            generated NaN to the implementation (x86's 0/0 is the negative quiet NaN the fixture holds, gfx950's the positive one).
  bytes     "fsgs" and "identity": equal everywhere.  "dng": the reference takes numpy's float32 log of a pixel, the device the
            double logarithm rounded once.  The two were measured on every case image on the CPU (test_depth_vis_cpu.py
            re-measures): at most 3 ulp of the curve's value apart, doubled to depth_vis_cases.LOG_ULP_ALLOW = 6.  A pixel may
            differ from the fixture only if its float64 256 v lies within delta = 256 * 6 ulp / |curve(hi) - curve(lo)| of an
            interior integer 1..255, and must then take an adjacent table row; at most 0.5 % of a case's pixels are so placed
            (the CPU test holds the fixtures to that).  Pixels clipped to either end are never exempt.
The number of pixels that did differ goes to the file DEPTH_VIS_PARITY_OUT names, when it is set (profiles/depth_vis_parity.json
is one such run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import depth_vis_cases as dc
from gsplat_amd import depth_vis as dv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
CASES = dc.cases()
PAIRS = [(name, rule) for name, (_, _, rules) in CASES.items() for rule in rules]
DIFFERED = {}


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_vis.npz"))


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    out = os.environ.get("DEPTH_VIS_PARITY_OUT")
    if out and DIFFERED:
        json.dump(dict(log_ulp_measured_cpu=dc.LOG_ULP_MEASURED, log_ulp_allowance=dc.LOG_ULP_ALLOW,
                       max_exempt_fraction=dc.MAX_EXEMPT_FRACTION, dng_pixels_differing_on_gpu=DIFFERED), open(out, "w"), indent=1)


def dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def same_bits_nan_as_nan(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    for g, w in zip(got, want):
        if np.isnan(w):
            assert np.isnan(g), (got, want)
        else:
            assert g.view(np.int64) == w.view(np.int64), (got, want, float(g) - float(w))


@pytest.mark.parametrize("name,rule", PAIRS)
def test_bounds_and_bytes_against_the_reference(hip, z, name, rule):
    depth, alpha, _ = CASES[name]
    out, bounds = dv.colour_depth(dev(depth), dev(alpha), rule=rule, return_bounds=True)
    assert out.dtype == torch.uint8 and out.is_cuda and tuple(out.shape) == depth.shape + (3,)
    key = "%s_%s" % (name, rule)
    same_bits_nan_as_nan(bounds.cpu().numpy(), z[key + "_bounds"])
    got, want = out.cpu().numpy(), z[key + "_rgb"]
    diff = (got != want).any(axis=-1)
    print("%s: %d of %d pixels differ" % (key, int(diff.sum()), diff.size))
    if rule != "dng":
        assert not diff.any(), "%s: %d pixels differ" % (key, int(diff.sum()))
        return
    DIFFERED[name] = int(diff.sum())
    x = z[name + "_composite"] if alpha is not None else depth
    lo, hi = z[key + "_bounds"]
    exempt = dc.dng_exempt(x, z[key + "_v"], lo, hi)
    assert exempt.mean() <= dc.MAX_EXEMPT_FRACTION
    assert not (diff & ~exempt).any(), "%s: %d pixels differ outside the allowance" % (key, int((diff & ~exempt).sum()))
    if diff.any():   # an adjacent row's bytes
        idx = dv.table_index(z[key + "_v"])
        tab = dv.byte_tables()["save_image"]
        lower, upper = tab[np.clip(idx - 1, 0, 255)], tab[np.clip(idx + 1, 0, 255)]
        ok = (got == lower).all(axis=-1) | (got == upper).all(axis=-1)
        assert ok[diff].all()


@pytest.mark.parametrize("name", [n for n, (_, a, _) in CASES.items() if a is not None])
def test_composite_and_grey_are_the_torch_statements(hip, name):
    from gsplat_amd.imageio import save_image_bytes
    depth, alpha, _ = CASES[name]
    d, a = dev(depth), dev(alpha)
    comp, grey = dv.composite_depth(d, a)
    want = (d - d.min()) / (d.max() - d.min()) + 1 * (1 - a)     # render.py:121
    if bool(torch.isnan(want).any()):   # (torch.equal calls NaN unequal to itself: the bits, and no byte asked of a NaN)
        assert torch.equal(comp.view(torch.int32), want.view(torch.int32))
        return
    assert torch.equal(comp, want)
    assert torch.equal(grey, save_image_bytes(1 - want))          # render.py:124
    both, g2 = dv.colour_and_grey(d, a)
    assert torch.equal(g2, grey) and torch.equal(both, dv.colour_depth(d, a))


def raw_call(api, depth, alpha, H, W, rule, lut, tmp, nb, out, grey=None, comp=None, bounds=None):
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return api.raw("depth_vis")(p(depth), p(alpha), H, W, rule, p(lut), p(tmp), nb, p(out), p(grey), p(comp), p(bounds), stream)


def test_exact_scratch_behind_guard_words_and_reuse(hip):
    api = hip.api
    depth, alpha, _ = CASES["plain_alpha_64x48"]
    other = CASES["size_64x48"][0]
    H, W = depth.shape
    nb = int(api.raw("depth_vis_tmp_bytes")(H, W))
    assert nb > 4 * H * W and nb % 256 == 0
    lut = dev(dv.byte_tables()["save_image"])
    fresh = dv.colour_depth(dev(depth), dev(alpha), rule="dng")
    buf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    tmp = buf[256:256 + nb]
    runs = []
    for x, a in ((depth, alpha), (other, None), (depth, alpha)):   # the third call meets what the second left behind
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device=DEV)
        assert raw_call(api, dev(x), dev(a), H, W, dv.RULES["dng"], lut, tmp, nb, out) == 0
        runs.append(out)
    torch.cuda.synchronize()
    assert bool((buf[:256] == 0xA5).all()) and bool((buf[256 + nb:] == 0xA5).all()), "a write outside the scratch"
    assert torch.equal(runs[0], fresh) and torch.equal(runs[2], fresh)
    assert torch.equal(runs[1], dv.colour_depth(dev(other), rule="dng"))
    assert raw_call(api, dev(depth), None, H, W, 1, lut, tmp, nb - 1, runs[0]) == -2          # one byte short


def test_empty_images_and_every_bad_argument_status(hip):
    api = hip.api
    H, W = 4, 5
    nb = int(api.raw("depth_vis_tmp_bytes")(H, W))
    d, a = torch.rand((H, W), device=DEV), torch.rand((H, W), device=DEV)
    lut = dev(dv.byte_tables()["trunc"])
    tmp = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=DEV)
    grey, comp = torch.empty_like(out), torch.empty((H, W), device=DEV)
    assert raw_call(api, d, a, H, W, 2, lut, tmp, nb, out, grey, comp) == 0
    for h, w in ((0, 5), (5, 0), (0, 0)):                                                      # H * W == 0: nothing to do
        assert api.raw("depth_vis_tmp_bytes")(h, w) == 0
        assert raw_call(api, None, None, h, w, 0, None, None, 0, None) == 0
        e = dv.colour_depth(torch.empty((h, w), device=DEV))
        assert tuple(e.shape) == (h, w, 3) and e.is_cuda
    assert api.raw("depth_vis_tmp_bytes")(-1, 5) == 0 and api.raw("depth_vis_tmp_bytes")(4097, 4097) == 0
    assert raw_call(api, d, None, -1, W, 0, lut, tmp, nb, out) == -2                           # GS_E_SHAPE
    assert raw_call(api, d, None, 4097, 4097, 0, lut, tmp, nb, out) == -2                      # more than 2^24 pixels
    assert raw_call(api, d, None, H, W, 3, lut, tmp, nb, out) == -2                            # unknown rule
    assert raw_call(api, d, None, H, W, -1, lut, tmp, nb, out) == -2
    assert raw_call(api, d, None, H, W, 0, lut, tmp, nb - 1, out) == -2                        # scratch too small
    assert raw_call(api, d, None, H, W, 0, lut, tmp[1:], nb, out) == -2                        # scratch not 256-byte aligned
    assert raw_call(api, None, None, H, W, 0, lut, tmp, nb, out) == -1                         # GS_E_NULL
    assert raw_call(api, d, None, H, W, 0, None, tmp, nb, out) == -1
    assert raw_call(api, d, None, H, W, 0, lut, None, nb, out) == -1
    assert raw_call(api, d, None, H, W, 0, lut, tmp, nb, None) == -1
    assert raw_call(api, d, None, H, W, 0, lut, tmp, nb, out, grey) == -1                      # grey / composite without alpha
    assert raw_call(api, d, None, H, W, 0, lut, tmp, nb, out, None, comp) == -1
    torch.cuda.synchronize()


def test_colour_depth_makes_no_synchronising_call(hip):
    depth, alpha, _ = CASES["plain_alpha_64x48"]
    d, a = dev(depth), dev(alpha)
    for rule in dc.RULES:
        dv.colour_depth(d, a, rule=rule)          # (the first call of a rule copies its byte table to the device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [dv.colour_depth(d, a, rule=rule, return_bounds=True) for rule in dc.RULES]
        outs.append(dv.composite_depth(d, a))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(o[0].is_cuda for o in outs)


def read_frames(base, names):
    from gsplat_amd.imageio import read_png
    return [read_png(os.path.join(base, n)) for n in names]


def test_path_frames_of_a_small_model(hip, tmp_path):
    """write_path_frames on 64 x 48 renders along a generated path, through render_fsgs and render_dng; prune_for_path against
    the host statements of spiral.py:104-108."""
    import dgr_dng
    import dgr_fsgs
    import test_dng_trainer_cpu as cpu
    from gsplat_amd import paths, render_set
    from gsplat_amd.imageio import save_image_bytes
    from gsplat_amd.trainer import GaussianModelLite, TrainerDNG, camera_to, render_dng, render_fsgs
    sc, cams, gts, mono = cpu.inputs()
    poses = paths.generate_ellipse_path(cams, n_frames=2)
    path_cams = [camera_to(paths.camera_from_pose(cams[0], p), DEV) for p in poses]
    bg = torch.zeros(3, device=DEV)
    model = GaussianModelLite(sc, DEV, api=hip.api)
    model.active_sh_degree = 0
    with torch.no_grad():
        conf = torch.ones((model.P, 1), device=DEV)
        fs = [render_fsgs(c, model, dgr_fsgs.GaussianRasterizer, dgr_fsgs.GaussianRasterizationSettings, bg, conf) for c in path_cams]
        assert tuple(fs[0]["render"].shape) == (3, cpu.H, cpu.W) and float(fs[0]["alpha"].max()) > 0
        base = render_set.write_path_frames(str(tmp_path / "f"), fs, layout="fsgs_video", iteration=9, fsgs_depth=True)
        sets = os.path.join(str(tmp_path / "f"), "test", "ours_9", "renders")
        for i, f in enumerate(fs):
            (png,) = read_frames(base, ["%05d.png" % i])
            assert np.array_equal(png, save_image_bytes(f["render"].clamp(0, 1)).cpu().numpy())
            (cd,) = read_frames(sets, ["%05d_depth.png" % i])
            assert np.array_equal(cd, dv.colour_depth(f["depth"][0], rule="fsgs").cpu().numpy())
            assert np.array_equal(np.load(os.path.join(sets, "%05d_depth.npy" % i)), f["depth"][0].cpu().numpy())
        tr = TrainerDNG(GaussianModelLite(sc, DEV, api=hip.api), [camera_to(c, DEV) for c in cams], [g.to(DEV) for g in gts],
                        [m.to(DEV) for m in mono], near_centers=paths.path_centres(path_cams), near_range=0.0)
        ds = [render_dng(c, tr.model, tr.neural, dgr_dng.GaussianRasterizer, dgr_dng.GaussianRasterizationSettings, tr.bg)
              for c in path_cams]
        base = render_set.write_path_frames(str(tmp_path / "d"), ds, layout="dng_spiral", iteration=9)
        assert sorted(os.listdir(base)) == sorted(p + "%05d.png" % i for i in range(2) for p in ("", "depth_", "cdepth_"))
        for i, f in enumerate(ds):
            png, grey, cd = read_frames(base, ["%05d.png" % i, "depth_%05d.png" % i, "cdepth_%05d.png" % i])
            assert np.array_equal(png, save_image_bytes(f["render"]).cpu().numpy())
            comp, g = dv.composite_depth(f["depth"], f["alpha"])
            assert np.array_equal(grey, g.cpu().numpy())
            assert np.array_equal(cd, dv.colour_depth(f["depth"], f["alpha"], rule="dng").cpu().numpy())
    # the near-camera prune over the path's cameras
    centres = paths.path_centres(path_cams)
    xyz = model.get_xyz.detach().cpu()
    dmin = torch.stack([(xyz - c).norm(dim=1) for c in centres]).min(dim=0).values.sort().values
    gaps = dmin[1:] - dmin[:-1]
    k = int(gaps[xyz.shape[0] // 4: xyz.shape[0] // 2].argmax()) + xyz.shape[0] // 4
    near = float((dmin[k] + dmin[k + 1]) / 2)      # between two Gaussians' distances: no row sits on the threshold
    assert float(gaps[k]) > 1e-4
    want = torch.zeros((xyz.shape[0],), dtype=torch.bool)
    for c in centres:
        want = want + ((xyz - c.repeat(xyz.shape[0], 1)).norm(dim=1, keepdim=True) < near)[:, 0]
    P0 = model.P
    mask = render_set.prune_for_path(model, centres, near)
    assert 0 < int(want.sum()) < P0 and torch.equal(mask.cpu(), want)
    assert model.P == P0 - int(want.sum()) and torch.equal(model.get_xyz.detach().cpu(), xyz[~want])
