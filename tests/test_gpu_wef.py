"""GPU half of the Wavelet Error Field tests: csrc/gs_wef.hip through gsplat_amd.wef / lgdwt_loss and once through the raw ABI.
Cases, float64 twins and derived bars come from tests/wef_cases.py (tests/test_wef_cpu.py keeps the bars honest).

  maps         every case, both band sets: every element within the bar of the float64 twin, exact zeros and the NaN pattern
               as tabled, the same bits on two calls and through the raw ABI (tmp of exactly gs_wef_tmp_bytes between guards)
  out_bounds   equal to the minimum / maximum of the device's own values before normalisation: the energy planes are read back
               from tmp (the layout include/gsplat.h documents) and upsampled by bilinear_np, a numpy float32 statement of
               csrc/gs_haar.h's formula in which, as on the device, every operation rounds once
  grid         bytes EXACT against numpy's (clip(heatmap, 0, 1) * 255).astype(uint8) on the device's own maps
  Charbonnier  forward within 1 ulp of the correctly rounded float64 sum of the float32 terms, gradients within 2 ulp of
               float64 autograd, n off the float4 grid
  wef_report   leaves training alone; its maps are compute_wef_maps on the same clamped render"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import wef_cases as wc
from gsplat_amd import wef

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASE_IDS = [c.name for c in wc.CASES]
f32 = np.float32


def align256(n):
    return (n + 255) & ~255


def tap_np(n_out, n_in):
    o = np.arange(n_out, dtype=f32)
    scale = f32(n_in) / f32(n_out)
    src = np.maximum(scale * (o + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1) - l1
    edge = i1 == i0
    return i0, i1, np.where(edge, f32(1), l0).astype(f32), np.where(edge, f32(0), l1).astype(f32)


def bilinear_np(plane, H, W):
    y0, y1, ly0, ly1 = tap_np(H, plane.shape[0])
    x0, x1, lx0, lx1 = tap_np(W, plane.shape[1])
    top = lx0[None] * plane[y0][:, x0] + lx1[None] * plane[y0][:, x1]
    bot = lx0[None] * plane[y1][:, x0] + lx1[None] * plane[y1][:, x1]
    out = ly0[:, None] * top + ly1[:, None] * bot
    assert out.dtype == f32
    return out


def nan_min_max(a):
    return (f32("nan"), f32("nan")) if np.isnan(a).any() else (a.min(), a.max())


@pytest.fixture(scope="module")
def device_maps(hip):
    """every case through the public functions, once: {name: {all_bands: {key: [1,1,H,W] on the device}}}"""
    import lgdwt_loss
    out = {}
    for c in wc.CASES:
        pred, gt = (t.to(DEV) for t in wc.inputs(c))
        out[c.name] = {False: lgdwt_loss.compute_wef_maps(pred, gt), True: lgdwt_loss.compute_wef_all_subbands(pred[None], gt[None])}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", CASE_IDS)
def test_maps_within_the_bar_of_float64(device_maps, name):
    c = wc.BY_NAME[name]
    for all_bands in (False, True):
        maps = device_maps[name][all_bands]
        assert tuple(maps) == wc.keys_of(all_bands)
        assert all(m.shape == (1, 1, c.H, c.W) and m.dtype == torch.float32 and m.is_cuda for m in maps.values())
        dist = wc.check_maps(c, all_bands, maps, "hip")
        if dist:
            print("%s %s: HIP %.2e from float64, largest bar %.2e"
                  % (name, "all" if all_bands else "l2", max(dist.values()), max([b for b in wc.bars(c, all_bands).values() if b] or [0.0])))
        if (name, all_bands) in wc.ALL_FLAT:
            assert all(bool((m == 0).all()) for m in maps.values())


@pytest.mark.parametrize("name", CASE_IDS)
def test_raw_abi_guards_bounds_and_bits(hip, device_maps, name):
    c = wc.BY_NAME[name]
    api = hip.api
    pred, gt = (t.to(DEV) for t in wc.inputs(c))
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    h1, w1 = (c.H + 1) // 2, (c.W + 1) // 2
    h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
    for all_bands in (False, True):
        K = 8 if all_bands else 3
        nb = int(api.raw("wef_tmp_bytes")(c.C, c.H, c.W, int(all_bands)))
        assert nb > 0 and nb % 256 == 0
        G = 4096
        buf = torch.full((nb + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
        tmp = buf[G:G + nb]
        assert tmp.data_ptr() % 256 == 0
        outs = []
        for _ in range(2):
            out = torch.full((K + 1, c.H, c.W), -7.0, dtype=torch.float32, device=DEV)
            bounds = torch.full((K + 1, 2), -7.0, dtype=torch.float32, device=DEV)
            api.call("wef_maps", pred.data_ptr(), gt.data_ptr(), c.C, c.H, c.W, int(all_bands), tmp.data_ptr(), nb, out.data_ptr(),
                     bounds.data_ptr(), stream)
            outs.append((out, bounds))
        torch.cuda.synchronize()
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + nb:] == 0xA5).all()), "gs_wef_maps wrote outside tmp"
        (out, bounds), (out2, bounds2) = outs
        as_bits = lambda t: t.view(torch.int32)   # noqa: E731  (NaN == NaN)
        assert torch.equal(as_bits(out), as_bits(out2)) and torch.equal(as_bits(bounds), as_bits(bounds2)), "bits differ between calls"
        public = torch.cat([device_maps[name][all_bands][k][0] for k in wc.keys_of(all_bands)])
        assert torch.equal(as_bits(out), as_bits(public)), "the raw ABI and the public function differ"
        # the energy planes at the head of tmp -> the values before normalisation
        raw = tmp.cpu().numpy()
        q, hsz = align256(4 * h2 * w2), align256(4 * h1 * w1)
        plane = lambda off, h, w: raw[off:off + 4 * h * w].view(f32).reshape(h, w)   # noqa: E731
        planes = ([plane(4 * q + k * hsz, h1, w1) for k in range(4)] if all_bands else []) + [plane(k * q, h2, w2) for k in range(4 if all_bands else 3)]
        b = bounds.cpu().numpy()
        for k, p in enumerate(planes):
            mn, mx = nan_min_max(bilinear_np(p, c.H, c.W))
            assert np.array_equal(b[k], np.array([mn, mx], dtype=f32), equal_nan=True), (name, all_bands, k, b[k], mn, mx)
        maps = out.cpu().numpy()
        acc = maps[0]
        for k in range(1, K):
            acc = acc + maps[k]
        comb = acc / f32(8.0 if all_bands else 3.0)
        mn, mx = nan_min_max(comb)
        assert np.array_equal(b[K], np.array([mn, mx], dtype=f32), equal_nan=True), (name, all_bands, b[K], mn, mx)
        if c.kind != "nan":   # and the maps are the normalisation of exactly those values
            for k, p in enumerate(planes):
                u = bilinear_np(p, c.H, c.W)
                assert np.array_equal(maps[k], (u - b[k, 0]) / ((b[k, 1] - b[k, 0]) + f32(1e-8)))
            assert np.array_equal(maps[K], (comb - b[K, 0]) / ((b[K, 1] - b[K, 0]) + f32(1e-8)))


def test_raw_abi_refusals(hip):
    api = hip.api
    size = api.raw("wef_tmp_bytes")
    assert size(0, 8, 8, 0) == 0 and size(5, 8, 8, 0) == 0 and size(3, 0, 8, 1) == 0 and size(3, 8, 8, 2) == 0
    assert size(3, 65536, 32768, 0) == 0 and size(3, 46340, 46340, 1) > 0
    x = torch.zeros((3, 8, 8), device=DEV)
    nb = int(size(3, 8, 8, 1))
    tmp = torch.empty((nb + 256,), dtype=torch.uint8, device=DEV)
    out = torch.empty((9, 8, 8), device=DEV)
    f = api.raw("wef_maps")
    p = lambda t: t.data_ptr()   # noqa: E731
    GS_E_NULL, GS_E_SHAPE = -1, -2   # include/gsplat.h
    codes = {f(None, p(x), 3, 8, 8, 1, p(tmp), nb, p(out), None, None), f(p(x), p(x), 3, 8, 8, 1, None, nb, p(out), None, None),
             f(p(x), p(x), 3, 8, 8, 1, p(tmp), nb, None, None, None)}
    shape = {f(p(x), p(x), 5, 8, 8, 1, p(tmp), nb, p(out), None, None), f(p(x), p(x), 3, 8, 8, 1, p(tmp), nb - 1, p(out), None, None),
             f(p(x), p(x), 3, 8, 8, 1, p(tmp) + 4, nb, p(out), None, None), f(p(x), p(x), 3, 8, 8, 7, p(tmp), nb, p(out), None, None)}
    assert codes == {GS_E_NULL} and shape == {GS_E_SHAPE}
    g = api.raw("wef_grid")
    order = torch.zeros((1,), dtype=torch.int32, device=DEV)
    u8 = torch.empty((8, 8, 3), dtype=torch.uint8, device=DEV)
    assert g(p(out), 9, 8, 8, p(order), 0, 3, None, p(u8), None) == GS_E_SHAPE
    assert g(p(out), 9, 8, 8, p(order), 1, 0, None, p(u8), None) == GS_E_SHAPE
    assert g(None, 9, 8, 8, p(order), 1, 1, None, p(u8), None) == GS_E_NULL
    assert api.raw("charbonnier_tmp_bytes")(0) == 0
    assert api.raw("charbonnier_fwd")(p(x), p(x), 0, 1e-3, p(tmp), nb, p(out), None) == GS_E_SHAPE
    assert api.raw("charbonnier_bwd")(p(x), p(x), 4, 1e-3, p(out), None, None, None) == GS_E_NULL
    torch.cuda.synchronize()


def heat_bytes_np(v):
    x = np.clip(v, f32(0), f32(1))
    heat = np.stack([x, np.clip(f32(1) - np.abs(x - f32(0.5)) * f32(2), f32(0), f32(1)), f32(1) - x], axis=-1)
    return (np.clip(heat, 0, 1) * f32(255)).astype(np.uint8)


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if c.kind != "nan"])
def test_grid_bytes_exact(device_maps, name):
    c = wc.BY_NAME[name]
    for all_bands, cols in ((False, 3), (True, 4), (True, 1)):
        maps = device_maps[name][all_bands]
        keys = list(wc.keys_of(all_bands))
        grid = wef.make_wef_grid_image(maps, keys, tile_cols=cols)
        rows = (len(keys) + cols - 1) // cols
        assert grid.is_cuda and grid.dtype == torch.uint8 and tuple(grid.shape) == (rows * c.H, cols * c.W, 3)
        want = np.zeros((rows * c.H, cols * c.W, 3), dtype=np.uint8)
        for idx, k in enumerate(keys):
            r, cc = idx // cols, idx % cols
            want[r * c.H:(r + 1) * c.H, cc * c.W:(cc + 1) * c.W] = heat_bytes_np(maps[k][0, 0].cpu().numpy())
        assert np.array_equal(grid.cpu().numpy(), want), (name, all_bands, cols)


def test_grid_nan_and_heatmap(device_maps):
    maps = device_maps["nan_6x9"][False]
    grid = wef.make_wef_grid_image(maps, ["LL2"], tile_cols=1).cpu().numpy()
    assert (grid[..., 0] == 0).all() and (grid[..., 1] == 0).all() and (grid[..., 2] == 255).all()   # x = clamp(NaN) -> 0
    x = torch.linspace(-0.25, 1.25, 97).reshape(1, 1, 1, 97)
    assert torch.equal(wef.make_heatmap_rgb(x.to(DEV)).cpu(), wef.make_heatmap_rgb(x))


@pytest.mark.parametrize("shape,cols", [((40, 150), 3), ((5, 7), 3), ((30, 100), 2)])
def test_titled_grid_labels(hip, shape, cols):
    H, W = shape
    keys = list(wc.ALL_KEYS[4:])
    maps = {k: torch.rand((1, 1, H, W), generator=torch.Generator().manual_seed(i)).to(DEV) for i, k in enumerate(keys)}
    got = wef.make_wef_grid_image_titled(maps, keys, tile_cols=cols).cpu().numpy()
    plain = wef.make_wef_grid_image(maps, keys, tile_cols=cols).cpu().numpy()
    labels = np.stack([wef.label_mask(k) for k in keys])
    want = wef.grid_numpy([maps[k][0, 0].cpu().numpy() for k in keys], cols, labels)
    assert np.array_equal(got, want)
    inside = np.zeros(got.shape[:2], dtype=bool)
    for idx in range(len(keys)):
        r, c = idx // cols, idx % cols
        inside[r * H:r * H + 27, c * W:c * W + 121] = True
    assert np.array_equal(got[~inside], plain[~inside]) and set(np.unique(got[inside]).tolist()) <= {0, 255}
    if W >= 121 and H >= 27:
        a, b = got[:27, :121], got[:27, W:W + 121]
        assert a.any() and b.any() and not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ Charbonnier
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(f32)).astype(np.float64)


@pytest.mark.parametrize("n", [1, 3, 255, 257, 4097])
@pytest.mark.parametrize("eps", [1e-3, 0.05])
def test_charbonnier(hip, n, eps):
    import lgdwt_loss
    g = torch.Generator().manual_seed(n)
    pred, target = torch.rand((n,), generator=g), torch.rand((n,), generator=g)
    if n >= 3:
        target[1] = pred[1]
    # forward: the float32 terms formed on the CPU, their correctly rounded float64 sum, one rounding of the mean
    d = pred - target
    terms = torch.sqrt(d * d + torch.tensor(eps * eps, dtype=torch.float32))
    want = f32(math.fsum(terms.double().tolist()) / n)
    p, t = pred.to(DEV).requires_grad_(True), target.to(DEV).requires_grad_(True)
    loss = lgdwt_loss.charbonnier_loss(p, t, eps)
    assert loss.shape == () and loss.dtype == torch.float32
    (3.0 * loss).backward()
    got = f32(loss.item())
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), (n, eps, got, want)
    p64, t64 = pred.double().requires_grad_(True), target.double().requires_grad_(True)
    d64 = p64 - t64
    (3.0 * torch.sqrt(d64 * d64 + eps * eps).mean()).backward()
    for got_g, want_g, what in ((p.grad, p64.grad, "pred"), (t.grad, t64.grad, "target")):
        err = np.abs(got_g.cpu().double().numpy() - want_g.numpy())
        assert (err <= 2 * ulp32(want_g.numpy())).all(), (n, eps, what, float(err.max()))
    # one argument only, the same bits; a shape of higher rank
    p2 = pred.to(DEV).requires_grad_(True)
    (3.0 * lgdwt_loss.charbonnier_loss(p2, target.to(DEV), eps)).backward()
    assert torch.equal(p2.grad, p.grad)
    t2 = target.to(DEV).requires_grad_(True)
    (3.0 * lgdwt_loss.charbonnier_loss(pred.to(DEV), t2, eps)).backward()
    assert torch.equal(t2.grad, t.grad)
    if n == 4097:
        assert torch.equal(lgdwt_loss.charbonnier_loss(pred[:4096].reshape(2, 8, 16, 16).to(DEV), target[:4096].reshape(2, 8, 16, 16).to(DEV), eps),
                           lgdwt_loss.charbonnier_loss(pred[:4096].to(DEV), target[:4096].to(DEV), eps))
        with pytest.raises(ValueError, match="float32"):
            lgdwt_loss.charbonnier_loss(pred.double().to(DEV), target.double().to(DEV))


# -------------------------------------------------------------------------------------------------------------- trainer
def test_wef_report_leaves_training_alone(hip, tmp_path):
    from gsplat_amd import imageio
    from gsplat_amd.trainer import TrainOptions, render
    from test_gpu_eval_metrics import small_trainer
    opt = TrainOptions()
    a, b = small_trainer(hip), small_trainer(hip)
    reports = []
    for tr, report_between in ((a, True), (b, False)):
        tr.train_iteration(1, opt)
        if report_between:
            reports.append(tr.wef_report(camera=1, path=str(tmp_path / "wef.png")))
            reports.append(tr.wef_report(camera=2, bands="all", titled=True, tile_cols=4))
        tr.train_iteration(2, opt)
        tr.sync()
    torch.cuda.synchronize()
    assert a.last["path"] == b.last["path"]
    assert torch.equal(a.model.flat, b.model.flat)
    assert torch.equal(a.model.optimizer.exp_avg, b.model.optimizer.exp_avg)
    assert torch.equal(a.model.optimizer.exp_avg_sq, b.model.optimizer.exp_avg_sq)
    assert a.model.optimizer.t == b.model.optimizer.t
    H, W = 64, 64
    assert tuple(reports[0]) == wc.LEVEL2_KEYS + ("grid",) and tuple(reports[1]) == wc.ALL_KEYS + ("grid",)
    assert tuple(reports[0]["grid"].shape) == (2 * H, 3 * W, 3) and tuple(reports[1]["grid"].shape) == (3 * H, 4 * W, 3)
    back = imageio.read_png(str(tmp_path / "wef.png"))
    assert np.array_equal(np.asarray(back), reports[0]["grid"].cpu().numpy())
    with pytest.raises(ValueError, match="bands"):
        a.wef_report(bands="level1")
    # the report's maps are compute_wef_maps on the same clamped render (of the model as it now is)
    rep = a.wef_report(camera=1)
    with torch.no_grad():
        img = render(a.cameras[1], a.model, a.Rasterizer, a.Settings, a.bg, filter_as_indices=None, clamp=False)["render"].clamp(0, 1)
    want = wef.compute_wef_maps(img, a.gts[1])
    for k in wc.LEVEL2_KEYS:
        assert torch.equal(rep[k], want[k]), k
    assert float(rep["WEF"].max()) > 0.5 and float(rep["WEF"].min()) == 0.0
