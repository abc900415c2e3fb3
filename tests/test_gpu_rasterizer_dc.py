"""The `dc=` / `shs=` rasterizer call (gsplat_amd.accel, gs_backward_split) against the concatenated call of the default package
on the same numbers: image, radii, inverse depth and EVERY gradient bit for bit (the backward is run-to-run bit-identical) - and
the reference's accelerated loop on top of it (DropInLoop(optimizer="sparse_adam", separate_sh=True)), each optimizer step held
to the restatement of tests/sparse_adam_reference.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import dc_cases
import sparse_adam_reference as ref
from step_reference import bits, param_tolerance

pytestmark = pytest.mark.gpu

W, H = 64, 48
E_NULL, E_UNSUPPORTED = -1, -5


def _poison(dev, P, K):
    """Leave NaN-filled blocks of the gradients' sizes in the allocator's cache: the split backward allocates its two SH
    gradients uninitialised, so a row the kernel does not write shows."""
    junk = [torch.full(s, float("nan"), device=dev) for s in ((P, 1, 3), (P, max(K, 1), 3), (P, 1 + K, 3))]
    del junk


def _pair(hip, sc, cam, degree, K, **kw):
    import diff_gaussian_rasterization as dgr
    from gsplat_amd import accel
    dev = torch.device("cuda:0")
    P = sc["means3D"].shape[0]
    key = kw.pop("camera_key", None)
    cat = dc_cases.run(dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, sc, cam, dev, degree, split=False,
                       camera_key=None if key is None else key + ("cat",), **kw)
    _poison(dev, P, K)
    split = dc_cases.run(accel.GaussianRasterizer, accel.GaussianRasterizationSettings, sc, cam, dev, degree, split=True,
                         camera_key=None if key is None else key + ("split",), **kw)
    return split, cat


def _check_culled_rows(split, what):
    culled = split["radii"] == 0
    for k in ("dc", "rest"):
        g = split["grads"][k]
        if g is not None and g.numel():
            assert torch.isfinite(g).all(), "%s: dL/d%s has rows the kernel did not write" % (what, k)
            assert not g[culled].any(), "%s: dL/d%s of a culled Gaussian is not zero" % (what, k)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_split_call_is_the_concatenated_call(hip, P):
    sc = dc_cases.scene_rows(P, 15, seed=P)
    cam = dc_cases.inside_camera(W, H)
    seen = 0
    for degree in range(4):
        for antialiasing in (False, True):
            for use_depth in (False, True):
                what = "P=%d degree=%d aa=%d depth=%d" % (P, degree, antialiasing, use_depth)
                split, cat = _pair(hip, sc, cam, degree, 15, antialiasing=antialiasing, use_depth=use_depth)
                dc_cases.assert_same(split, cat, what)
                _check_culled_rows(split, what)
                assert tuple(split["grads"]["dc"].shape) == (P, 1, 3) and tuple(split["grads"]["rest"].shape) == (P, 15, 3)
                # coefficients above the active degree take no gradient
                assert not split["grads"]["rest"][:, (degree + 1) ** 2 - 1:, :].any(), what
                seen += int((split["radii"] > 0).sum())
                if P >= 255:
                    culled = int((split["radii"] == 0).sum())
                    assert 0 < culled < P, "%s: the camera must cull a share of the Gaussians (%d of %d)" % (what, culled, P)
                    assert split["grads"]["dc"].abs().max() > 0 and (degree == 0 or split["grads"]["rest"].abs().max() > 0), what
    assert P == 1 or seen > 0


@pytest.mark.parametrize("K", [3, 8])
def test_generic_row_counts(hip, K):
    """shs of 3 and 8 rows (M = 4 and 9: the per-Gaussian kernel writes the two global rows directly)."""
    P = 257
    sc = dc_cases.scene_rows(P, K, seed=K)
    cam = dc_cases.inside_camera(W, H)
    for degree in range(2 if K == 3 else 3):
        for antialiasing, use_depth in ((False, False), (True, True)):
            what = "K=%d degree=%d aa=%d" % (K, degree, antialiasing)
            split, cat = _pair(hip, sc, cam, degree, K, antialiasing=antialiasing, use_depth=use_depth)
            dc_cases.assert_same(split, cat, what)
            _check_culled_rows(split, what)
            assert tuple(split["grads"]["rest"].shape) == (P, K, 3) and split["grads"]["dc"].abs().max() > 0
            assert not split["grads"]["rest"][:, (degree + 1) ** 2 - 1:, :].any(), what


def test_degree_zero_model_camera_key_and_precomputed_covariance(hip):
    P = 257
    cam = dc_cases.inside_camera(W, H)
    # a degree-0 model: shs is [P,0,3] and dc alone is the SH tensor
    sc0 = dc_cases.scene_rows(P, 0, seed=1, max_degree=0)
    assert tuple(sc0["shs"].shape) == (P, 1, 3)
    split, cat = _pair(hip, sc0, cam, 0, 0, use_depth=True)
    dc_cases.assert_same(split, cat, "degree-0 model")
    assert split["grads"]["dc"].abs().max() > 0
    # a camera_key over two visits (the second renders from the camera's kept state), a different key for each form
    sc = dc_cases.scene_rows(P, 15, seed=2)
    for degree in (0, 3):
        split, cat = _pair(hip, sc, cam, degree, 15, use_depth=True, camera_key=("dc-test", degree), visits=2)
        dc_cases.assert_same(split, cat, "camera_key degree=%d" % degree)
        _check_culled_rows(split, "camera_key degree=%d" % degree)
    hip.drop_camera_entries(("dc-test",))
    # cov3D_precomp with dc=: the fall-back (concatenate, ordinary call), same numbers
    split, cat = _pair(hip, sc, cam, 3, 15, precomputed_cov=True)
    dc_cases.assert_same(split, cat, "cov3D_precomp", precomputed_cov=True)
    assert split["grads"]["cov3D_precomp"].abs().max() > 0 and split["grads"]["rest"].abs().max() > 0


def test_entry_point_rules(hip):
    """gs_backward keeps refusing split rows; gs_backward_split refuses one-row layouts and raw activations; nothing is launched."""
    from gsplat_amd.capi import GsGaussians, GsGrads
    from test_abi_errors import setup
    api, dev = hip.api, torch.device("cuda")
    t, v, g, s, bufs, wsb = setup(api, dev)
    radii = torch.zeros(8, dtype=torch.int32, device=dev)
    img = torch.zeros(3, 32, 32, device=dev)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    out = {k: torch.full(shape, 7.0, device=dev) for k, shape in
           (("dsh", (8, 1, 3)), ("rest", (8, 15, 3)), ("m3", (8, 3)), ("m2", (8, 3)), ("op", (8, 1)), ("sc", (8, 3)), ("rot", (8, 4)))}
    grads = GsGrads()
    grads.dL_dmeans3D, grads.dL_dmeans2D, grads.dL_dsh = out["m3"].data_ptr(), out["m2"].data_ptr(), out["dsh"].data_ptr()
    grads.dL_dopacity, grads.dL_dscales, grads.dL_drotations = out["op"].data_ptr(), out["sc"].data_ptr(), out["rot"].data_ptr()
    rest = torch.rand(8, 15, 3, device=dev)
    gsplit = GsGaussians.from_buffer_copy(g)
    gsplit.shs_rest = rest.data_ptr()
    bw, bs = api.raw("backward"), api.raw("backward_split")

    def split(gg, grads_, rest_out):
        return bs(C.byref(v), C.byref(gg), radii.data_ptr(), C.byref(s), 0, img.data_ptr(), None,
                  None if grads_ is None else C.byref(grads_), rest_out, ws.data_ptr(), wsb, None)
    assert bw(C.byref(v), C.byref(gsplit), radii.data_ptr(), C.byref(s), 0, img.data_ptr(), None, C.byref(grads), ws.data_ptr(), wsb,
              None) == E_UNSUPPORTED
    assert split(g, grads, out["rest"].data_ptr()) == E_UNSUPPORTED            # no shs_rest: that is gs_backward's layout
    graw = GsGaussians.from_buffer_copy(gsplit)
    graw.raw_activations = 1
    assert split(graw, grads, out["rest"].data_ptr()) == E_UNSUPPORTED         # raw rows: the fused step's gradients-out form
    assert split(gsplit, grads, None) == E_NULL
    assert split(gsplit, None, out["rest"].data_ptr()) == E_NULL
    nosh = GsGrads.from_buffer_copy(grads)
    nosh.dL_dsh = None
    assert split(gsplit, nosh, out["rest"].data_ptr()) == E_NULL
    torch.cuda.synchronize()
    for k, x in out.items():
        assert bool((x == 7.0).all()), "a refused call wrote %s" % k


def test_accelerated_loop_steps_only_the_rows_the_view_saw(hip):
    """DropInLoop(optimizer="sparse_adam", separate_sh=True): five iterations over two cameras; every optimizer step is held to the
    restatement on its own (state snapshotted before the step), so a last-bit difference could not cascade."""
    from gsplat_amd import synthetic
    from gsplat_amd.dropin import DropInLoop
    from gsplat_amd.optim import SparseGaussianAdam
    dev = torch.device("cuda:0")
    P, LW, LH = 300, 128, 128
    scene = synthetic.trained_like(P, seed=3)
    cams = [synthetic.orbit_cameras(LW, LH)[1], dc_cases.inside_camera(LW, LH)]
    g = torch.Generator().manual_seed(4)
    gts = [torch.rand((3, LH, LW), generator=g).to(dev) for _ in cams]
    loop = DropInLoop(scene, cams, gts, dev, dwt=True, patch=False, optimizer="sparse_adam", separate_sh=True)
    opt = loop.optimizer
    assert type(opt) is SparseGaussianAdam and opt.bias_correction is False
    snaps = []
    inner = opt.step

    def spying_step(visibility, N):
        assert visibility.dtype == torch.bool and N == P and visibility.shape == (P,)
        before = []
        for group in opt.param_groups:
            p = group["params"][0]
            st = opt.state.get(p, {})
            zero = np.zeros(p.numel(), np.float32)
            before.append(dict(p=p.detach().cpu().numpy().ravel().copy(), g=p.grad.cpu().numpy().ravel().copy(),
                               m=st["exp_avg"].cpu().numpy().ravel().copy() if st else zero,
                               v=st["exp_avg_sq"].cpu().numpy().ravel().copy() if st else zero,
                               grad_ptr_ok=p.grad.is_contiguous()))
        inner(visibility, N)
        torch.cuda.synchronize()
        snaps.append((visibility.cpu().numpy().copy(), before, [
            dict(p=group["params"][0].detach().cpu().numpy().ravel().copy(),
                 m=opt.state[group["params"][0]]["exp_avg"].cpu().numpy().ravel().copy(),
                 v=opt.state[group["params"][0]]["exp_avg_sq"].cpu().numpy().ravel().copy(),
                 t=float(opt.state[group["params"][0]]["step"])) for group in opt.param_groups]))
    opt.step = spying_step
    losses = [loop.iteration(i % 2) for i in range(5)]
    assert all(np.isfinite(x) for x in losses) and len(snaps) == 5
    off32 = 0
    for it, (vis, before, after) in enumerate(snaps):
        assert 0 < int(vis.sum()), "iteration %d: no visible Gaussian" % it
        for group, b, a, w in zip(opt.param_groups, before, after, ref.WIDTHS):
            what = "iteration %d %s" % (it, group["name"])
            assert a["t"] == it + 1.0 and b["grad_ptr_ok"], what      # (the gradients arrive contiguous: one per model tensor)
            p32, m32, v32 = ref.sparse_adam_ref(b["p"], b["g"], b["m"], b["v"], group["lr"], it + 1, w, vis, False, np.float32)
            p64, _, _ = ref.sparse_adam_ref(b["p"], b["g"], b["m"], b["v"], group["lr"], it + 1, w, vis, False, np.float64)
            assert np.array_equal(bits(a["m"]), bits(m32)) and np.array_equal(bits(a["v"]), bits(v32)), what
            on = ref.stepped_elements(P, w, vis)
            assert np.array_equal(bits(a["p"])[~on], bits(b["p"])[~on]), what + ": a row with radii == 0 moved"
            assert np.array_equal(bits(a["m"])[~on], bits(b["m"])[~on]) and np.array_equal(bits(a["v"])[~on], bits(b["v"])[~on]), what
            tol, own = param_tolerance(p32[on], p64[on])
            worst = float(np.abs(a["p"][on].astype(np.float64) - p64[on]).max())
            n_off = int((bits(a["p"]) != bits(p32)).sum())
            off32 += n_off
            print("%s max|p32-p64| %.3e  bar %.3e  largest deviation %.3e  (%d of %d not the float32 restatement's bits)"
                  % (what, own, tol, worst, n_off, int(on.sum())))
            assert worst <= tol, what
    # the second camera sees a part of the scene only: its steps left rows untouched
    assert any(int(vis.sum()) < P for vis, _, _ in snaps)
    print("loop: %d parameter elements off the float32 restatement's bits in all" % off32)
