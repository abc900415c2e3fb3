"""The image stage of the train step on the GPU (csrc/gs_image_stage.hip): trained exposure, clamp and alpha mask between the
rasterizer and the loss (LGDWT-GS/train.py:117-124, gaussian_renderer/__init__.py:112-119), the exposures' device Adam, and
the fast step that now keeps its shape with them."""
import ctypes as C

import pytest
import torch

import diff_gaussian_rasterization as dgr
import lgdwt_loss
from gsplat_amd import synthetic
from gsplat_amd.trainer import GaussianModelLite, TrainOptions, Trainer, camera_to

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
E_NULL, E_SHAPE = -1, -2


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def stage_inputs(W, H, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.rand((3, H, W), generator=g) * 1.6 - 0.3          # both clamp sides
    E = torch.eye(3, 4) + 0.15 * torch.randn((3, 4), generator=g)
    alpha = torch.rand((H, W), generator=g)
    alpha[alpha < 0.15] = 0.0
    alpha[alpha > 0.85] = 1.0
    alpha[:, : W // 2] = 0.0 if seed % 2 else alpha[:, : W // 2]
    alpha[: H // 3] = 0.0                                          # a zeroed band either way
    g_pred = torch.randn((3, H, W), generator=g)
    return raw, E, alpha, g_pred


def restated(raw, E, alpha, g_pred):
    """float64 torch: exposure (matmul of gaussian_renderer/__init__.py:114), clamp, mask, and the autograd backward"""
    r = raw.double().requires_grad_(True)
    e = E.double().requires_grad_(True)
    lin = torch.matmul(r.permute(1, 2, 0), e[:3, :3]).permute(2, 0, 1) + e[:3, 3, None, None]
    pred = lin.clamp(0, 1) * alpha.double()
    pred.backward(g_pred.double())
    return lin.detach(), pred.detach(), r.grad, e.grad


@pytest.mark.parametrize("W,H", [(480, 320), (1920, 1080), (322, 242)])
def test_stage_forward_backward_against_float64(hip, W, H):
    api = hip.api
    raw, E, alpha, g_pred = stage_inputs(W, H, seed=W)
    lin64 = (torch.matmul(raw.double().permute(1, 2, 0), E.double()[:3, :3]).permute(2, 0, 1) + E.double()[:3, 3, None, None])
    near = ((lin64.abs() < 1e-6) | ((lin64 - 1).abs() < 1e-6))   # float rounding may put these on either side of the clamp
    n_near = int(near.sum())
    assert n_near <= 1e-4 * near.numel() + 8, n_near
    # ... so they carry no gradient in this comparison (torch.where takes the permuted layout of `near`: make it planes again)
    g_pred = torch.where(near, torch.zeros_like(g_pred), g_pred).contiguous()
    lin, pred64, graw64, dE64 = restated(raw, E, alpha, g_pred)
    d_raw, d_E, d_a, d_g = raw.to(DEV), E.to(DEV).contiguous(), alpha.to(DEV), g_pred.to(DEV)
    pred = torch.empty_like(d_raw)
    api.call("image_stage_fwd", d_raw.data_ptr(), d_E.data_ptr(), d_a.data_ptr(), H, W, pred.data_ptr(), _st())
    n_part = int(api.raw("image_stage_partials_count")(H, W))
    assert 1 <= n_part <= 1024
    part = torch.full((n_part * 12,), float("nan"), device=DEV)
    g_raw = torch.empty_like(d_raw)
    api.call("image_stage_bwd", d_raw.data_ptr(), d_E.data_ptr(), d_a.data_ptr(), d_g.data_ptr(), H, W, g_raw.data_ptr(),
             part.data_ptr(), _st())
    dE = torch.empty((3, 4), device=DEV)
    api.call("exposure_adam", part.data_ptr(), n_part, 0, dE.data_ptr(), None, None, None, 1, 0.0, 0.0, 0.0, 0.0, 0, None, _st())
    torch.cuda.synchronize()
    assert not torch.isnan(part).any(), "every workgroup writes its row"
    ok = ~near
    err_pred = float((pred.cpu().double() - pred64).abs()[ok].max())
    assert err_pred <= 1e-6, err_pred
    assert float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0
    scale = float(graw64.abs().max())
    err_g = float((g_raw.cpu().double() - graw64).abs().max()) / scale
    assert err_g <= 1e-5, err_g
    err_e = float((dE.cpu().double() - dE64).abs().max()) / float(dE64.abs().max())
    print("%dx%d: %d pixels near the clamp, pred err %.1e, g_raw rel %.1e, dE rel %.1e" % (W, H, n_near, err_pred, err_g, err_e))
    assert err_e <= 1e-5, err_e
    # without an exposure and a mask: the plain clamp, and g_raw = g_pred where 0 <= raw <= 1
    api.call("image_stage_fwd", d_raw.data_ptr(), None, None, H, W, pred.data_ptr(), _st())
    api.call("image_stage_bwd", d_raw.data_ptr(), None, None, d_g.data_ptr(), H, W, g_raw.data_ptr(), None, _st())
    torch.cuda.synchronize()
    assert torch.equal(pred, d_raw.clamp(0, 1))
    assert torch.equal(g_raw, torch.where((d_raw >= 0) & (d_raw <= 1), d_g, torch.zeros_like(d_g)))


def _criterion_run(gt, raw, mask, **kw):
    crit = lgdwt_loss.criterion(dwt_enable=True, patch_dwt_enable=True)
    x = raw.clone().requires_grad_(True)
    loss, parts = crit.fused_call(x, gt, mask=mask, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), x.grad.clone(), parts


def test_identity_exposure_and_unit_mask_give_the_plain_criterion_bits(hip):
    W, H = 480, 320
    g = torch.Generator().manual_seed(7)
    raw = (torch.rand((3, H, W), generator=g) * 1.6 - 0.3).to(DEV)
    gt = torch.rand((3, H, W), generator=g).to(DEV)
    mask = lgdwt_loss.criterion().elf_mask(gt)
    l0, g0, _ = _criterion_run(gt, raw, mask)
    eye = torch.eye(3, 4, device=DEV)
    ones = torch.ones((1, H, W), device=DEV)
    grad = torch.full((3, 4), float("nan"), device=DEV)
    l1, g1, parts = _criterion_run(gt, raw, mask, exposure=eye, alpha=ones, exposure_grad=grad)
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert torch.equal(g0, g1)
    assert "exposure_partials" in parts and not torch.isnan(grad).any()
    # with neither, parts carry nothing new (the stage-less path is today's)
    assert "exposure_partials" not in _criterion_run(gt, raw, mask)[2]


def test_exposure_gradient_is_the_same_bits_every_run(hip):
    W, H = 1920, 1080
    g = torch.Generator().manual_seed(9)
    raw = (torch.rand((3, H, W), generator=g) * 1.6 - 0.3).to(DEV)
    gt = torch.rand((3, H, W), generator=g).to(DEV)
    E = (torch.eye(3, 4) + 0.1 * torch.randn((3, 4), generator=g)).to(DEV)
    alpha = torch.rand((H, W), generator=g).to(DEV)
    mask = lgdwt_loss.criterion().elf_mask(gt)
    outs = []
    for _ in range(2):
        buf = torch.zeros((5, 3, 4), device=DEV)
        loss, graw, _ = _criterion_run(gt, raw, mask, exposure=E, alpha=alpha, exposure_grad=buf[2])
        outs.append((loss, graw, buf))
    assert float(outs[0][2][2].abs().max()) > 0 and float(outs[0][2][[0, 1, 3, 4]].abs().max()) == 0
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0])


def test_exposure_adam_matches_torch_adam_over_50_steps(hip):
    n = 6
    g = torch.Generator().manual_seed(4)
    start = (torch.eye(3, 4)[None].repeat(n, 1, 1) + 0.05 * torch.randn((n, 3, 4), generator=g)).to(DEV)
    from gsplat_amd.optim import ExposureAdam
    a = torch.nn.Parameter(start.clone())
    b = torch.nn.Parameter(start.clone())
    ta = torch.optim.Adam([a])
    tb = ExposureAdam(b)
    for k in range(50):
        lr = 0.01 * (0.1 ** (k / 50))
        ta.param_groups[0]["lr"] = lr
        tb.param_groups[0]["lr"] = lr
        grad = torch.zeros((n, 3, 4))
        grad[k % n] = torch.randn((3, 4), generator=g) * (10.0 ** (k % 3 - 1))   # one camera's row per step
        a.grad, b.grad = grad.to(DEV), grad.to(DEV)
        ta.step()
        tb.step()
        ta.zero_grad(set_to_none=True)
        tb.zero_grad(set_to_none=True)
        assert b.grad is None
    torch.cuda.synchronize()
    st = ta.state[a]
    assert tb.steps == 50 and int(st["step"]) == 50
    for x, y, what in ((a.detach(), b.detach(), "param"), (st["exp_avg"], tb.exp_avg, "exp_avg"),
                       (st["exp_avg_sq"], tb.exp_avg_sq, "exp_avg_sq")):
        err = float((x - y).abs().max()) / float(x.abs().max())
        assert err <= 2e-6, (what, err)
    assert float((b.detach() - start).abs().amin(dim=(1, 2)).min()) > 0   # every camera's row moved (zero-gradient steps too)


def test_exposure_adam_gate_and_partials_form(hip):
    """step_from_partials = (add the sums up, step) in one launch, the same as grad_row + step; a non-zero gate changes nothing"""
    from gsplat_amd.optim import ExposureAdam
    n, H, W = 3, 64, 96
    api = hip.api
    raw, E, alpha, g_pred = [t.to(DEV) for t in stage_inputs(W, H, seed=1)]
    part = torch.empty((int(api.raw("image_stage_partials_count")(H, W)) * 12,), device=DEV)
    api.call("image_stage_bwd", raw.data_ptr(), E.contiguous().data_ptr(), alpha.data_ptr(), g_pred.data_ptr(), H, W,
             torch.empty_like(raw).data_ptr(), part.data_ptr(), _st())
    p1 = torch.nn.Parameter(torch.eye(3, 4, device=DEV)[None].repeat(n, 1, 1))
    p2 = torch.nn.Parameter(p1.detach().clone())
    o1, o2 = ExposureAdam(p1), ExposureAdam(p2)
    o1.step_from_partials(part, 1)
    o2.grad_row(part, 1)
    o2.step()
    torch.cuda.synchronize()
    assert torch.equal(p1.grad, p2.grad) and torch.equal(p1.detach(), p2.detach())
    assert float(p1.grad[1].abs().max()) > 0 and float(p1.grad[[0, 2]].abs().max()) == 0
    before = (p1.detach().clone(), o1.exp_avg.clone(), o1.exp_avg_sq.clone())
    gate = torch.ones((1,), device=DEV)
    o1.step_from_partials(part, 2, gate=gate)
    torch.cuda.synchronize()
    assert torch.equal(before[0], p1.detach()) and torch.equal(before[1], o1.exp_avg) and torch.equal(before[2], o1.exp_avg_sq)


def test_image_stage_argument_errors(hip):
    f = hip.api.raw
    st = _st()
    img = torch.zeros((3, 8, 8), device=DEV)
    e = torch.zeros((3, 4), device=DEV)
    part = torch.zeros((12,), device=DEV)
    p = img.data_ptr()
    assert f("image_stage_partials_count")(0, 8) == 0 and f("image_stage_partials_count")(8, -1) == 0
    assert f("image_stage_fwd")(None, None, None, 8, 8, p, st) == E_NULL
    assert f("image_stage_fwd")(p, None, None, 8, 8, None, st) == E_NULL
    assert f("image_stage_fwd")(p, None, None, 0, 8, p, st) == E_SHAPE
    assert f("image_stage_fwd")(p, None, None, 8, -2, p, st) == E_SHAPE
    assert f("image_stage_bwd")(None, None, None, p, 8, 8, p, None, st) == E_NULL
    assert f("image_stage_bwd")(p, None, None, None, 8, 8, p, None, st) == E_NULL
    assert f("image_stage_bwd")(p, None, None, p, 8, 8, None, None, st) == E_NULL
    assert f("image_stage_bwd")(p, None, None, p, -1, 8, p, None, st) == E_SHAPE
    ea = f("exposure_adam")
    q = e.data_ptr()
    assert ea(None, 0, 0, None, q, q, q, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, st) == E_NULL        # no gradient source
    assert ea(part.data_ptr(), 1, 0, None, None, None, None, 1, 0.0, 0.9, 0.999, 1e-8, 1, None, st) == E_NULL  # nothing out
    assert ea(None, 0, 0, q, q, None, q, 1, 0.01, 0.9, 0.999, 1e-8, 1, None, st) == E_NULL        # moments missing
    assert ea(None, 0, 0, q, q, q, q, 0, 0.01, 0.9, 0.999, 1e-8, 1, None, st) == E_SHAPE          # no camera
    assert ea(part.data_ptr(), 1, 1, q, None, None, None, 1, 0.0, 0.9, 0.999, 1e-8, 1, None, st) == E_SHAPE  # camera out of range
    assert ea(part.data_ptr(), 0, 0, q, None, None, None, 1, 0.0, 0.9, 0.999, 1e-8, 1, None, st) == E_SHAPE  # no partial rows
    assert ea(None, 0, 0, q, q, q, q, 1, 0.01, 0.9, 0.999, 1e-8, 0, None, st) == E_SHAPE          # step is 1-based
    torch.cuda.synchronize()


# ---- the train step -------------------------------------------------------------------------------------------------
def alpha_masks(cams, W, H):
    from gsplat_amd.io import camera_alpha_mask
    g = torch.Generator().manual_seed(21)
    out = []
    for k, _ in enumerate(cams):
        rgba = torch.rand((4, H, W), generator=g)
        rgba[3][rgba[3] < 0.1] = 0.0
        rgba[3][rgba[3] > 0.7] = 1.0
        out.append(camera_alpha_mask(rgba, train_test_exp=True, is_test_view=(k == 2), is_test_dataset=False).to(DEV))
    return out


def make_trainer(hip, fused, P=30000, W=480, H=320, n_cams=4):
    from simple_knn._C import distCUDA2
    sc = synthetic.trained_like(P, seed=3, sh_degree=3, knn=lambda x: distCUDA2(x.to(DEV)).cpu())
    cams = [camera_to(c, DEV) for c in synthetic.orbit_cameras(W, H)[:n_cams]]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand((3, H, W), generator=g).to(DEV) for _ in cams]
    model = GaussianModelLite(sc, DEV, api=hip.api)
    model.enable_exposure(len(cams))
    crit = lgdwt_loss.criterion(dwt_enable=True, patch_dwt_enable=True)
    tr = Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, torch.zeros(3, device=DEV),
                 optimizer_step=True, alpha_masks=alpha_masks(cams, W, H))
    tr.FUSED_STEP = fused
    return tr


def test_train_step_with_exposure_alpha_and_random_background_keeps_the_fast_form(hip):
    from gsplat_amd.optim import ExposureAdam
    old = hip.binning
    hip.binning = "region"
    hip._cam_cache.clear()
    try:
        a, b = make_trainer(hip, False), make_trainer(hip, True)
        assert isinstance(b.model.exposure_optimizer, ExposureAdam)
        opt = TrainOptions(random_background=True, seed=2)
        la, lb, paths = [], [], []
        for it in range(1, 6):
            la.append(float(a.train_iteration(it, opt)["loss"]))
            lb.append(float(b.train_iteration(it, opt)["loss"]))
            paths.append((a.last["path"], b.last["path"]))
        torch.cuda.synchronize()
    finally:
        hip.binning = old
        hip._cam_cache.clear()
    assert all(p == ("unfused", "manual") for p in paths), paths
    assert torch.equal(a.bg, b.bg)      # the same backgrounds were drawn
    print("losses", la, lb)
    assert max(abs(x - y) for x, y in zip(la, lb)) <= 1e-3 * max(la)
    d = (a.model.flat - b.model.flat).double()
    assert float(d.pow(2).mean().sqrt()) <= 1e-4 * float(a.model.flat.double().pow(2).mean().sqrt())
    for x, y in ((a.model.optimizer.exp_avg, b.model.optimizer.exp_avg), (a.model.optimizer.exp_avg_sq, b.model.optimizer.exp_avg_sq)):
        assert float((x - y).double().pow(2).mean().sqrt()) <= 1e-2 * float(x.double().pow(2).mean().sqrt())
    ea, eb = a.model.exposure.detach(), b.model.exposure.detach()
    eye = torch.eye(3, 4, device=DEV)
    moved = float((ea - eye).abs().max())
    print("exposure moved by %.3e, forms differ by %.3e" % (moved, float((ea - eb).abs().max())))
    assert moved > 1e-3
    assert float((ea - eb).abs().max()) <= 0.05 * moved
    assert a.model.exposure_optimizer.steps == b.model.exposure_optimizer.steps == 5


def test_deferred_depth_limits_with_an_exposure(hip):
    """The deferred depth-limited mode no longer drops out for a trained exposure: camera 1's limits are sabotaged, the step
    that used them changes neither the model nor the exposure, the repeat steps the exposure once, and the run is the
    un-limited run."""
    from test_gpu_depth_limit import make
    old = (hip.tile_cull, hip.depth_limit_on)
    hip.tile_cull = hip.depth_limit_on = True
    hip._cam_cache.clear()
    try:
        a, b = make(hip), make(hip)
        for t in (a, b):
            t.model.enable_exposure(len(t.cameras))
        hip.depth_limit_on = False
        b.depth_limit = "deferred"
        la = [float(a.step(k)) for k in range(12)]
        lb = [b.step(k) for k in range(5)]
        b.sync()
        assert b.last["path"] == "manual"
        used0 = hip.depth_limit_stats["used"]
        hip.camera_entry(480, 320, camera_key=("trainer", b.uid, 1))["limit"].fill_(1e-3)
        failed0 = hip.depth_limit_stats["failed"]
        before = (b.model.flat.detach().clone(), b.model.exposure.detach().clone())
        lb.append(b.step(5))
        torch.cuda.synchronize()
        assert hip.depth_limit_stats["used"] > used0, "the step ran with limits (no fallback to the slow form)"
        assert torch.equal(before[0], b.model.flat.detach()) and torch.equal(before[1], b.model.exposure.detach())
        assert b.model.exposure_optimizer.steps == 6
        lb += [b.step(k) for k in range(6, 12)]
        b.sync()
    finally:
        hip.tile_cull, hip.depth_limit_on = old
        hip._cam_cache.clear()
    assert hip.depth_limit_stats["failed"] >= failed0 + 1
    assert b.model.optimizer.t == 12 and b.model.exposure_optimizer.steps == 12 == a.model.exposure_optimizer.steps
    lb = [float(x) for x in lb]
    assert max(abs(x - y) for x, y in zip(la, lb)) <= 1e-3 * max(la)
    d = (a.model.flat - b.model.flat).double()
    assert float(d.pow(2).mean().sqrt()) <= 1e-4 * float(a.model.flat.double().pow(2).mean().sqrt())
    ea, eb = a.model.exposure.detach(), b.model.exposure.detach()
    moved = float((ea - torch.eye(3, 4, device=DEV)).abs().max())
    print("exposure moved by %.3e, runs differ by %.3e" % (moved, float((ea - eb).abs().max())))
    assert moved > 1e-4 and float((ea - eb).abs().max()) <= 0.05 * moved
