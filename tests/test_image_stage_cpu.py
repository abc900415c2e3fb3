"""What LGDWT-GS/train.py does to the render between the rasterizer and the loss, on the CPU oracle: a random background
per iteration (train.py:117), the alpha mask (train.py:121-124) and the mask a camera is built with (scene/cameras.py:43-54)."""
import torch

from gsplat_amd import synthetic
from gsplat_amd.io import camera_alpha_mask
from gsplat_amd.losses import LGDWTCriterion, LossOps
from gsplat_amd.trainer import GaussianModelLite, TrainOptions, Trainer, camera_to, render

P, W, H = 400, 96, 64


def scene(oracle):
    dev = torch.device("cpu")
    sc = synthetic.trained_like(P, seed=3, scale_mult=1.5)
    cams = [camera_to(c, dev) for c in synthetic.orbit_cameras(W, H)[:3]]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((3, H, W), generator=g) for _ in cams]
    return sc, cams, gts


def alpha_for(k):
    """zeros, fractions and a zeroed half"""
    g = torch.Generator().manual_seed(100 + k)
    a = torch.rand((1, H, W), generator=g)
    a[a < 0.2] = 0.0
    a[a > 0.8] = 1.0
    a[..., : W // 2] = 0.0
    return a


class _Recorder:
    """Settings stand-in that keeps a copy of every background the rasterizer is handed."""

    def __init__(self, Settings):
        self.Settings, self.seen = Settings, []

    def __call__(self, **kw):
        self.seen.append(torch.as_tensor(kw["bg"]).detach().cpu().clone())
        return self.Settings(**kw)


def backgrounds(oracle, seed):
    sc, cams, gts = scene(oracle)
    model = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    rec = _Recorder(oracle.Settings)
    crit = LGDWTCriterion(LossOps(oracle.api), dwt_enable=False, patch_dwt_enable=False)
    tr = Trainer(model, cams, gts, crit, oracle.Rasterizer, rec, torch.zeros(3))
    opt = TrainOptions(random_background=True, seed=seed)
    bg_ptrs = []
    for it in (1, 2, 3):
        tr.train_iteration(it, opt)
        bg_ptrs.append(tr.bg.data_ptr())
    assert len(set(bg_ptrs)) == 1, "one persistent background buffer"
    return rec.seen


def test_random_background_is_drawn_every_iteration_and_follows_the_seed(oracle):
    assert TrainOptions().random_background is False
    a = backgrounds(oracle, seed=4)
    assert len(a) == 3
    for x in a:
        assert x.shape == (3,) and float(x.min()) >= 0.0 and float(x.max()) < 1.0
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    b = backgrounds(oracle, seed=4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = backgrounds(oracle, seed=5)
    assert not torch.equal(a[0], c[0])


def test_alpha_masked_step_matches_the_reference_loop(oracle):
    """Trainer(alpha_masks=...).step(k) against a restatement of train.py:117-124 + the loss of :128-202: render -> clamp ->
    image *= alpha_mask -> criterion -> backward.  Loss and every parameter gradient agree."""
    sc, cams, gts = scene(oracle)
    masks = [alpha_for(k) for k in range(len(cams))]
    ci = 1
    m1 = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    crit1 = LGDWTCriterion(LossOps(oracle.api), patch_size=32)
    tr = Trainer(m1, cams, gts, crit1, oracle.Rasterizer, oracle.Settings, torch.zeros(3), optimizer_step=False,
                 alpha_masks=masks)
    loss1 = float(tr.step(ci))
    assert tr.last["path"] == "unfused"
    g1 = m1.flat_grad.clone()

    m2 = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    crit2 = LGDWTCriterion(LossOps(oracle.api), patch_size=32, fused=False)
    m2.zero_grad()
    pkg = render(cams[ci], m2, oracle.Rasterizer, oracle.Settings, torch.zeros(3))
    image = pkg["render"] * masks[ci]       # (render() has clamped it, gaussian_renderer/__init__.py:119)
    loss2, _ = crit2(image, gts[ci])
    loss2.backward()
    m2.collect_grads()
    g2 = m2.flat_grad

    loss2 = float(loss2.detach())
    assert abs(loss1 - loss2) < 1e-5 * max(1.0, abs(loss2))
    assert float(g2.abs().max()) > 0
    off = 0
    for name, n in m2.fields:
        a, b = g1[off:off + P * n], g2[off:off + P * n]
        off += P * n
        scale = max(float(b.abs().max()), 1e-12)
        err = float((a - b).abs().max()) / scale
        assert err < 1e-4, "dL/d%s rel err %.2e" % (name, err)
    # and the mask matters: without it the same step gives another loss
    m3 = GaussianModelLite(sc, torch.device("cpu"), api=oracle.api)
    tr3 = Trainer(m3, cams, gts, LGDWTCriterion(LossOps(oracle.api), patch_size=32), oracle.Rasterizer, oracle.Settings,
                  torch.zeros(3), optimizer_step=False)
    assert abs(float(tr3.step(ci)) - loss1) > 1e-4


def _reference_mask(image, train_test_exp, is_test_view, is_test_dataset):
    """scene/cameras.py:43-54, restated"""
    if image.shape[0] == 4:
        mask = image[3:4].clone()
    else:
        mask = torch.ones_like(image[0:1])
    if train_test_exp and is_test_view:
        half = mask.shape[-1] // 2
        if is_test_dataset:
            mask[..., :half] = 0
        else:
            mask[..., half:] = 0
    return mask


def test_camera_alpha_mask_matches_the_camera_class():
    g = torch.Generator().manual_seed(2)
    for C in (3, 4):
        for w in (31, 32):
            img = torch.rand((C, 9, w), generator=g)
            for exp, view, dataset in ((False, False, False), (False, True, True), (True, False, False), (True, True, False),
                                       (True, True, True)):
                got = camera_alpha_mask(img, train_test_exp=exp, is_test_view=view, is_test_dataset=dataset)
                want = _reference_mask(img, exp, view, dataset)
                assert got.dtype == torch.float32 and got.shape == (1, 9, w)
                assert torch.equal(got, want), (C, w, exp, view, dataset)
    img = torch.rand((4, 5, 8), generator=g)
    m = camera_alpha_mask(img, True, True, True)
    assert torch.equal(m[..., :4], torch.zeros(1, 5, 4)) and torch.equal(m[..., 4:], img[3:4, :, 4:])
    m = camera_alpha_mask(img, True, True, False)
    assert torch.equal(m[..., 4:], torch.zeros(1, 5, 4)) and torch.equal(m[..., :4], img[3:4, :, :4])
