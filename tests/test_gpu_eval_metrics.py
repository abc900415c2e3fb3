"""Test-set evaluation on the device (csrc/gs_eval.hip, gsplat_amd/evaluate.py) against the float64 restatement
tests/eval_reference.py on the same float32 inputs, and against the reference's recorded values (tests/golden/eval_metrics.npz).

Bars (set by the formats, not by what the kernel gives):
  mse, l1, count  relative 1e-6: the transformed pixels are the restatement's float32 values, their differences are within
                  2^-24 relative, the sums are float64; x10 margin
  psnr            1e-5 dB: 20 / ln 10 / 2 = 4.34 x that relative error, x10 margin
  ssim            relative 2e-5: the bar tests/test_gpu_loss_parity.py holds the criterion's SSIM value to
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_reference as ref
from gsplat_amd import evaluate

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
E_NULL, E_SHAPE = -1, -2
SHAPES = [(1, 1), (5, 7), (32, 32), (33, 40), (31, 65), (64, 96), (131, 260)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]
WORDS = ("mse", "psnr", "ssim", "l1", "count")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")


def assert_close(got, want, extra=None, what=""):
    """got / want: {word: float}; extra: {word: margin added to the bar}"""
    for k in WORDS:
        g, w, e = float(got[k]), float(want[k]), 0.0 if extra is None else float(extra[k])
        print("%s %-5s got %.17g want %.17g" % (what, k, g, w))
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, k, g, w)
            continue
        bar = {"mse": 1e-6 * abs(w), "l1": 1e-6 * abs(w), "count": 1e-6 * abs(w), "psnr": 1e-5, "ssim": 2e-5 * abs(w)}[k]
        assert abs(g - w) <= bar + e, (what, k, g, w, abs(g - w), bar + e)


def host(out):
    return {k: float(out[k]) for k in WORDS}


_inputs = {}


def inputs(Cn, H, W):
    """One seeded pair (values beyond [0, 1]) and one grey mask per shape, and the restatement's answers, computed once."""
    key = (Cn, H, W)
    if key not in _inputs:
        render, gt = ref.seeded_pair(Cn, H, W, seed=100 + 7 * H + W + Cn, spread=0.2)
        mask = ref.seeded_mask(H, W, seed=H + W)
        mask.view(-1)[0] = 1.0   # (never an empty selection here: that case has its own test)
        _inputs[key] = dict(render=render, gt=gt, mask=mask, dev=(render.to(DEV), gt.to(DEV), mask.to(DEV)), want={})
    return _inputs[key]


def wanted(inp, masked, clamp, quantise):
    k = (masked, clamp, quantise)
    if k not in inp["want"]:
        inp["want"][k] = ref.metrics(inp["render"], inp["gt"], inp["mask"] if masked else None, clamp, quantise)
    return inp["want"][k]


def raw_call(hip, render, gt, mask, flags, tmp=None, qout=None, C1=evaluate.C1, C2=evaluate.C2):
    """gs_eval_metrics itself -> (status, the 8 doubles as a device tensor)"""
    Cn, H, W = render.shape
    if tmp is None:
        tmp = torch.empty((int(hip.api.raw("eval_tmp_bytes")(Cn, H, W)),), dtype=torch.uint8, device=DEV)
    row = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    rc = hip.api.raw("eval_metrics")(render.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), Cn, H, W, flags,
                                     C1, C2, tmp.data_ptr(), tmp.numel(), row.data_ptr(),
                                     None if qout is None else qout.data_ptr(), None)
    return rc, row


def bits(t):
    return t.contiguous().view(torch.int64).cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask_dtu"])
@pytest.mark.parametrize("clamp,quantise", FLAGS, ids=["none", "clamp", "quantise", "clamp_quantise"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_metrics_match_the_float64_restatement(hip, H, W, Cn, clamp, quantise, masked):
    inp = inputs(Cn, H, W)
    r, g, m = inp["dev"]
    got = evaluate.image_metrics(r, g, mask=m if masked else None, clamp=clamp, quantise=quantise)
    want = wanted(inp, masked, clamp, quantise)
    assert_close(host(got), want, what="%dx%dx%d" % (Cn, H, W))
    assert all(got[k].dtype == torch.float64 and got[k].dim() == 0 and got[k].is_cuda for k in WORDS)
    assert want["count"] == (Cn * H * W if not masked else Cn * int((inp["mask"] == 1).sum()))


def test_four_channels_and_batched_shape(hip):
    render, gt = ref.seeded_pair(4, 33, 40, seed=9, spread=0.1)
    got = evaluate.image_metrics(render.to(DEV)[None], gt.to(DEV)[None], clamp=True, quantise=True)
    assert_close(host(got), ref.metrics(render, gt, None, True, True), what="4x33x40")
    with pytest.raises(ValueError, match="batch 1 only"):
        evaluate.image_metrics(torch.zeros(2, 3, 8, 8, device=DEV), torch.zeros(2, 3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="fp32 only"):
        evaluate.image_metrics(torch.zeros(3, 8, 8, device=DEV, dtype=torch.float64), torch.zeros(3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="differ in shape"):
        evaluate.image_metrics(torch.zeros(3, 8, 8, device=DEV), torch.zeros(3, 8, 9, device=DEV))
    with pytest.raises(ValueError, match="mask"):
        evaluate.image_metrics(torch.zeros(3, 8, 8, device=DEV), torch.zeros(3, 8, 8, device=DEV), mask=torch.ones(8, 9, device=DEV))


def test_fixture_cases_against_the_references_recorded_values(hip):
    z = np.load(GOLDEN)
    names = json.loads(str(z["metrics"]))
    for c in json.loads(str(z["cases"])):
        render, gt = ref.seeded_pair(3, c["H"], c["W"], c["seed"], c["spread"])
        mask = ref.seeded_mask(c["H"], c["W"], c["mask_seed"]) if c["masked"] else None
        sums = [float(render.double().sum()), float(gt.double().sum()), float(mask.double().sum()) if c["masked"] else 0.0]
        assert np.allclose(sums, z[c["key"] + "_checksum"], rtol=1e-12, atol=0), "the seeded inputs are not the generator's"
        got = evaluate.image_metrics(render.to(DEV), gt.to(DEV), mask=None if mask is None else mask.to(DEV), clamp=c["clamp"],
                                     quantise=c["quantise"])
        want = dict(zip(names, z[c["key"] + "_ref"]))
        dist = dict(zip(names, z[c["key"] + "_dist"]))
        assert_close(host(got), want, extra=dist, what=c["key"])


def edge_image():
    """(k + 0.5) / 255 for every k in 0..254, formed in float32 and in float64, each with its float32 neighbours on both
    sides, and 0, 1, -0.25, 1.75, -0.0: 1 x 40 x 39 (the rest zeros)."""
    k = torch.arange(255, dtype=torch.float32)
    mids = torch.cat([k.add(0.5).div(255), ((k.double() + 0.5) / 255).float()])
    up = torch.nextafter(mids, torch.full_like(mids, 2.0))
    down = torch.nextafter(mids, torch.full_like(mids, -1.0))
    vals = torch.cat([mids, up, down, torch.tensor([0.0, 1.0, -0.25, 1.75, -0.0])])
    img = torch.zeros(40 * 39)
    img[: vals.numel()] = vals
    return img.reshape(1, 40, 39).contiguous()


@pytest.mark.parametrize("clamp,quantise", FLAGS, ids=["none", "clamp", "quantise", "clamp_quantise"])
def test_quantised_bytes_are_torchs_bytes_exactly(hip, clamp, quantise):
    rnd = ref.seeded_pair(3, 33, 40, seed=4, spread=0.3)[0]
    for name, img in (("random", rnd), ("edges", edge_image())):
        want = ref.to_bytes(img).permute(1, 2, 0).contiguous()
        d = img.to(DEV)
        assert torch.equal(ref.to_bytes(d).permute(1, 2, 0).cpu(), want), "torch's own bytes differ between host and device"
        out = evaluate.image_metrics(d, d.flip(-1).contiguous(), clamp=clamp, quantise=quantise, return_bytes=True)
        got = out["bytes"]
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
        wrong = (got.cpu() != want).nonzero()
        assert wrong.numel() == 0, (name, wrong[:8].tolist())
    # with a mask the bytes are still those of the plain render
    m = ref.seeded_mask(33, 40, seed=2).to(DEV)
    d = rnd.to(DEV)
    got = evaluate.image_metrics(d, d, mask=m, clamp=clamp, quantise=quantise, return_bytes=True)["bytes"]
    assert torch.equal(got.cpu(), ref.to_bytes(rnd).permute(1, 2, 0))


def test_identical_images(hip):
    for Cn, H, W in ((3, 33, 40), (1, 1, 1)):
        img = ref.seeded_pair(Cn, H, W, seed=3)[0].to(DEV)
        for clamp, quantise in FLAGS:
            got = host(evaluate.image_metrics(img, img.clone(), clamp=clamp, quantise=quantise))
            assert got["psnr"] == float("inf") and got["mse"] == 0.0 and got["l1"] == 0.0, got
            assert abs(got["ssim"] - 1.0) <= 2e-5 and got["count"] == Cn * H * W, got


def test_empty_and_full_masks(hip):
    inp = inputs(3, 33, 40)
    r, g, _ = inp["dev"]
    got = host(evaluate.image_metrics(r, g, mask=torch.zeros(33, 40, device=DEV), quantise=True))
    assert math.isnan(got["psnr"]) and math.isnan(got["mse"]) and got["count"] == 0.0, got
    # everything is white under an all-zero mask: the blended images are identical
    assert math.isfinite(got["ssim"]) and math.isfinite(got["l1"]) and got["l1"] == 0.0 and abs(got["ssim"] - 1.0) <= 2e-5
    for flags in (0, 1, 2, 3):
        rc0, plain = raw_call(hip, r, g, None, flags)
        rc1, ones = raw_call(hip, r, g, torch.ones(33, 40, device=DEV), flags | evaluate.MASK_DTU)
        assert rc0 == 0 and rc1 == 0
        assert torch.equal(bits(plain), bits(ones)), (flags, plain.tolist(), ones.tolist())


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask_dtu"])
def test_same_bits_on_every_run_and_from_nan_scratch(hip, masked):
    inp = inputs(3, 131, 260)
    r, g, m = inp["dev"]
    flags = evaluate.CLAMP | evaluate.QUANTISE | (evaluate.MASK_DTU if masked else 0)
    rc, first = raw_call(hip, r, g, m if masked else None, flags)
    rc2, second = raw_call(hip, r, g, m if masked else None, flags)
    nbytes = int(hip.api.raw("eval_tmp_bytes")(3, 131, 260))
    tmp = torch.full((nbytes // 8 + 4,), float("nan"), dtype=torch.float64, device=DEV).view(torch.uint8)
    rc3, third = raw_call(hip, r, g, m if masked else None, flags, tmp=tmp)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert torch.equal(bits(first), bits(second)) and torch.equal(bits(first), bits(third)), (first.tolist(), third.tolist())
    assert first[5:].tolist() == [0.0, 0.0, 0.0]
    # nothing was written beyond the bytes the size query names
    assert bool(torch.isnan(tmp.view(torch.float64)[nbytes // 8:]).all())
    n = int(hip.api.raw("eval_partials_count")(3, 131, 260))
    assert not bool(torch.isnan(tmp.view(torch.float64)[: 5 * n]).any()), "a partial was left unwritten"


def test_evaluator_rows_in_any_order(hip):
    Cn, H, W = 3, 33, 40
    pairs = [ref.seeded_pair(Cn, H, W, seed=40 + i, spread=0.1) for i in range(5)]
    dev = [(a.to(DEV), b.to(DEV)) for a, b in pairs]
    ev = evaluate.Evaluator(7, Cn, H, W, DEV)
    initial = bits(ev.table)
    order = [3, 0, 4, 1, 2]
    for i in order:
        ev.add(i, dev[i][0], dev[i][1], clamp=True, quantise=True)
    table = bits(ev.table)
    for i in range(5):
        single = evaluate.image_metrics(dev[i][0], dev[i][1], clamp=True, quantise=True)
        rc, row = raw_call(hip, dev[i][0], dev[i][1], None, evaluate.CLAMP | evaluate.QUANTISE)
        assert rc == 0 and torch.equal(table[i], bits(row)), i
        assert float(single["psnr"]) == float(ev.table[i, 1]) and float(single["ssim"]) == float(ev.table[i, 2])
    assert torch.equal(table[5:], initial[5:]), "rows no view was added to were written"
    five = evaluate.Evaluator(5, Cn, H, W, DEV)
    for i in range(5):
        five.add(i, dev[i][0], dev[i][1], clamp=True, quantise=True)
    res = five.result(names=["v%d" % i for i in range(5)])
    want = [ref.metrics(a, b, None, True, True) for a, b in pairs]
    assert abs(res["PSNR"] - sum(w["psnr"] for w in want) / 5) <= 1e-5
    assert abs(res["SSIM"] - sum(w["ssim"] for w in want) / 5) <= 2e-5
    assert abs(res["L1"] - sum(w["l1"] for w in want) / 5) <= 1e-6
    assert list(res["per_view"]["PSNR"]) == ["v%d" % i for i in range(5)]
    with pytest.raises(ValueError, match="table was built for"):
        ev.add(0, torch.zeros(3, 32, 40, device=DEV), torch.zeros(3, 32, 40, device=DEV))
    with pytest.raises(ValueError, match="outside"):
        ev.add(7, dev[0][0], dev[0][1])


def test_reference_named_psnr_and_ssim(hip):
    pairs = [ref.seeded_pair(3, 37, 53, seed=60 + i) for i in range(2)]
    a = torch.stack([p[0] for p in pairs]).to(DEV)
    b = torch.stack([p[1] for p in pairs]).to(DEV)
    p, s = evaluate.psnr(a, b), evaluate.ssim(a, b)
    assert tuple(p.shape) == (2, 1) and s.dim() == 0 and p.dtype == torch.float32 and s.dtype == torch.float32
    want = [ref.metrics(x, y) for x, y in pairs]
    for i in range(2):
        assert abs(float(p[i, 0]) - want[i]["psnr"]) <= 1e-5 + 2.0 ** -24 * want[i]["psnr"]   # (+ the float32 it is returned in)
    ws = (want[0]["ssim"] + want[1]["ssim"]) / 2
    assert abs(float(s) - ws) <= (2e-5 + 2.0 ** -24) * ws
    assert tuple(evaluate.psnr(a[0], b[0]).shape) == (1, 1)


def test_abi_errors_return_before_anything_is_launched(hip):
    f = hip.api.raw("eval_metrics")
    img = torch.rand(3, 32, 32, device=DEV)
    m = torch.ones(32, 32, device=DEV)
    nb = int(hip.api.raw("eval_tmp_bytes")(3, 32, 32))
    tmp = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    row = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    c1, c2 = evaluate.C1, evaluate.C2
    assert f(None, p(img), None, 3, 32, 32, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_NULL
    assert f(p(img), None, None, 3, 32, 32, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_NULL
    assert f(p(img), p(img), None, 3, 32, 32, 0, c1, c2, None, nb, p(row), None, None) == E_NULL
    assert f(p(img), p(img), None, 3, 32, 32, 0, c1, c2, p(tmp), nb, None, None, None) == E_NULL
    assert f(p(img), p(img), None, 3, 32, 32, 4, c1, c2, p(tmp), nb, p(row), None, None) == E_NULL    # MASK_DTU without a mask
    assert f(p(img), p(img), None, 3, 0, 32, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE
    assert f(p(img), p(img), None, 3, 32, -1, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE
    assert f(p(img), p(img), None, 0, 32, 32, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE
    assert f(p(img), p(img), None, 5, 32, 32, 0, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE
    assert f(p(img), p(img), None, 3, 32, 32, 0, c1, c2, p(tmp), nb - 1, p(row), None, None) == E_SHAPE
    assert f(p(img), p(img), p(m), 3, 32, 32, 8, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE    # unknown flag bit
    assert f(p(img), p(img), p(m), 3, 32, 32, -1, c1, c2, p(tmp), nb, p(row), None, None) == E_SHAPE
    torch.cuda.synchronize()
    assert row.tolist() == [-7.0] * 8 and int(tmp.max()) == 0, "a refused call wrote something"
    assert f(p(img), p(img), p(m), 3, 32, 32, 7, c1, c2, p(tmp), nb, p(row), None, None) == 0
    torch.cuda.synchronize()
    assert row[4].item() == 3 * 32 * 32 and row[0].item() == 0.0


# ---------------------------------------------------------------------------------------------- end to end
def small_trainer(hip, P=300, W=64, H=64):
    import diff_gaussian_rasterization as dgr
    import lgdwt_loss
    from gsplat_amd import synthetic
    from gsplat_amd.trainer import GaussianModelLite, Trainer, camera_to
    from gsplat_amd.trainer import render
    sc = synthetic.trained_like(P, seed=0, scale_mult=1.5)
    cams = [camera_to(c, DEV) for c in synthetic.orbit_cameras(W, H)[:3]]
    # the ground truth is what a test set is to a trained model: renders of a slightly different scene, plus sensor noise
    g = torch.Generator().manual_seed(5)
    target = GaussianModelLite(dict(sc, shs=sc["shs"] + 0.05 * torch.randn(sc["shs"].shape, generator=g)), DEV, api=hip.api)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        gts = [(render(c, target, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, bg)["render"]
                + 0.02 * torch.randn((3, H, W), generator=g).to(DEV)).clamp(0, 1).contiguous() for c in cams]
    model = GaussianModelLite(sc, DEV, api=hip.api)
    crit = lgdwt_loss.criterion(dwt_enable=False, patch_dwt_enable=False)
    return Trainer(model, cams, gts, crit, dgr.GaussianRasterizer, dgr.GaussianRasterizationSettings, torch.zeros(3, device=DEV))


def test_evaluate_views_equals_the_restatement_on_the_same_renders(hip):
    from gsplat_amd.trainer import render
    tr = small_trainer(hip)
    R, S = tr.Rasterizer, tr.Settings
    with torch.no_grad():
        renders = [render(c, tr.model, R, S, tr.bg, clamp=False)["render"].clone() for c in tr.cameras]
    assert float(renders[0].abs().max()) > 0
    names = ["a.png", "b.png", "c.png"]
    res = evaluate.evaluate_views(tr.model, tr.cameras, tr.gts, R, S, tr.bg, names=names)
    want = [ref.metrics(r, g, None, True, True) for r, g in zip(renders, tr.gts)]
    for i, n in enumerate(names):
        got = {"psnr": res["per_view"]["PSNR"][n], "ssim": res["per_view"]["SSIM"][n], "l1": res["per_view"]["L1"][n],
               "mse": want[i]["mse"], "count": want[i]["count"]}   # (the result carries the three reported metrics)
        assert_close(got, want[i], what=n)
    assert abs(res["PSNR"] - sum(w["psnr"] for w in want) / 3) <= 1e-5
    assert abs(res["SSIM"] - sum(w["ssim"] for w in want) / 3) <= 2e-5
    # unquantised, unclamped, masked: the flags reach the kernel
    m = ref.seeded_mask(64, 64, seed=1)
    res2 = evaluate.evaluate_views(tr.model, tr.cameras, tr.gts, R, S, tr.bg, quantise=False, clamp=False, masks=[m.to(DEV)] * 3)
    w2 = ref.metrics(renders[1], tr.gts[1], m, False, False)
    assert abs(res2["per_view"]["PSNR"]["00001.png"] - w2["psnr"]) <= 1e-5
    assert abs(res2["per_view"]["SSIM"]["00001.png"] - w2["ssim"]) <= 2e-5 * w2["ssim"]


def test_trainer_evaluate_leaves_training_alone(hip):
    from gsplat_amd.trainer import TrainOptions
    opt = TrainOptions()
    a, b = small_trainer(hip), small_trainer(hip)
    results = []
    for tr, evaluate_between in ((a, True), (b, False)):
        tr.train_iteration(1, opt)
        if evaluate_between:
            results.append(tr.evaluate())
            results.append(tr.evaluate(names=["x", "y", "z"], quantise=False))
        tr.train_iteration(2, opt)
        tr.sync()
    torch.cuda.synchronize()
    assert a.last["path"] == b.last["path"]
    assert torch.equal(a.model.flat, b.model.flat)
    assert torch.equal(a.model.optimizer.exp_avg, b.model.optimizer.exp_avg)
    assert torch.equal(a.model.optimizer.exp_avg_sq, b.model.optimizer.exp_avg_sq)
    assert a.model.optimizer.t == b.model.optimizer.t
    assert set(results[0]) == {"SSIM", "PSNR", "L1", "per_view"} and len(results[0]["per_view"]["PSNR"]) == 3
    assert math.isfinite(results[0]["PSNR"]) and 0 < results[0]["SSIM"] < 1 and list(results[1]["per_view"]["L1"]) == ["x", "y", "z"]
