"""csrc/gs_lpips.hip on the GPU, stage by stage and as a whole (gsplat_amd/lpips.py, lpipsPyTorch/, evaluate, render_set).

  convolution   integer data: == F.conv2d + ReLU on the CPU (every partial sum an integer below 2^24, so exact in any order);
                random data: every element within the any-order fp32 bound (9 Cin + 2) 2^-24 (sum |w x| + |b|) of the float64
                twin, the sum evaluated in float64 (ReLU is 1-Lipschitz, so the bound holds after it)
  pool          == F.max_pool2d
  distance      against the float64 twin on the same fp32 features: n 2^-52 relative with non-negative lin weights, n the
                number of terms summed (C H W); the same factor times the sum of the terms' absolute values with signed ones
  whole call    the golden cases (the reference's own module in float64) and each per-tap term, relative, at 8 x the largest
                float32-to-float64 relative distance of the reference itself over the table (recorded in the golden; the factor
                8 for the summation order of a k-ordered MFMA chain over K up to 4 608)
The measured whole-call distances go to the file LPIPS_PARITY_OUT names, when it is set (profiles/lpips_parity.json is one
such run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_cases as cases
import lpips_reference as ref
from test_lpips_cpu import NAMES, golden, whole_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}


@functools.lru_cache(maxsize=None)
def weights():
    from gsplat_amd.lpips import LpipsWeights
    return LpipsWeights.from_state_dicts(*cases.make_state_dicts())


def case_images(name):
    g = golden()
    return cases.planar(g[name + "/render_u8"]).to(DEV), cases.planar(g[name + "/gt_u8"]).to(DEV)


# ------------------------------------------------------------------------------------------------ 1, 2: convolution
def _conv_sizes(cout):
    return cases.CONV_SIZES + (cases.large_tile_size(cout),)


@pytest.mark.parametrize("pair", cases.PAIRS, ids=lambda p: "%dto%d" % p)
def test_convolution_is_exact_on_integer_data(pair):
    from gsplat_amd.lpips import conv3x3_relu
    cin, cout = pair
    for k, (H, W) in enumerate(_conv_sizes(cout)):
        x, w, b = cases.int_conv_case(cin, cout, H, W, 100 + k)
        want = ref.conv3x3_relu(x, w, b)
        got = conv3x3_relu(x.to(DEV), w.to(DEV), b.to(DEV)).cpu()
        assert got.shape == want.shape
        assert torch.equal(got, want), "%d->%d at %dx%d: %d of %d elements differ, first at %s" % (
            cin, cout, H, W, int((got != want).sum()), want.numel(), (got != want).nonzero()[0].tolist())
        assert float(want.max()) > 0


@pytest.mark.parametrize("pair", cases.PAIRS, ids=lambda p: "%dto%d" % p)
def test_convolution_on_random_data_is_within_the_any_order_bound(pair):
    from gsplat_amd.lpips import conv3x3_relu
    cin, cout = pair
    for k, (H, W) in enumerate((cases.RANDOM_CONV_SMALL, cases.large_tile_size(cout))):
        x, w, b = cases.random_conv_case(cin, cout, H, W, 200 + k)
        x64, w64, b64 = x.double(), w.double(), b.double()
        want = ref.conv3x3_relu(x64, w64, b64)
        mag = F.conv2d(x64.abs(), w64.abs(), b64.abs(), padding=1)
        bound = (9 * cin + 2) * 2.0 ** -24 * mag
        got = conv3x3_relu(x.to(DEV), w.to(DEV), b.to(DEV)).cpu().double()
        err = (got - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("%d->%d at %dx%d: worst error %.3g of the bound" % (cin, cout, H, W, worst))
        assert bool((err <= bound).all()), "%d->%d at %dx%d: %.3g of the bound" % (cin, cout, H, W, worst)


def test_convolution_does_not_depend_on_the_slot():
    from gsplat_amd.lpips import conv3x3_relu
    x, w, b = cases.random_conv_case(64, 128, 19, 45, 7)
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
    y = conv3x3_relu(x, w, b)
    assert torch.equal(conv3x3_relu(x.flip(0).contiguous(), w, b), y.flip(0))
    assert torch.equal(conv3x3_relu(x[:1].contiguous(), w, b), y[:1])
    assert torch.equal(conv3x3_relu(x, w, b), y)


# ------------------------------------------------------------------------------------------------ 3: pool
@pytest.mark.parametrize("size", cases.POOL_SIZES, ids=lambda s: "%dx%d" % s)
def test_pool_is_exact(size):
    from gsplat_amd.lpips import maxpool2
    H, W = size
    x = torch.from_numpy(np.random.default_rng(H * 100 + W).standard_normal((2, 3, H, W)).astype(np.float32))
    want = F.max_pool2d(x, 2, 2)
    got = maxpool2(x.to(DEV)).cpu()
    assert got.shape == want.shape == (2, 3, H // 2, W // 2) and torch.equal(got, want)


def test_pool_below_two_pixels_raises():
    from gsplat_amd.lpips import maxpool2
    with pytest.raises(ValueError):
        maxpool2(torch.zeros(1, 1, 1, 5, device=DEV))


# ------------------------------------------------------------------------------------------------ 4: distance
@pytest.mark.parametrize("shape", cases.DIST_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("signed", (False, True), ids=("lin_nonneg", "lin_signed"))
def test_distance_against_the_float64_twin(shape, signed):
    from gsplat_amd.lpips import tap_distance
    C, H, W = shape
    fx, fy, lin = cases.dist_case(C, H, W, 300 + C + H, signed_lin=signed, zero_pixel=True)
    want, terms = ref.distance(fx, fy, lin, return_terms=True)
    got = float(tap_distance(fx.to(DEV), fy.to(DEV), lin.to(DEV)))
    n = C * H * W
    scale = float(terms.abs().sum()) / (H * W)     # = |want| when no term is negative
    if not signed:
        assert abs(scale - abs(float(want))) <= 1e-15 * scale
    err = abs(got - float(want))
    print("C %d %dx%d %s: %.3g of the bar" % (C, H, W, "signed" if signed else "non-negative", err / (n * 2.0 ** -52 * scale)))
    assert err <= n * 2.0 ** -52 * scale


def test_distance_of_identical_features_is_exactly_zero_and_a_zero_pixel_adds_nothing():
    from gsplat_amd.lpips import tap_distance
    fx, fy, lin = cases.dist_case(64, 23, 31, 5, zero_pixel=True)
    fx, fy, lin = fx.to(DEV), fy.to(DEV), lin.to(DEV)
    assert float(tap_distance(fx, fx.clone(), lin)) == 0.0
    # the zero-norm pixel: with fy zero there too it contributes exactly 0, so the mean is that of the other pixels
    fy0 = fy.clone()
    fy0[:, 0, 0] = 0.0
    want = ref.distance(fx.cpu(), fy0.cpu(), lin.cpu())
    got = float(tap_distance(fx, fy0, lin))
    assert np.isfinite(got) and abs(got - float(want)) <= 64 * 23 * 31 * 2.0 ** -52 * abs(float(want))
    one = tap_distance(fx[:, :1, :1].contiguous(), fy0[:, :1, :1].contiguous(), lin)
    assert float(one) == 0.0
    assert float(tap_distance(fx, fy, lin)) == float(tap_distance(fy, fx, lin))


# ------------------------------------------------------------------------------------------------ 5: whole call
@pytest.mark.parametrize("name", NAMES)
def test_whole_call_against_the_golden(name):
    from gsplat_amd.lpips import lpips_vgg
    g = golden()
    render, gt = case_images(name)
    val, taps = lpips_vgg(render, gt, weights(), return_taps=True)
    val, taps = float(val), taps.cpu().numpy()
    want, want_taps = float(g[name + "/lpips_f64"]), g[name + "/taps_f64"]
    rel = abs(val - want) / abs(want)
    rel_taps = [abs(float(taps[k]) - want_taps[k]) / abs(want_taps[k]) for k in range(5)]
    bar = whole_bar()
    MEASURED[name] = {"lpips_hip": val, "lpips_reference_f64": want, "rel": rel, "rel_taps": rel_taps,
                      "reference_f32_rel": float(g[name + "/rel_f32_f64"]), "bar": bar}
    print("%s: HIP %.3e from the reference's float64 (its own float32: %.3e; bar %.3e); taps %s"
          % (name, rel, float(g[name + "/rel_f32_f64"]), bar, ["%.2e" % r for r in rel_taps]))
    out = os.environ.get("LPIPS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1)
    assert rel <= bar
    assert max(rel_taps) <= bar, rel_taps
    assert (((taps[0] + taps[1]) + taps[2]) + taps[3]) + taps[4] == val


def test_whole_call_identical_swapped_repeated():
    from gsplat_amd.lpips import lpips_vgg
    render, gt = case_images("35x50")
    w = weights()
    a, ta = lpips_vgg(render, gt, w, return_taps=True)
    b, tb = lpips_vgg(gt, render, w, return_taps=True)
    c, tc = lpips_vgg(render, gt, w, return_taps=True)
    assert torch.equal(a, b) and torch.equal(ta, tb), "swapping the images changes the bits"
    assert torch.equal(a, c) and torch.equal(ta, tc), "two calls differ"
    z, tz = lpips_vgg(render, render.clone(), w, return_taps=True)
    assert float(z) == 0.0 and float(tz.abs().max()) == 0.0
    assert a.dtype == torch.float64 and a.dim() == 0 and float(a) > 0


def test_whole_call_stays_inside_its_scratch():
    from gsplat_amd import lpips as impl
    render, gt = case_images("17x19")
    n, G = impl.tmp_bytes(17, 19), 1 << 16
    assert n > 0
    buf = torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    val = impl.lpips_vgg(render, gt, weights(), tmp=buf[G:G + n])
    assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + n:] == 0xA5).all()), "the call wrote outside gs_lpips_tmp_bytes"
    assert torch.equal(val, impl.lpips_vgg(render, gt, weights()))
    from gsplat_amd import GsError
    with pytest.raises(GsError):
        impl.lpips_vgg(render, gt, weights(), tmp=buf[G:G + n - 256])


def test_images_below_sixteen_raise():
    from gsplat_amd import lpips as impl
    x = torch.rand(3, 15, 40, device=DEV)
    with pytest.raises(ValueError, match="16"):
        impl.lpips_vgg(x, x, weights())
    assert impl.tmp_bytes(15, 40) == 0 and impl.tmp_bytes(40, 15) == 0 and impl.tmp_bytes(16, 16) > 0
    with pytest.raises(ValueError):
        impl.lpips_vgg(x[:2], x[:2], weights())


# ------------------------------------------------------------------------------------------------ 6: interfaces
def _pair(H=33, W=47, seed=11):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand((3, H, W), generator=g)
    render = gt + 0.2 * (torch.rand((3, H, W), generator=g) - 0.4)   # (leaves [0, 1]: the clamp has work to do)
    mask = (torch.rand((H, W), generator=g) > 0.4).to(torch.float32)
    return render.to(DEV), gt.to(DEV), mask.to(DEV)


def test_image_metrics_carries_lpips_and_leaves_the_other_words():
    from gsplat_amd.evaluate import image_metrics
    from gsplat_amd.lpips import lpips_vgg
    render, gt, mask = _pair()
    for kw in (dict(), dict(clamp=True, quantise=True), dict(mask=mask, quantise=True)):
        plain = image_metrics(render, gt, ssim_sk=True, **kw)
        with_lp = image_metrics(render, gt, ssim_sk=True, lpips=weights(), **kw)
        assert "lpips" not in plain and set(with_lp) == set(plain) | {"lpips"}
        for k in plain:
            assert torch.equal(plain[k], with_lp[k]) or (torch.isnan(plain[k]) and torch.isnan(with_lp[k])), k
        assert torch.equal(with_lp["lpips"], lpips_vgg(render, gt, weights(), **kw))
        # the transform in torch beforehand gives the same bits (on the CPU, where to_tensor's division is a division: the
        # device's division by a scalar multiplies by its reciprocal)
        m = None if kw.get("mask") is None else kw["mask"].cpu()
        r2 = ref.transform(render.cpu(), m, kw.get("clamp", False), kw.get("quantise", False))
        g2 = ref.transform(gt.cpu(), m, kw.get("clamp", False), kw.get("quantise", False))
        assert torch.equal(with_lp["lpips"], lpips_vgg(r2.contiguous().to(DEV), g2.contiguous().to(DEV), weights()))
    assert not torch.equal(image_metrics(render, gt, lpips=weights())["lpips"],
                           image_metrics(render, gt, lpips=weights(), mask=mask)["lpips"])


def test_evaluator_reports_lpips():
    from gsplat_amd.evaluate import Evaluator
    from gsplat_amd.lpips import lpips_vgg
    render, gt, _ = _pair()
    other, _, _ = _pair(seed=12)
    ev = Evaluator(2, 3, 33, 47, DEV, lpips=weights())
    ev.add(0, render, gt, clamp=True, quantise=True)
    ev.add(1, other, gt, clamp=True, quantise=True)
    res = ev.result(["a.png", "b.png"])
    want = [float(lpips_vgg(r, gt, weights(), clamp=True, quantise=True)) for r in (render, other)]
    assert res["per_view"]["LPIPS"] == {"a.png": want[0], "b.png": want[1]}
    assert res["LPIPS"] == sum(want) / 2
    plain = Evaluator(1, 3, 33, 47, DEV)
    plain.add(0, render, gt)
    assert "LPIPS" not in plain.result() and "LPIPS" not in plain.result()["per_view"]
    with pytest.raises(ValueError):
        Evaluator(1, 3, 15, 47, DEV, lpips=weights())


def test_evaluate_dir_writes_the_key(tmp_path):
    from gsplat_amd.render_set import evaluate_dir, write_render_set
    render, gt, _ = _pair()
    write_render_set(str(tmp_path), "test", 7, [{"render": render.clamp(0, 1), "gt": gt}])
    res = evaluate_dir(str(tmp_path), lpips=weights(), device=DEV)
    assert res["ours_7"]["LPIPS"] > 0 and list(res["ours_7"]["per_view"]["LPIPS"]) == ["00000.png"]
    full, per = json.load(open(tmp_path / "results.json")), json.load(open(tmp_path / "per_view.json"))
    assert full["ours_7"]["LPIPS"] == res["ours_7"]["LPIPS"] and per["ours_7"]["LPIPS"]["00000.png"] == res["ours_7"]["LPIPS"]
    # the files hold bytes: the same number as the quantised pair gives directly
    from gsplat_amd.lpips import lpips_vgg
    assert res["ours_7"]["LPIPS"] == float(lpips_vgg(render, gt, weights(), clamp=True, quantise=True))
    evaluate_dir(str(tmp_path), device=DEV)
    full, per = json.load(open(tmp_path / "results.json")), json.load(open(tmp_path / "per_view.json"))
    assert "LPIPS" not in full["ours_7"] and "LPIPS" not in per["ours_7"]


def test_drop_in_package_returns_the_reference_shape():
    import lpipsPyTorch
    from gsplat_amd import lpips as impl
    render, gt, _ = _pair()
    impl.set_default_weights(weights())
    try:
        got = lpipsPyTorch.lpips(render[None], gt[None], net_type="vgg")
        assert tuple(got.shape) == (1, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
        want = impl.lpips_vgg(render, gt, weights()).to(torch.float32)
        assert float(got) == float(want)
        assert torch.equal(lpipsPyTorch.LPIPS("vgg")(render, gt), got)
    finally:
        impl.set_default_weights(None)
