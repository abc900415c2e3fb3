"""LPIPS without a GPU: the torch restatement (tests/lpips_reference.py) against the golden of the reference's own module,
the weight files' parsing, and the properties the case tables of tests/lpips_cases.py are named for."""
import functools
import os

import numpy as np
import pytest
import torch

import lpips_cases as cases
import lpips_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
NAMES = [c[0] for c in cases.WHOLE_CASES]


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def weights():
    return cases.make_state_dicts()


def whole_bar():
    """GPU test 5's bar: 8 x the reference's own largest float32-to-float64 relative distance over the table"""
    g = golden()
    return 8.0 * max(float(g[n + "/rel_f32_f64"]) for n in NAMES)


def test_golden_holds_the_table():
    g = golden()
    assert int(g["weight_seed"]) == cases.WEIGHT_SEED and list(g["names"]) == NAMES
    for name, H, W, seed in cases.WHOLE_CASES:
        r8, g8 = cases.whole_images(H, W, seed)
        assert np.array_equal(g[name + "/render_u8"], r8) and np.array_equal(g[name + "/gt_u8"], g8)
        assert abs(float(g[name + "/taps_f64"].sum()) - float(g[name + "/lpips_f64"])) < 1e-15
        assert 0 < float(g[name + "/rel_f32_f64"]) < 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_reproduces_the_golden(name):
    g = golden()
    vgg, lin = weights()
    val, taps = ref.lpips(cases.planar(g[name + "/render_u8"]), cases.planar(g[name + "/gt_u8"]), vgg, lin, torch.float64)
    want, want_taps = float(g[name + "/lpips_f64"]), g[name + "/taps_f64"]
    assert abs(float(val) - want) <= 1e-12 * abs(want)
    for k in range(5):
        assert abs(float(taps[k]) - want_taps[k]) <= 1e-12 * abs(want_taps[k]), (k, float(taps[k]), want_taps[k])


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_is_inside_the_whole_call_bar(name):
    g = golden()
    vgg, lin = weights()
    val, _ = ref.lpips(cases.planar(g[name + "/render_u8"]), cases.planar(g[name + "/gt_u8"]), vgg, lin, torch.float32)
    want = float(g[name + "/lpips_f64"])
    rel = abs(float(val) - want) / abs(want)
    print("%s: float32 restatement %.3e from the float64 golden (bar %.3e)" % (name, rel, whole_bar()))
    assert rel <= whole_bar()


# ---------------------------------------------------------------------------------------------- weight files
def _small_sds(renamed=False):
    return cases.make_state_dicts(seed=3, renamed=renamed)


def test_files_in_both_key_namings_load_to_the_same_weights(tmp_path):
    from gsplat_amd.lpips import LpipsWeights
    vgg, lin = _small_sds()
    _, lin_renamed = _small_sds(renamed=True)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin_a.pth")
    torch.save(lin_renamed, tmp_path / "lin_b.pth")
    a = LpipsWeights.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin_a.pth"))
    b = LpipsWeights.from_files(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin_b.pth"))
    c = LpipsWeights.from_state_dicts(vgg, lin)
    assert len(a.conv_w) == 13 and len(a.conv_b) == 13 and len(a.lin) == 5
    for x, y, z in zip(a.conv_w + a.conv_b + a.lin, b.conv_w + b.conv_b + b.lin, c.conv_w + c.conv_b + c.lin):
        assert torch.equal(x, y) and torch.equal(x, z)
    for i, (w, bias) in enumerate(zip(a.conv_w, a.conv_b)):
        assert torch.equal(w, vgg["features.%d.weight" % cases.CONV_INDEX[i]]) and tuple(w.shape) == cases.CONV_SHAPE[i][::-1] + (3, 3)
        assert torch.equal(bias, vgg["features.%d.bias" % cases.CONV_INDEX[i]])
    for k in range(5):
        assert torch.equal(a.lin[k], lin["lin%d.model.1.weight" % k].reshape(-1))


def test_every_missing_or_misshapen_key_raises_naming_it():
    from gsplat_amd.lpips import LpipsWeights
    vgg, lin = _small_sds()
    for key in vgg:
        sd = dict(vgg)
        del sd[key]
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            LpipsWeights.from_state_dicts(sd, lin)
        sd = dict(vgg)
        sd[key] = vgg[key][..., :-1] if vgg[key].dim() == 4 else vgg[key][:-1]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            LpipsWeights.from_state_dicts(sd, lin)
    for src in (lin, _small_sds(renamed=True)[1]):
        for key in src:
            sd = dict(src)
            del sd[key]
            with pytest.raises(KeyError, match=key.replace(".", r"\.")):
                LpipsWeights.from_state_dicts(vgg, sd)
            sd = dict(src)
            sd[key] = src[key][:, :-1]
            with pytest.raises(ValueError, match=key.replace(".", r"\.")):
                LpipsWeights.from_state_dicts(vgg, sd)


def test_find_weights_names_both_files_and_fetches_nothing(tmp_path, monkeypatch):
    from gsplat_amd import lpips as impl
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    monkeypatch.setattr(torch.hub, "_hub_dir", None, raising=False)   # (a hub directory set earlier in the process wins otherwise)
    with pytest.raises(FileNotFoundError) as e:
        impl.find_weights()
    assert "vgg16-397923af.pth" in str(e.value) and "vgg.pth" in str(e.value) and str(tmp_path) in str(e.value)


def test_only_vgg_is_served():
    import lpipsPyTorch
    x = torch.zeros(3, 16, 16)
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError):
            lpipsPyTorch.lpips(x, x, net_type=net)
        with pytest.raises(NotImplementedError):
            lpipsPyTorch.LPIPS(net)
    with pytest.raises(NotImplementedError):
        lpipsPyTorch.lpips(x, x)   # the reference's default is 'alex'


# ---------------------------------------------------------------------------------------------- the tables' properties
def test_whole_cases_put_an_odd_size_in_front_of_every_pool_and_start_at_the_minimum():
    assert (cases.WHOLE_CASES[0][1], cases.WHOLE_CASES[0][2]) == (16, 16)
    assert cases.pool_sizes(16, 16)[-1] == (2, 2)    # the fifth tap of the minimum is one pixel
    for p in range(4):
        assert any(h % 2 or w % 2 for _, H, W, _ in cases.WHOLE_CASES for h, w in [cases.pool_sizes(H, W)[p]]), p


def test_integer_convolution_cases_are_exact_in_any_order():
    for cin, cout in cases.PAIRS:
        assert cases.int_conv_bound(cin) < 2 ** 24
    assert len(cases.PAIRS) == 8 and set(cases.PAIRS) == set(cases.CONV_SHAPE)
    x, w, b = cases.int_conv_case(64, 128, 33, 31, 0)
    for t, lo, hi in ((x, 0, cases.INT_X_MAX), (w, -cases.INT_W_MAX, cases.INT_W_MAX), (b, -cases.INT_B_MAX, cases.INT_B_MAX)):
        assert torch.equal(t, t.round()) and float(t.min()) >= lo and float(t.max()) <= hi
    # float32 and float64 give the same integers
    y32 = ref.conv3x3_relu(x, w, b)
    y64 = ref.conv3x3_relu(x.double(), w.double(), b.double())
    assert torch.equal(y32.double(), y64) and float(y64.max()) > 0


def test_convolution_sizes_reach_both_tile_shapes_for_every_pair():
    for cin, cout in cases.PAIRS:
        H, W = cases.large_tile_size(cout)
        assert cases.conv_workgroups_large(2, cout, H, W) >= 256 > cases.conv_workgroups_large(2, cout, H - 8, W)
        assert cases.conv_workgroups_large(2, cout, *cases.RANDOM_CONV_SMALL) < 256
        assert W % 32 == 1 and H % 8 == 1     # a one-pixel column tile and a one-row last tile


def test_distance_cases_have_a_zero_norm_pixel_that_adds_nothing():
    fx, fy, lin = cases.dist_case(64, 23, 31, 1, zero_pixel=True)
    assert float(fx[:, 0, 0].abs().max()) == 0.0 and float(fy[:, 0, 0].abs().max()) > 0
    _, terms = ref.distance(fx, fx, lin, return_terms=True)
    assert float(terms.abs().max()) == 0.0                      # identical features: exactly 0, the zero pixel included (0 / 1e-10)
    val, terms = ref.distance(fx, fy, lin, return_terms=True)
    assert torch.isfinite(terms).all() and float(val) > 0
    _, _, signed = cases.dist_case(64, 23, 31, 1, signed_lin=True)
    assert float(signed.min()) < 0 < float(signed.max()) and float(lin.min()) >= 0


def test_pool_cases_reach_a_one_pixel_output_and_both_parities():
    outs = [(h // 2, w // 2) for h, w in cases.POOL_SIZES]
    assert (1, 1) in outs and any(h % 2 for h, _ in cases.POOL_SIZES) and any(w % 2 == 0 for _, w in cases.POOL_SIZES)
