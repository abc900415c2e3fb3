"""CPU half of the Wavelet Error Field tests (gsplat_amd/wef.py, lgdwt_loss): the module's torch restatement against the
reference's own results (tests/golden/wef_maps.npz, written by tests/golden/make_golden_wef.py), the two conditions that keep
the derived bar of tests/wef_cases.py honest, the grid layout and bytes, the titled grid, Charbonnier and the error paths.
tests/test_gpu_wef.py runs the same cases through the kernels.

Two things the reference does are NOT held against the module, and both are stated where they are skipped:
  * a plane of one coefficient (4 x 4 at level 2): the reference's float32 interpolate blurs it by an ulp and divides that by
    1e-8 (fixture: up to 4.4e-2 on LH2 / HL2 / HH2 of one_coeff_4x4 and 1.0 on its WEF, in float64 2.1e-2 on the WEF); the
    module returns the exact 0 the case table asks for.  Such maps, and a combined field built from them, are compared with
    nothing but 0.
  * a NaN pixel has no byte: the NaN case has no grid in the fixture."""
import os
import re

import numpy as np
import pytest
import torch

import torch_loss_reference as tlr
import wef_cases as wc
from gsplat_amd import wef

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = ((False, "l2"), (True, "all"))
FIXTURE_IDS = [c.name for c in wc.FIXTURE_CASES]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "wef_maps.npz"))


@pytest.fixture(scope="module")
def rest32():
    """the module's float32 restatement of every case, computed once"""
    out = {}
    for c in wc.CASES:
        pred, gt = wc.inputs(c)
        out[c.name] = {False: wef.compute_wef_maps(pred, gt), True: wef.compute_wef_all_subbands(pred[None], gt[None])}
    return out


def stacked(maps, keys):
    return torch.cat([maps[k][0] for k in keys]).numpy()


def noisy_keys(case, all_bands, ref32):
    """keys on which the reference's float32 result is rounding noise over 1e-8: flat maps it does not return as 0, and then
    the combined field built from them"""
    keys = wc.keys_of(all_bands)
    if case.kind == "nan":
        return set()
    bars = wc.bars(case, all_bands)
    bad = {k for i, k in enumerate(keys[:-1]) if bars[k] is None and np.any(ref32[i] != 0)}
    if bad:
        bad.add(keys[-1])
    return bad


def test_train_import_line():
    from lgdwt_loss import (  # noqa: F401  (LGDWT-GS/train.py:15-20 with utils.loss_utils -> lgdwt_loss)
        l1_loss, ssim, get_dwt_subbands, charbonnier_loss,
        make_heatmap_rgb, make_wef_grid_image,
        make_wef_grid_image_titled, compute_elf_map, compute_patch_dwt_loss,
        compute_wef_maps, compute_wef_all_subbands
    )
    assert compute_wef_maps is wef.compute_wef_maps and charbonnier_loss is wef.charbonnier_loss


def test_case_table_covers_the_issue():
    sizes = {(c.C, c.H, c.W) for c in wc.CASES}
    for s in ((3, 2, 2), (3, 4, 4), (3, 1, 9), (3, 5, 7), (3, 6, 9), (3, 8, 8), (3, 37, 53), (3, 3, 130), (3, 64, 96),
              (3, 70, 300), (1, 270, 480), (4, 270, 480)):
        assert s in sizes, s
    assert {"same", "corner", "padded", "nan"} <= {c.kind for c in wc.CASES}
    for name, all_bands in wc.ALL_FLAT:
        assert all(v is None for v in wc.bars(wc.BY_NAME[name], all_bands).values()), (name, all_bands)


@pytest.mark.parametrize("name", FIXTURE_IDS)
def test_inputs_are_the_fixtures(fx, name):
    pred, gt = wc.inputs(name)
    assert np.array_equal(fx["pred_" + name], pred.numpy(), equal_nan=True) and np.array_equal(fx["gt_" + name], gt.numpy())


@pytest.mark.parametrize("name", FIXTURE_IDS)
def test_restatement_float64_is_the_references(fx, name):
    """tight: both are float64 evaluations of the same statements (the bands by slices here, by conv2d there)"""
    c = wc.BY_NAME[name]
    for all_bands, tag in FORMS:
        keys = wc.keys_of(all_bands)
        ref64, ref32 = fx["maps64_%s_%s" % (name, tag)], fx["maps32_%s_%s" % (name, tag)]
        got = stacked(wc.twin(c, all_bands), keys)
        skip = noisy_keys(c, all_bands, ref32)
        for i, k in enumerate(keys):
            if k in skip:
                assert wc.bars(c, all_bands)[k] is not None or np.all(got[i] == 0), (name, tag, k)
            elif c.kind == "nan":
                assert np.isnan(got[i]).all() and np.isnan(ref64[i]).all(), (name, tag, k)
            else:
                # a flat map is 0 here; the reference may leave 1e-17 / 1e-8 there
                assert np.abs(got[i] - ref64[i]).max() <= 1e-8, (name, tag, k, np.abs(got[i] - ref64[i]).max())


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_restatement_float32_within_the_bar(rest32, name):
    c = wc.BY_NAME[name]
    for all_bands, tag in FORMS:
        dist = wc.check_maps(c, all_bands, rest32[name][all_bands], "restatement float32")
        if dist:
            print("%s %s: float32 restatement %.2e from float64, largest bar %.2e"
                  % (name, tag, max(dist.values()), max([b for b in wc.bars(c, all_bands).values() if b] or [0.0])))


@pytest.mark.parametrize("name", FIXTURE_IDS)
def test_bar_holds_the_references_own_float32(fx, name):
    """condition 1: the reference's float32 result lies within the bar of its float64 twin"""
    c = wc.BY_NAME[name]
    if c.kind == "nan":
        for _, tag in FORMS:
            assert np.isnan(fx["maps32_%s_%s" % (name, tag)]).all()
        return
    for all_bands, tag in FORMS:
        keys = wc.keys_of(all_bands)
        ref32, ref64 = fx["maps32_%s_%s" % (name, tag)], fx["maps64_%s_%s" % (name, tag)]
        skip, bars = noisy_keys(c, all_bands, ref32), wc.bars(c, all_bands)
        for i, k in enumerate(keys):
            if k in skip:
                continue
            d = float(np.abs(ref32[i].astype(np.float64) - ref64[i]).max())
            if bars[k] is None:
                assert d <= 1e-8, (name, tag, k, d)   # flat and returned as (all but) 0
            else:
                assert d <= bars[k], "%s %s %s: reference float32 %.3e from its float64, bar %.3e" % (name, tag, k, d, bars[k])


@pytest.mark.parametrize("name", [c.name for c in wc.CASES if c.kind != "nan"])
def test_bar_is_at_most_1e_3(name):
    """condition 2: on every map that is not flat"""
    for all_bands, tag in FORMS:
        for k, b in wc.bars(wc.BY_NAME[name], all_bands).items():
            assert b is None or 4 * wc.U <= b <= 1e-3, (name, tag, k, b)


@pytest.mark.parametrize("name", ["odd_5x7", "even_odd_6x9", "row_1x9", "odd_37x53"])
def test_restatement_bands(name):
    pred, gt = (t.double() for t in wc.inputs(name))
    want = tlr.haar_bands_2level((pred - gt)[None])
    got = wef.residual_bands(pred, gt)
    for k in want:
        assert got[k].shape == want[k].shape[1:]
        assert float((got[k] - want[k][0]).abs().max()) <= 1e-15, k


def test_heatmap_against_the_fixture(fx):
    x = torch.from_numpy(fx["heat_in"])
    assert np.array_equal(wef.make_heatmap_rgb(x).numpy(), fx["heat_out"])
    assert wef.make_heatmap_rgb(torch.rand(2, 1, 3, 5)).shape == (2, 3, 3, 5)


def ramp_maps(n, H, W):
    return {"K%d" % i: torch.full((1, 1, H, W), i / max(n - 1, 1)) for i in range(n)}


@pytest.mark.parametrize("n,cols", [(4, 1), (4, 3), (9, 3), (9, 4), (2, 5)])
def test_grid_layout(n, cols):
    H, W = 3, 5
    maps = ramp_maps(n, H, W)
    grid = wef.make_wef_grid_image(maps, list(maps), tile_cols=cols)
    rows = (n + cols - 1) // cols
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == (rows * H, cols * W, 3)
    for idx in range(rows * cols):
        tile = grid[(idx // cols) * H:(idx // cols + 1) * H, (idx % cols) * W:(idx % cols + 1) * W]
        if idx >= n:
            assert int(tile.max()) == 0
            continue
        x = np.float32(idx / max(n - 1, 1))
        want = [np.uint8(x * np.float32(255)),
                np.uint8(np.clip(np.float32(1) - np.abs(x - np.float32(0.5)) * np.float32(2), 0, 1) * np.float32(255)),
                np.uint8((np.float32(1) - x) * np.float32(255))]
        assert tile.reshape(-1, 3).unique(dim=0).tolist() == [[int(v) for v in want]], idx


@pytest.mark.parametrize("name", [c.name for c in wc.FIXTURE_CASES if c.kind != "nan"])
def test_grid_bytes_against_the_fixture(fx, rest32, name):
    """Equal bytes, except where the reference's value sits within the bar of a truncation step (the two float32 results are
    each within the bar of float64, so 2 bars apart at most; the green channel has slope 2).  Measured share of bytes that
    differ (level 2 / all bands, either tile_cols): even_odd_6x9 0.46 % / 0, every other case 0 / 0; the cap is 35 %."""
    c = wc.BY_NAME[name]
    for all_bands, tag in FORMS:
        keys = wc.keys_of(all_bands)
        ref32 = fx["maps32_%s_%s" % (name, tag)]
        skip, bars = noisy_keys(c, all_bands, ref32), wc.bars(c, all_bands)
        for cols, key in ((3, "grid_%s_%s" % (name, tag)),) + (((4, "grid4_%s_all" % name),) if all_bands else ()):
            got = wef.make_wef_grid_image(rest32[name][all_bands], list(keys), tile_cols=cols).numpy()
            want = fx[key]
            assert got.shape == want.shape and got.dtype == want.dtype
            near, total = 0, 0
            for i, k in enumerate(keys):
                r, cc = i // cols, i % cols
                sl = (slice(r * c.H, (r + 1) * c.H), slice(cc * c.W, (cc + 1) * c.W))
                if k in skip:
                    continue
                diff = got[sl].astype(np.int32) - want[sl].astype(np.int32)
                total += diff.size
                if not diff.any():
                    continue
                x = np.clip(ref32[i].astype(np.float64), 0, 1)
                h = np.stack([x, np.clip(1 - np.abs(x - 0.5) * 2, 0, 1), 1 - x], axis=-1) * 255
                step = np.abs(h - np.round(h))
                allow = 255 * 2 * 2 * (bars[k] or 0.0)
                bad = (diff != 0) & ((np.abs(diff) > 1) | (step > allow))
                assert not bad.any(), "%s %s cols %d %s: %d bytes differ away from a truncation step" % (name, tag, cols, k, bad.sum())
                near += int((diff != 0).sum())
            for idx in range(len(keys), want.shape[0] // c.H * cols):
                r, cc = idx // cols, idx % cols
                assert not got[r * c.H:(r + 1) * c.H, cc * c.W:(cc + 1) * c.W].any()
            share = near / max(total, 1)
            print("%s %s cols %d: %.2f %% of the bytes sit on a truncation step" % (name, tag, cols, 100 * share))
            assert share <= 0.35


def test_titled_grid():
    H, W = 40, 150
    maps = {k: torch.rand((1, 1, H, W), generator=torch.Generator().manual_seed(i)) for i, k in enumerate(wc.LEVEL2_KEYS)}
    keys = list(wc.LEVEL2_KEYS)
    plain = wef.make_wef_grid_image(maps, keys, tile_cols=3).numpy()
    titled = wef.make_wef_grid_image_titled(maps, keys, tile_cols=3).numpy()
    assert plain.shape == titled.shape == (2 * H, 3 * W, 3)
    inside = np.zeros(plain.shape[:2], dtype=bool)
    labels = []
    for idx in range(len(keys)):
        r, c = idx // 3, idx % 3
        inside[r * H:r * H + 27, c * W:c * W + 121] = True
        labels.append(titled[r * H:r * H + 27, c * W:c * W + 121])
    assert np.array_equal(plain[~inside], titled[~inside])
    assert set(np.unique(titled[inside]).tolist()) == {0, 255}
    for a in range(len(labels)):
        assert labels[a].any() and (labels[a][..., 0] == labels[a][..., 1]).all()
        for b in range(a + 1, len(labels)):
            assert not np.array_equal(labels[a], labels[b]), (keys[a], keys[b])
    # the longest key fits its box with a margin, an unknown character is a filled box, a label is cut at the box
    m = wef.label_mask("COMBINED")
    assert m.shape == (27, 121) and m[:, -6:].sum() == 0 and m[:6].sum() == 0 and m[:, :6].sum() == 0 and m.any()
    assert wef.label_mask("a")[6:20, 6:16].all()
    assert wef.label_mask("W" * 40).shape == (27, 121)


def test_titled_grid_clipped_on_a_small_tile():
    """5 x 7 tiles: every box reaches over its neighbours and is clipped at the image border; they are drawn in key order"""
    c = wc.BY_NAME["odd_5x7"]
    pred, gt = wc.inputs(c)
    maps = wef.compute_wef_maps(pred, gt)
    keys = list(wc.LEVEL2_KEYS)
    titled = wef.make_wef_grid_image_titled(maps, keys, tile_cols=3).numpy()
    assert titled.shape == (2 * c.H, 3 * c.W, 3)
    want = np.zeros((2 * c.H, 3 * c.W), dtype=np.uint8)
    for idx, k in enumerate(keys):
        r, cc = idx // 3, idx % 3
        box = want[r * c.H:r * c.H + 27, cc * c.W:cc * c.W + 121]
        box[...] = wef.label_mask(k)[:box.shape[0], :box.shape[1]] * 255
    assert all(np.array_equal(titled[..., ch], want) for ch in range(3))   # (the boxes cover the whole 10 x 21 image)


def test_as_pil():
    maps = ramp_maps(2, 3, 4)
    try:
        import PIL  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            wef.make_wef_grid_image(maps, list(maps), as_pil=True)
        return
    im = wef.make_wef_grid_image(maps, list(maps), tile_cols=2, as_pil=True)
    assert im.size == (8, 3) and im.mode == "RGB"
    assert np.array_equal(np.array(im), wef.make_wef_grid_image(maps, list(maps), tile_cols=2).numpy())


def test_charbonnier_against_the_fixture(fx):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_golden_wef import CH_SHAPES, charbonnier_inputs
    for i in range(len(CH_SHAPES)):
        for eps_tag, eps in (("d", None), ("e", 0.05)):
            for dt_tag, dt in (("32", torch.float32), ("64", torch.float64)):
                pred, target = (t.to(dt).requires_grad_(True) for t in charbonnier_inputs(i))
                loss = wef.charbonnier_loss(pred, target) if eps is None else wef.charbonnier_loss(pred, target, eps)
                loss.backward()
                pre = "ch_%d_%s_%s_" % (i, eps_tag, dt_tag)
                assert np.array_equal(loss.detach().numpy(), fx[pre + "loss"]), pre
                assert np.array_equal(pred.grad.numpy(), fx[pre + "dpred"]) and np.array_equal(target.grad.numpy(), fx[pre + "dtarget"])


def test_error_paths():
    a = torch.rand(3, 6, 9)
    with pytest.raises(ValueError, match="one image per call"):
        wef.compute_wef_maps(torch.rand(2, 3, 6, 9), torch.rand(2, 3, 6, 9))
    with pytest.raises(ValueError, match="same shape"):
        wef.compute_wef_all_subbands(a, torch.rand(3, 6, 8))
    with pytest.raises(ValueError, match="1 to 4 channels"):
        wef.compute_wef_maps(torch.rand(5, 6, 9), torch.rand(5, 6, 9))
    with pytest.raises(ValueError):
        wef.compute_wef_maps(torch.rand(6, 9), torch.rand(6, 9))
    with pytest.raises(ValueError, match="float32 or float64"):
        wef.compute_wef_maps(a.half(), a.half())
    with pytest.raises(ValueError, match="device or dtype"):
        wef.compute_wef_maps(a, a.double())
    with pytest.raises(ValueError, match="No images for grid"):
        wef.make_wef_grid_image({}, [])
    with pytest.raises(ValueError, match="tile_cols"):
        wef.make_wef_grid_image(ramp_maps(2, 3, 4), ["K0"], tile_cols=0)
    with pytest.raises(ValueError, match="share a shape"):
        wef.make_wef_grid_image({"a": torch.rand(1, 1, 3, 4), "b": torch.rand(1, 1, 3, 5)}, ["a", "b"])
    with pytest.raises(ValueError, match="same shape"):
        wef.charbonnier_loss(torch.rand(3), torch.rand(4))
    with pytest.raises(ValueError, match="at least one element"):
        wef.charbonnier_loss(torch.rand(0), torch.rand(0))
    # no gradient flows through the maps
    p = a.clone().requires_grad_(True)
    assert not any(v.requires_grad for v in wef.compute_wef_maps(p, torch.rand(3, 6, 9)).values())


def test_abi_is_declared_and_bound():
    from gsplat_amd import capi
    header = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", header)
    for n in ("wef_tmp_bytes", "wef_maps", "wef_grid", "charbonnier_tmp_bytes", "charbonnier_fwd", "charbonnier_bwd"):
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
        decl = re.search(r"\bgs_%s\(([^;]*)\);" % n, header)
        assert decl and len(decl.group(1).split(",")) == len(capi.PROTOTYPES[n][1]), n
    assert (wef.LABEL_W, wef.LABEL_H) == tuple(int(re.search(r"#define\s+GS_WEF_LABEL_%s\s+(\d+)" % a, header).group(1)) for a in "WH")
    assert "gs_wef.o" in open(os.path.join(ROOT, "sparse-view-3dgs-pack_amd", "csrc", "Makefile")).read()
