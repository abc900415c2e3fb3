"""The constructed blend scenes (tests/blend_cases.py) on the host: the construction is what it claims to be, clears its
margin condition in the float64 model, and the oracle agrees with that model - with EXACT n_contrib / last contributors -
before any GPU is involved.  Bars: tests/test_oracle_dense.py's (2e-5 absolute on the image, 2e-4 of each gradient
tensor's largest entry)."""
import pytest
import torch

import blend_cases
from helpers import run_scene
from test_gpu_raster_parity import forward_state, last_contributor_id

CPU = torch.device("cpu")
IMG_BAR, GRAD_BAR = 2e-5, 2e-4


@pytest.mark.parametrize("name", blend_cases.NAMES)
def test_margin_condition(name):
    """A condition on the scene, not a tolerance: no skip / stop / clamp decision of any (pixel, entry) pair lies within
    MARGIN of its threshold in float64, so no fp32 implementation may take it the other way."""
    case = blend_cases.build(name)
    out, _ = blend_cases.dense(case)
    m = blend_cases.margins(out["detail"])
    print(name, {k: "%.3g" % v for k, v in m.items()})
    for k, v in m.items():
        assert v > 1.0, "%s: %s margin is %.3g of the required one" % (name, k, v)


def test_margin_condition_bites():
    """Moving one tuned blob by a fraction of a pixel puts a pixel on the alpha = 1/255 contour, and it is the margin
    assertion (not a tolerance) that fails.  A blob of variance 1.3 and opacity 0.05 has that contour at d^2 = 2.6 ln(12.75) =
    6.6196; centred on the quarter-pixel lattice at (2.5, 3.5) pixel (0, 3) lies at d^2 = 6.5, clear of it by 4.6 % of
    alpha; 0.0238 pixels further right the same pixel lies on it."""
    import math
    d0sq = 2.0 * blend_cases.VAR_BLOB * math.log(255.0 * 0.05)
    for x, ok in ((2.5, True), (math.sqrt(d0sq - 0.25), False)):
        b = blend_cases.Builder(16, 16)
        b.add(x, 3.5, blend_cases.VAR_BLOB, 0.05)
        m = blend_cases.margins(_dense(b.case("blob_at_%.4f" % x))["detail"])
        assert abs(x - 2.5) < 0.03 and (m["alpha"] > 1.0) == ok, (x, m)


def _dense(case):
    import dense_reference
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.scene.items()}
    return dense_reference.render(d, case.cam, case.bg, False, detail=True)


@pytest.mark.parametrize("name", blend_cases.NAMES)
def test_construction(oracle, name):
    """the lists are the intended ones (lengths against the oracle's ranges and the float64 model's rectangles) and the
    events each case is named after happen where the case says"""
    case = blend_cases.build(name)
    out, _ = blend_cases.dense(case)
    o = forward_state(oracle.backend, case.scene, case.cam, CPU, case.bg, False)
    rng = o["ranges"].reshape(-1, 2).long()
    assert torch.equal(rng[:, 1] - rng[:, 0], torch.tensor(case.tile_len)), (rng[:, 1] - rng[:, 0], case.tile_len)
    # power <= 0 in fp32: the conic the kernels are handed (bit-equal between oracle and HIP, tests/test_gpu_blend_cases.py) is
    # positive definite, and for the axis-aligned footprints its cross term is too small by six orders of magnitude to
    # turn the sign of qa dx^2 + qb dx dy + qc dy^2 through rounding - also on the pixel an opacity-1 Gaussian is centred on
    co = o["conic_opacity"][o["radii"] > 0].double()
    a, b, c = co[:, 0], co[:, 1], co[:, 2]
    assert bool((a > 0).all()) and bool((c > 0).all()) and bool((b * b < a * c).all())
    if case.scene_sr is not None:
        assert bool((b * b < 1e-6 * a * c).all()), float((b * b / (a * c)).max())
    W, H = case.W, case.H
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tile = (ys // 16) * ((W + 15) // 16) + xs // 16
    assert torch.equal(out["detail"]["tile_len"], torch.tensor(case.tile_len)[tile])
    n, T, meta = out["n_contrib"], out["final_T"], case.meta
    stopped = out["detail"]["tested"] & (out["detail"]["test_T"] < 1e-4)        # [N, G]: the pixel's stop entry
    stop_at = (stopped.to(torch.int64) * torch.arange(1, stopped.shape[1] + 1)[None]).sum(1).reshape(H, W)   # (at most one per pixel)
    if meta["group"] in ("length", "partial") and "n" in meta:
        assert int(stop_at.max()) == 0 and int(n.min()) == int(n.max()) == meta["n"]
    if "stop" in meta:
        for t, k in meta["stop"].items():
            assert int(stop_at[tile == t].min()) > 0 and int(stop_at[tile == t].max()) == k, (t, stop_at[tile == t].max())
            assert int(n[tile == t].max()) == k - 1
        assert int(case.tile_len.min()) >= max(meta["stop"].values()) + 130
    if "outside_alive" in meta:   # the columns outside the image would see (almost) nothing of what stops the inside ones
        x0, x1 = meta["outside_alive"]
        k = meta["stop"][0]
        col = out["detail"]["raw"][:, k - 1].reshape(H, W)[0]
        var = 8.0
        import math
        assert all(0.97 * math.exp(-(x - 2) ** 2 / (2 * var)) < 0.5 / 255.0 for x in range(x0, x1)) and float(col[8]) > 0.1
    if "last_pixel" in meta:
        x, y = meta["last_pixel"]
        others = stop_at.clone()
        others[y, x] = 0
        assert int(stop_at[y, x]) == meta["stop"][0] and int(others.max()) <= 34 and int(stop_at.min()) > 0
    if name == "quad_early_sat":
        assert 0 < int(stop_at[:8, :8].min()) and int(stop_at[:8, :8].max()) <= 64
        for q in (1, 2, 3):
            assert int(n[(q >> 1) * 8:(q >> 1) * 8 + 8, (q & 1) * 8:(q & 1) * 8 + 8].max()) == 200
    if "only" in meta:
        q = meta["only"]
        inq = ((xs // 8) == (q & 1)) & ((ys // 8) == (q >> 1))
        assert int(n[~inq].max()) == 0 and float((T[~inq] - 1).abs().max()) == 0 and int(n[inq].max()) == 100
    if name == "quad_four_batches":
        lane = [int(n[3 + (q >> 1) * 8, 3 + (q & 1) * 8]) for q in range(4)]
        assert [(v - 1) // 64 for v in lane] == [0, 1, 2, 3], lane
    if "clamp" in meta:
        pos, x, y = meta["clamp"]
        raw = out["detail"]["raw"]
        assert float(raw[y * W + x, pos - 1]) > 0.999 and int((raw >= 0.99).sum()) == 1
    if "skipped" in meta:
        assert not set(meta["skipped"]) & set(n.reshape(-1).tolist()), "an entry that reaches no pixel is a last contributor"
        assert int(n.max()) < case.tile_len[0] or name == "alpha_low_opacity"
    if "corner_pixel" in meta:
        x, y = meta["corner_pixel"]
        col = out["detail"]["raw"][:, meta["ellipse"] - 1].reshape(H, W)
        reached = col[:16, :16] >= 1.0 / 255.0
        assert int(reached.sum()) == 1 and bool(reached[y, x])
    if "run" in meta:
        z = o["depths"]
        start = 30 if meta["run"] > 3 else 10
        assert int((z.view(torch.int32) == z.view(torch.int32)[start]).sum()) == meta["run"]
        assert torch.equal(o["point_list"].long()[start:start + meta["run"]], torch.arange(start, start + meta["run"]))


# Oracle against float64, measured (largest over all cases, the 1 025-entry list included; each case prints its own):
# colour 2.7e-6, inverse depth 8.6e-7, final_T 8.5e-7; gradients, of the tensor's largest entry: means3D 1.3e-5, scales 5.1e-6,
# every other tensor below 3e-6.  test_oracle_dense.py's bars hold everywhere with a factor 7 to spare, so none is widened.
# (alpha_diagonal_corner has the one footprint that scales + identity rotation cannot describe: no scene_sr for it)
@pytest.mark.parametrize("name,which", [(n, w) for n in blend_cases.NAMES for w in ("scene", "scene_sr")
                                        if not (w == "scene_sr" and n in blend_cases.NO_SCALES_ROTATIONS)])
def test_oracle_matches_dense_float64(oracle, name, which):
    case = blend_cases.build(name)
    sc = getattr(case, which)
    assert sc is not None
    dn, dg = blend_cases.dense(case, which)
    W, H = case.W, case.H
    o = forward_state(oracle.backend, sc, case.cam, CPU, case.bg, False)
    assert torch.equal(o["radii"].long(), dn["radii"].long()), "radii differ"
    assert torch.equal(o["n_contrib"].reshape(H, W).long(), dn["n_contrib"]), "n_contrib differs"
    assert torch.equal(last_contributor_id(o, W, H), dn["last_id"]), "last contributor differs"
    errs = dict(color=float((o["color"].double() - dn["color"]).abs().max()),
                invdepth=float((o["invdepth"].double() - dn["invdepth"]).abs().max()) / max(1.0, float(dn["invdepth"].abs().max())),
                final_T=float((o["final_T"].reshape(H, W).double() - dn["final_T"]).abs().max()))
    dc, di = blend_cases.cotangents(case)
    r = run_scene(oracle.Rasterizer, oracle.Settings, sc, case.cam, CPU, bg=case.bg, dL_dcolor=dc, dL_dinvdepth=di)
    for k in ("means3D", "opacities", "colors_precomp", "scales", "rotations", "cov3D_precomp"):
        if k in r["grads"]:
            errs["d" + k] = float((r["grads"][k].double() - dg[k]).abs().max()) / max(float(dg[k].abs().max()), 1e-12)
    errs["dmeans2D"] = float((r["grads"]["means2D"][:, :2].double() - dg["ndc_probe"]).abs().max()) / \
        max(float(dg["ndc_probe"].abs().max()), 1e-12)
    print(name, which, {k: "%.1e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v < (IMG_BAR if k in ("color", "invdepth", "final_T") else GRAD_BAR), "%s %s: %s err %.3e" % (name, which, k, v)
