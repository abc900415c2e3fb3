"""gsplat_amd/depth_priors.py on the host: depth_scales against the twins of tests/depth_prior_reference.py over the case table
of tests/depth_prior_cases.py (each case's claim is proved first), make_depth_params / read_depth_params on a COLMAP model
written to disk, prepare_invdepth against its float32 and float64 twins at the bars the case table derives, and
Trainer.load_depth_priors from files.  cv2 is not involved anywhere: DESIGN.md 4.8.4 says what that leaves unverified."""
import json
import math
import os

import numpy as np
import pytest
import torch

import depth_prior_cases as dc
import depth_prior_reference as ref
from gsplat_amd import depth_priors as dp
from gsplat_amd import imageio
from gsplat_amd import io as gio

SCALE_CASES = {c.name: c for c in dc.scale_cases()}
PREPARE_CASES = {c.name: c for c in dc.prepare_cases()}
STATS = ("scale", "offset", "n_valid", "t_colmap", "s_colmap", "t_mono", "s_mono")


def twins(case, wide=False, coord_bits=5):
    table = dp.dense_point_table(case.xyz, case.ids)
    out = {}
    for image in case.images.values():
        key = dp.image_key(image.name)
        if case.maps.get(key) is not None:
            out[key] = ref.scales_twin(image, case.cams[image.camera_id], table, case.maps[key], coord_bits, wide)
    return out


def same_bits(a, b):
    a, b = np.float64(a), np.float64(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.int64) == b.view(np.int64) or (a == 0 and b == 0)


@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_each_case_is_what_it_claims(name):
    case = SCALE_CASES[name]
    tw = twins(case)
    assert sorted(tw) == sorted(case.expect)
    table = dp.dense_point_table(case.xyz, case.ids)
    for key, exp in case.expect.items():
        t = tw[key]
        assert t["n_valid"] == exp["n_valid"], (key, t["n_valid"])
        if "zero" in exp:
            assert (t["scale"] == 0 and t["offset"] == 0) == exp["zero"], (key, t)
        image = next(i for i in case.images.values() if dp.image_key(i.name) == key)
        ids = np.asarray(image.point3D_ids)
        if exp.get("ties"):
            used = (ids >= 0) & (ids < len(table))
            inv = np.sort(1.0 / table[ids[used]][:, 2])
            field = case.maps[key].astype(np.float32) / np.float32(65536)
            mono = np.sort(ref.sample_twin(field, image.xys[:, 0].astype(np.float32), image.xys[:, 1].astype(np.float32)))
            n = len(inv)
            for seq in (inv, mono):
                assert seq[(n - 1) // 2 - 1] == seq[(n - 1) // 2] == seq[n // 2] == seq[n // 2 + 1], (key, seq)
        if exp.get("absent_used"):
            assert 7 not in case.ids and (ids == 7).sum() == 1 and not table[7].any() and len(table) > 7
            assert (ids == -1).sum() == 2 and (ids >= len(table)).sum() == 2
            assert t["n_valid"] == (ids >= 0).sum() - 2     # every in-range id counts, the absent one too
        if exp.get("valid_range_below_gate"):
            z = table[ids][:, 2]
            inv_valid = 1.0 / z[z > 0]
            assert inv_valid.max() - inv_valid.min() <= 1e-3 < t["range"] and (z < 0).sum() == 2
        if exp.get("range_nan"):
            assert math.isnan(t["range"]) and t["n_valid"] > 10
        if exp.get("nonfinite"):
            assert math.isinf(t["s_colmap"]) and math.isinf(t["scale"]) and not math.isfinite(t["offset"])
        if "range_is" in exp:
            assert t["range"] == exp["range_is"] and t["n_valid"] > 10
        if "range_above" in exp:
            assert exp["range_above"] < t["range"] <= math.nextafter(math.nextafter(exp["range_above"], 1.0), 1.0)
        if exp.get("replicated"):
            field = case.maps[key].astype(np.float32) / np.float32(65536)
            got = ref.sample_twin(field, np.array([63.5, 63.99], np.float32), np.array([10.0, 47.99], np.float32))
            assert got[0] == field[10, 63] and got[1] == field[47, 63]
    if name == "edge_excluded_s05":
        m = case.maps[name]
        assert m.shape[0] / dc.HEIGHT == 0.5 and np.float32(64.0 * 0.5) == np.float32(dc.WIDTH * 0.5)
    if name == "several":
        assert sorted(case.maps[k].shape for k in ("a", "b", "c")) == [(12, 16), (24, 32), (48, 64)]
        assert case.maps["nomap"] is None and len(case.images[4].point3D_ids) == 0


@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_host_path_equals_the_twin_bit_for_bit(name):
    case = SCALE_CASES[name]
    got = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, return_stats=True)
    tw = twins(case)
    assert list(got) == [dp.image_key(i.name) for i in case.images.values() if case.maps.get(dp.image_key(i.name)) is not None]
    for key in tw:
        for k in STATS:
            assert same_bits(got[key][k], tw[key][k]), (key, k, got[key][k], tw[key][k])
    plain = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps)
    assert all(sorted(v) == ["offset", "scale"] for v in plain.values())
    assert all(same_bits(plain[k]["scale"], got[k]["scale"]) for k in plain)


def test_unquantised_coordinates_are_a_keyword():
    case = SCALE_CASES["n257"]
    got = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, coord_bits=None, return_stats=True)
    tw, tw5 = twins(case, coord_bits=None), twins(case)
    for k in STATS:
        assert same_bits(got["n257"][k], tw["n257"][k]), k
    assert tw["n257"]["t_mono"] != tw5["n257"]["t_mono"] or tw["n257"]["s_mono"] != tw5["n257"]["s_mono"]


def test_float32_mean_against_the_float64_form_is_within_the_any_order_bound():
    """numpy's float32 mean of the mono deviations (the host path) against their exact sum: the distance between the host
    path's s_mono and the device's.  Held to n v; the measured distances are printed (and recorded by the GPU test)."""
    worst = 0.0
    for name, case in SCALE_CASES.items():
        narrow, wide = twins(case), twins(case, wide=True)
        for key in narrow:
            a, b, n = narrow[key]["s_mono"], wide[key]["s_mono"], narrow[key]["n_valid"]
            if b == 0 or not math.isfinite(b):
                continue
            rel = abs(a - b) / b
            worst = max(worst, rel)
            assert rel <= (n + 1) * dc.V, (name, key, rel)
            if math.isfinite(wide[key]["s_colmap"]):      # (z_zero_one's is infinite in both)
                assert abs(narrow[key]["s_colmap"] - wide[key]["s_colmap"]) <= dc.DEV_REL(n) * wide[key]["s_colmap"]
            else:
                assert narrow[key]["s_colmap"] == wide[key]["s_colmap"]
    print("float32 mean vs float64 form, worst relative distance: %.3e" % worst)
    assert worst > 0      # the two are different computations


# ------------------------------------------------------------------------------------------------ files
def write_text_model(dirpath, cams, images, xyz, ids):
    os.makedirs(dirpath, exist_ok=True)
    with open(os.path.join(dirpath, "cameras.txt"), "w") as f:
        f.write("# cameras\n")
        for c in cams.values():
            f.write("%d %s %d %d %s\n" % (c.id, c.model, c.width, c.height, " ".join(repr(float(p)) for p in c.params)))
    with open(os.path.join(dirpath, "images.txt"), "w") as f:
        f.write("# images\n")
        for im in images.values():
            f.write("%d %s %s %d %s\n" % (im.id, " ".join(repr(float(v)) for v in im.qvec), " ".join(repr(float(v)) for v in im.tvec),
                                           im.camera_id, im.name))
            f.write(" ".join("%r %r %d" % (float(x), float(y), int(p)) for (x, y), p in zip(im.xys, im.point3D_ids)) + "\n")
    with open(os.path.join(dirpath, "points3D.txt"), "w") as f:
        f.write("# points\n")
        for p, i in zip(xyz, ids):
            f.write("%d %r %r %r 10 20 30 0.5\n" % (int(i), float(p[0]), float(p[1]), float(p[2])))


def test_make_depth_params_from_a_colmap_model_on_disk(tmp_path):
    case = SCALE_CASES["several"]
    base, depths = str(tmp_path / "scene"), str(tmp_path / "scene" / "depths")
    sparse = os.path.join(base, "sparse", "0")
    n = len(case.ids)
    assert np.array_equal(case.ids, np.arange(1, n + 1))      # write_colmap_binary numbers the points 1..N
    gio.write_colmap_binary(sparse, case.cams, case.images, (case.xyz, np.zeros((n, 3)), np.zeros((n, 1))))
    write_text_model(sparse, case.cams, case.images, case.xyz, case.ids)
    os.makedirs(depths)
    for key, m in case.maps.items():
        if m is not None:
            imageio.write_png16(os.path.join(depths, key + ".png"), m)
    want = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps)
    got_bin = dp.make_depth_params(base, depths, "bin")
    path = os.path.join(sparse, "depth_params.json")
    text_bin = open(path).read()
    got_txt = dp.make_depth_params(base, depths, "txt")
    assert list(got_bin) == ["a", "b", "c", "empty"] and "nomap" not in got_bin      # the image without a file is left out
    assert got_bin == want and got_txt == got_bin and got_bin["empty"] == {"scale": 0, "offset": 0}
    assert got_bin["a"]["scale"] > 0
    assert open(path).read() == text_bin == json.dumps(got_bin, indent=2)
    back = dp.read_depth_params(path)
    med = float(np.median([v["scale"] for v in got_bin.values() if v["scale"] > 0]))
    assert all(back[k]["scale"] == got_bin[k]["scale"] and back[k]["offset"] == got_bin[k]["offset"] and back[k]["med_scale"] == med
               for k in got_bin)
    xyz, rgb, err, ids = gio.read_points3D_binary(os.path.join(sparse, "points3D.bin"), with_ids=True)
    assert np.array_equal(ids, case.ids) and ids.dtype == np.int64 and len(gio.read_points3D_binary(os.path.join(sparse, "points3D.bin"))) == 3
    xyz_t, _, _, ids_t = gio.read_points3D_text(os.path.join(sparse, "points3D.txt"), with_ids=True)
    assert np.array_equal(ids_t, case.ids) and np.array_equal(xyz_t, xyz) and len(gio.read_points3D_text(os.path.join(sparse, "points3D.txt"))) == 3
    with pytest.raises(ValueError, match="model_type"):
        dp.make_depth_params(base, depths, "ply")
    imageio.write_png16(os.path.join(depths, "a.png"), np.zeros((48, 64, 3), dtype=np.uint16))
    with pytest.raises(ValueError, match="channels"):
        dp.make_depth_params(base, depths, "bin")


@pytest.mark.parametrize("scales,want", [((0.0, 0, -1.0), 0), ((0.0, 2.5, -3.0), 2.5), ((4.0, 0, 1.0, 2.0, 8.0), 3.0)])
def test_med_scale_with_none_one_and_an_even_number_of_positive_scales(tmp_path, scales, want):
    path = str(tmp_path / "depth_params.json")
    with open(path, "w") as f:
        json.dump({"k%d" % i: {"scale": s, "offset": 0.5} for i, s in enumerate(scales)}, f, indent=2)
    back = dp.read_depth_params(path)
    assert [back["k%d" % i]["med_scale"] for i in range(len(scales))] == [want] * len(scales)
    assert [back["k%d" % i]["scale"] for i in range(len(scales))] == list(scales)


# ------------------------------------------------------------------------------------------------ the camera's map
@pytest.mark.parametrize("name", sorted(PREPARE_CASES))
def test_prepare_invdepth_on_the_host(name):
    c = PREPARE_CASES[name]
    inv, mask, reliable = dp.prepare_invdepth(c.src, c.size, c.entry, c.divisor)
    W2, H2 = c.size
    assert inv.dtype == torch.float32 and tuple(inv.shape) == (1, H2, W2) == tuple(mask.shape) and not inv.is_cuda
    t32, m32, r32 = ref.prepare_twin(c.src, c.size, c.entry, c.divisor)
    t64, m64, r64 = ref.prepare_twin64(c.src, c.size, c.entry, c.divisor)
    assert reliable is c.reliable and r32 is c.reliable and r64 is c.reliable
    assert np.array_equal(mask.numpy(), m32) and float(mask.min()) == float(mask.max()) == (1.0 if reliable else 0.0)
    assert np.array_equal(inv.numpy().view(np.int32), t32.view(np.int32)), "the host path is the float32 twin, bit for bit"
    err = float(np.abs(inv.numpy().astype(np.float64) - t64).max())
    bar = 0.0 if c.exact else dc.prepare_bar(c.src, c.divisor, c.entry)
    print("%s: max |host - float64 twin| = %.3e (bar %.3e)" % (name, err, bar))
    assert err <= bar
    assert float(inv.min()) >= 0 or (c.entry is not None and c.entry["scale"] > 0)
    if name == "same_size":
        assert np.array_equal(inv.numpy()[0], c.src.astype(np.float32) / np.float32(65536))
    if name == "negative_source":
        assert (c.src < 0).any() and float(inv.min()) == 0.0
    if name.startswith("scale_"):       # scale <= 0: the map stays unscaled
        plain, _, _ = dp.prepare_invdepth(c.src, c.size, None, c.divisor)
        assert torch.equal(inv, plain)
    # a float32 source holding the same samples gives the same bits
    if c.src.dtype == np.uint16:
        inv_f, _, _ = dp.prepare_invdepth(c.src.astype(np.float32), c.size, c.entry, c.divisor)
        assert torch.equal(inv, inv_f)


def test_scale_and_offset_round_twice_never_fused():
    src, entry, two, one = dc.fma_case(np.random.default_rng(5))
    assert two != one, "the builder found a sample where fma(x, s, o) is not the two roundings"
    inv, _, _ = dp.prepare_invdepth(src, (4, 4), entry)
    assert float(inv[0, 0, 0]) == two


def test_trainer_loads_priors_from_files_with_the_same_loss_bits(oracle, tmp_path):
    from test_trainer_cpu import make_trainer
    a, b = make_trainer(oracle, P=300, W=96, H=64), make_trainer(oracle, P=300, W=96, H=64)
    rng = np.random.default_rng(9)
    keys = ["v0", "v1", "v2", "v3"]
    params = {"v0": dict(scale=1.5, offset=0.01, med_scale=1.5), "v1": dict(scale=9.0, offset=0.0, med_scale=1.5),
              "v3": dict(scale=0.0, offset=0.0, med_scale=1.5)}       # v1: unreliable; v2: no file; v3: scale 0 < 0.2 med: unreliable
    maps = {k: rng.integers(0, 30000, size=(32, 48)).astype(np.uint16) for k in ("v0", "v1", "v3")}
    for k, m in maps.items():
        imageio.write_png16(str(tmp_path / (k + ".png")), m)
    got = a.load_depth_priors(keys, str(tmp_path), params)
    assert got is a.depth_priors and [p is None for p in got] == [False, True, True, True]
    assert got[0][1] is None and tuple(got[0][0].shape) == (1, 64, 96)
    inv, mask, reliable = dp.prepare_invdepth(maps["v0"], (96, 64), params["v0"])
    assert reliable and bool((mask == 1).all())
    b.depth_priors = [(inv, None), None, None, None]
    a.optimizer_step = b.optimizer_step = False
    a.depth_l1_weight = b.depth_l1_weight = 0.37
    for ci in (0, 1):
        la, lb = a._step_camera(ci, False, ()), b._step_camera(ci, False, ())
        assert float(la) == float(lb) and torch.equal(a.model.flat_grad, b.model.flat_grad)
        assert ("depth_l1" in a.last["parts"]) == (ci == 0)       # the term ran for the camera with a reliable file only
    # without depth_params every file is reliable and unscaled; nerf_synthetic divides by 512
    plain = dp.load_depth_priors(keys, str(tmp_path), None, [(48, 32)] * 4, nerf_synthetic=True)
    assert [p is None for p in plain] == [False, False, True, False]
    assert np.array_equal(plain[0][0].numpy()[0], maps["v0"].astype(np.float32) / np.float32(512))
