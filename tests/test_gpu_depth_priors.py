"""gs_depth_scales and gs_invdepth_prepare (csrc/gs_depth_priors.hip) on the GPU over the case table of
tests/depth_prior_cases.py, against the twins of tests/depth_prior_reference.py at the bars that table derives.

  gs_depth_scales      n_valid and both medians: the twin's bits.  Both deviations, scale and offset: within DEV_REL / SCALE_REL /
                       offset_bar of the twin's float64 form.  The gate's zero answers, and the non-finite ones of z = +0: equal.
  gs_invdepth_prepare  the host path's bits on every case (the same IEEE operations in the same order), hence exact where the
                       case is exact and within prepare_bar of the float64 twin elsewhere, no pixel exempt; the mask plane exact.
The measured distances go to the file DEPTH_PRIORS_PARITY_OUT names, when it is set (profiles/depth_priors_parity.json is one
such run)."""
import ctypes as C
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

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SCALE_CASES = {c.name: c for c in dc.scale_cases()}
PREPARE_CASES = {c.name: c for c in dc.prepare_cases()}
MEASURED = {"depth_scales": {}, "prepare_invdepth": {}}


@pytest.fixture(scope="module")
def twins():
    """per case: {key: (the twin in the script's dtypes, its float64 form)}, computed once"""
    out = {}
    for name, case in SCALE_CASES.items():
        table = dp.dense_point_table(case.xyz, case.ids)
        out[name] = {}
        for image in case.images.values():
            key = dp.image_key(image.name)
            if case.maps.get(key) is not None:
                cam = case.cams[image.camera_id]
                out[name][key] = (ref.scales_twin(image, cam, table, case.maps[key]),
                                  ref.scales_twin(image, cam, table, case.maps[key], wide=True))
    return out


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    out = os.environ.get("DEPTH_PRIORS_PARITY_OUT")
    if out and (MEASURED["depth_scales"] or MEASURED["prepare_invdepth"]):
        json.dump(MEASURED, open(out, "w"), indent=1)


def bits(x):
    return np.float64(x).view(np.int64)


def check_against_twins(name, got, tw):
    assert list(got) == list(tw)
    for key, (narrow, wide) in tw.items():
        g, n = got[key], narrow["n_valid"]
        assert g["n_valid"] == n, (key, g["n_valid"], n)
        if narrow["scale"] == 0 and narrow["offset"] == 0:     # the gate failed: exact zeros, the script's integers
            assert g["scale"] == 0 and g["offset"] == 0 and isinstance(g["scale"], int), (key, g)
            continue
        assert bits(g["t_colmap"]) == bits(narrow["t_colmap"]) and bits(g["t_mono"]) == bits(narrow["t_mono"]), (key, g, narrow)
        rec = {}
        for k in ("s_colmap", "s_mono", "scale", "offset"):
            if not math.isfinite(wide[k]):
                assert (math.isnan(g[k]) and math.isnan(wide[k])) or g[k] == wide[k], (key, k, g[k], wide[k])
                continue
            bar = {"s_colmap": dc.DEV_REL(n) * abs(wide[k]), "s_mono": dc.DEV_REL(n) * abs(wide[k]),
                   "scale": dc.SCALE_REL(n) * abs(wide[k]),
                   "offset": dc.offset_bar(n, wide["t_mono"], wide["scale"], wide["offset"])}[k]
            err = abs(g[k] - wide[k])
            rec[k] = dict(err=err, bar=bar, host_err=abs(narrow[k] - wide[k]))
            print("%s/%s %s: |device - float64 form| = %.3e (bar %.3e), host path %.3e" % (name, key, k, err, bar, rec[k]["host_err"]))
            assert err <= bar, (key, k, g[k], wide[k], err, bar)
        MEASURED["depth_scales"]["%s/%s" % (name, key)] = rec


@pytest.mark.parametrize("name", sorted(SCALE_CASES))
def test_depth_scales_on_the_device(hip, twins, name):
    case = SCALE_CASES[name]
    got = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, on_device=True, return_stats=True)
    check_against_twins(name, got, twins[name])
    again = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, on_device=True, return_stats=True)
    assert all(bits(got[k][s]) == bits(again[k][s]) for k in got for s in dp.STAT_KEYS)       # the same bits on every run


def test_float32_maps_and_unquantised_coordinates(hip, twins):
    case = SCALE_CASES["several"]
    as_f32 = {k: None if m is None else m.astype(np.float32) for k, m in case.maps.items()}
    a = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, on_device=True, return_stats=True)
    b = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, as_f32, on_device=True, return_stats=True)
    assert all(bits(a[k][s]) == bits(b[k][s]) for k in a for s in dp.STAT_KEYS)
    case = SCALE_CASES["n257"]
    table = dp.dense_point_table(case.xyz, case.ids)
    image = case.images[1]
    tw = {"n257": (ref.scales_twin(image, case.cams[1], table, case.maps["n257"], None),
                   ref.scales_twin(image, case.cams[1], table, case.maps["n257"], None, wide=True))}
    got = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, on_device=True, coord_bits=None, return_stats=True)
    check_against_twins("n257_unquantised", got, tw)
    assert bits(got["n257"]["t_mono"]) != bits(twins["n257"]["n257"][0]["t_mono"]) or \
        got["n257"]["s_mono"] != twins["n257"]["n257"][1]["s_mono"]


def raw_scales(api, t, n_table, n_obs, dtype, n_images, tmp, nb, out, coord_bits=5):
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return api.raw("depth_scales")(p(t["table"]), n_table, p(t["ids"]), p(t["xys"]), n_obs, p(t["seg"]), p(t["cams"]), p(t["ptrs"]),
                                   p(t["hw"]), dtype, coord_bits, n_images, p(tmp), nb, p(out), stream)


def test_exact_scratch_behind_guard_words_and_every_bad_argument_status(hip):
    api = hip.api
    case = SCALE_CASES["several"]
    table = dp.dense_point_table(case.xyz, case.ids)
    items = [(i, case.cams[i.camera_id], case.maps[dp.image_key(i.name)]) for i in case.images.values()
             if case.maps[dp.image_key(i.name)] is not None]
    t, n_obs, dtype = dp.pack_device_inputs(items, table, DEV)
    n = len(items)
    nb = int(api.raw("depth_scales_tmp_bytes")(n_obs))
    assert nb >= 16 * n_obs and nb % 256 == 0 and api.raw("depth_scales_tmp_bytes")(-1) == 0
    buf = torch.full((nb + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    tmp = buf[256:256 + nb]
    guard = torch.full((n + 2, 8), -7.0, dtype=torch.float64, device=DEV)
    out = guard[1:n + 1]
    runs = []
    for _ in range(2):      # the second call meets what the first left in the scratch
        assert raw_scales(api, t, len(table), n_obs, dtype, n, tmp, nb, out) == 0
        runs.append(out.clone())
    torch.cuda.synchronize()
    assert bool((buf[:256] == 0xA5).all()) and bool((buf[256 + nb:] == 0xA5).all()), "a write outside the scratch"
    assert bool((guard[0] == -7.0).all()) and bool((guard[n + 1] == -7.0).all()), "a write outside the output rows"
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))
    want = dp.depth_scales(case.images, case.cams, case.xyz, case.ids, case.maps, on_device=True)
    assert [float(v) for v in runs[0][:, 0].cpu()] == [float(w["scale"]) for w in want.values()]
    assert raw_scales(api, t, len(table), n_obs, dtype, n, tmp, nb - 1, out) == -2          # one byte short
    assert raw_scales(api, t, len(table), n_obs, dtype, n, tmp[1:], nb, out) == -2          # not 256-byte aligned
    assert raw_scales(api, t, len(table), n_obs, 2, n, tmp, nb, out) == -2                  # unknown dtype
    assert raw_scales(api, t, len(table), n_obs, dtype, n, tmp, nb, out, coord_bits=11) == -2
    assert raw_scales(api, t, len(table), n_obs, dtype, -1, tmp, nb, out) == -2
    assert raw_scales(api, t, len(table), n_obs, dtype, 0, None, 0, None) == 0              # no image: nothing to do
    assert raw_scales(api, t, len(table), n_obs, dtype, n, None, nb, out) == -1             # GS_E_NULL
    assert raw_scales(api, t, len(table), n_obs, dtype, n, tmp, nb, None) == -1
    assert raw_scales(api, dict(t, seg=None), len(table), n_obs, dtype, n, tmp, nb, out) == -1
    src = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    dst = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda *a: api.raw("invdepth_prepare")(*a, stream)  # noqa: E731
    assert call(src.data_ptr(), 1, 4, 4, 4, 4, 65536.0, 0, 1.0, 0.0, 1.0, dst.data_ptr(), None) == 0
    assert call(src.data_ptr(), 1, 0, 4, 4, 4, 65536.0, 0, 1.0, 0.0, 1.0, dst.data_ptr(), None) == -2
    assert call(src.data_ptr(), 1, 4, 4, 4, 32769, 65536.0, 0, 1.0, 0.0, 1.0, dst.data_ptr(), None) == -2
    assert call(src.data_ptr(), 3, 4, 4, 4, 4, 65536.0, 0, 1.0, 0.0, 1.0, dst.data_ptr(), None) == -2
    assert call(None, 1, 4, 4, 4, 4, 65536.0, 0, 1.0, 0.0, 1.0, dst.data_ptr(), None) == -1
    assert call(src.data_ptr(), 1, 4, 4, 4, 4, 65536.0, 0, 1.0, 0.0, 1.0, None, None) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", sorted(PREPARE_CASES))
def test_invdepth_prepare_on_the_device(hip, name):
    c = PREPARE_CASES[name]
    W2, H2 = c.size
    inv, mask, reliable = dp.prepare_invdepth(c.src, c.size, c.entry, c.divisor, device=DEV)
    assert inv.is_cuda and mask.is_cuda and tuple(inv.shape) == (1, H2, W2) == tuple(mask.shape) and reliable is c.reliable
    host, host_mask, _ = dp.prepare_invdepth(c.src, c.size, c.entry, c.divisor)
    t64, m64, _ = ref.prepare_twin64(c.src, c.size, c.entry, c.divisor)
    got = inv.cpu().numpy()
    assert np.array_equal(mask.cpu().numpy(), m64) and torch.equal(mask.cpu(), host_mask)          # the mask plane is exact
    err = float(np.abs(got.astype(np.float64) - t64).max())
    bar = 0.0 if c.exact else dc.prepare_bar(c.src, c.divisor, c.entry)
    differ = int((got.view(np.int32) != host.numpy().view(np.int32)).sum())
    print("%s: max |device - float64 twin| = %.3e (bar %.3e); %d pixels differ from the host path" % (name, err, bar, differ))
    MEASURED["prepare_invdepth"][name] = dict(err=err, bar=bar, pixels_differing_from_host=differ)
    assert err <= bar                                   # every pixel
    assert differ == 0, "the device is the host path's operations in the host path's order"
    if c.src.dtype == np.uint16:                        # a float32 source holding the same samples: the same bits
        inv_f, _, _ = dp.prepare_invdepth(torch.from_numpy(c.src.astype(np.float32)).to(DEV), c.size, c.entry, c.divisor)
        assert torch.equal(inv_f, inv)
    if name == "no_fma":
        _, _, two, one = dc.fma_case(np.random.default_rng(5))
        assert two != one and float(got[0, 0, 0]) == two


def test_a_full_size_map_halved(hip):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 65536, size=(1200, 1600)).astype(np.uint16)
    inv, mask, _ = dp.prepare_invdepth(src, (800, 600), None, device=DEV)
    S = src.astype(np.float64) / 65536
    want = (S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2]) / 4        # exact: sums of 16-bit samples
    assert np.array_equal(inv.cpu().numpy()[0].astype(np.float64), want) and bool((mask == 1).all())
    same, _, _ = dp.prepare_invdepth(src, (1600, 1200), None, device=DEV)
    assert np.array_equal(same.cpu().numpy()[0], src.astype(np.float32) / np.float32(65536))


def test_load_depth_priors_on_the_device_equals_the_host_path(hip, tmp_path):
    rng = np.random.default_rng(9)
    keys = ["v0", "v1", "v2", "v3"]
    params = {"v0": dict(scale=1.5, offset=0.01, med_scale=1.5), "v1": dict(scale=9.0, offset=0.0, med_scale=1.5),
              "v3": dict(scale=0.4, offset=0.2, med_scale=1.5)}
    maps = {k: rng.integers(0, 30000, size=(32, 48)).astype(np.uint16) for k in ("v0", "v1", "v3")}
    for k, m in maps.items():
        imageio.write_png16(str(tmp_path / (k + ".png")), m)
    sizes = [(64, 48), (64, 48), (64, 48), (48, 32)]
    on_dev = dp.load_depth_priors(keys, str(tmp_path), params, sizes, device=DEV)
    on_cpu = dp.load_depth_priors(keys, str(tmp_path), params, sizes)
    assert [p is None for p in on_dev] == [p is None for p in on_cpu] == [False, True, True, False]
    for k, d, h in zip(keys, on_dev, on_cpu):
        if d is None:
            continue
        assert d[0].is_cuda and d[1] is None and h[1] is None and d[0].shape == h[0].shape
        err = float((d[0].cpu().double() - h[0].double()).abs().max())
        bar = dc.prepare_bar(maps[k], 65536.0, params[k])
        assert err <= bar, (k, err, bar)
        assert torch.equal(d[0].cpu(), h[0])        # (in fact the same bits: the same operations in the same order)
