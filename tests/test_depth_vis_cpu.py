"""The coloured depth map (gsplat_amd/depth_vis.py, csrc/gs_depth_vis.hip), the parts that need no GPU: the numpy restatement
against tests/golden/depth_vis.npz - what the reference's own visualize_cmap / vis_depth gave (tests/golden/make_golden_paths.py)
- with lo and hi equal as float64 bits and every byte equal; the cases' named properties; the colour table and the two byte
rules; the "dng" allowance measured and the fixtures held to its condition; the ABI's new names."""
import os
import re

import numpy as np
import pytest
import torch

import depth_vis_cases as dc
from gsplat_amd import depth_vis as dv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_vis.npz")
CASES = dc.cases()
PAIRS = [(name, rule) for name, (_, _, rules) in CASES.items() for rule in rules]


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def coloured_image(z, name):
    return z[name + "_composite"] if name + "_composite" in z.files else z[name + "_depth"]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64).tolist()


def test_fixture_holds_the_seeded_cases_and_arrays_only(z):
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    for name, (depth, alpha, rules) in CASES.items():
        assert z[name + "_depth"].dtype == np.float32 and np.array_equal(z[name + "_depth"].view(np.uint32), depth.view(np.uint32)), name
        assert (alpha is None) == (name + "_alpha" not in z.files)
        if alpha is not None:
            assert np.array_equal(z[name + "_alpha"], alpha)
        for rule in rules:
            key = "%s_%s" % (name, rule)
            assert z[key + "_bounds"].dtype == np.float64 and z[key + "_rgb"].dtype == np.uint8
            assert z[key + "_rgb"].shape == depth.shape + (3,)
    for k in z.files:
        assert z[k].dtype.kind in "fu", k   # numbers only
    for H, W in ((1, 1), (1, 199), (1, 200), (1, 201), (13, 17), (257, 3), (64, 48), (160, 128)):
        assert "size_%dx%d" % (H, W) in CASES
    for name in ("size_1x1_alpha", "const", "const_alpha", "two_values", "shared_bits", "shared_top24", "mixed_signs", "one_inf", "few_nan",
                 "alpha_0_1", "plain_alpha_64x48"):
        assert name in CASES, name


@pytest.mark.parametrize("name,rule", PAIRS)
def test_numpy_restatement_equals_the_reference(z, name, rule):
    depth, alpha, _ = CASES[name]
    rgb, lo, hi = dv.colour_depth_numpy(depth, alpha, rule)
    key = "%s_%s" % (name, rule)
    assert bits([lo, hi]) == bits(z[key + "_bounds"])
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, z[key + "_rgb"])
    if key + "_v" in z.files:
        v, _, _ = dv.normalise_numpy(coloured_image(z, name), rule)
        assert np.array_equal(v, z[key + "_v"])
    # the public entry on CPU tensors is the same restatement
    out, b = dv.colour_depth(torch.from_numpy(depth)[None], None if alpha is None else torch.from_numpy(alpha), rule, return_bounds=True)
    assert out.dtype == torch.uint8 and out.device.type == "cpu" and np.array_equal(out.numpy(), rgb)
    assert bits(b.numpy()) == bits([lo, hi]) or (np.isnan(lo) and bool(torch.isnan(b).all()))


def test_composite_on_cpu_is_render_py_121_and_124(z):
    from gsplat_amd.imageio import save_image_bytes
    for name in ("plain_alpha_64x48", "alpha_0_1"):
        depth, alpha, _ = CASES[name]
        d, a = torch.from_numpy(depth), torch.from_numpy(alpha)
        comp, grey = dv.composite_depth(d, a)
        want = (d - d.min()) / (d.max() - d.min()) + 1 * (1 - a)
        assert torch.equal(comp, want) and np.array_equal(comp.numpy(), z[name + "_composite"])
        assert torch.equal(grey, save_image_bytes(1 - want))


# ------------------------------------------------------------------------------------------------- named properties
def queries(n):
    return np.array([0.5, 99.5]) * (np.float32(n) / 100)


def test_query_positions_of_the_size_cases():
    assert queries(199)[0] < 1.0                        # left of the first node: the smallest value itself
    assert queries(200)[0] == 1.0                       # exactly node 1
    assert 1.0 < queries(201)[0] < 2.0                  # between nodes 1 and 2
    assert queries(1)[0] < 1.0 and queries(1)[1] < 1.0  # one node: both queries left of it
    assert queries(200)[1] == 199.0                     # 1 x 200: the high query sits on a node too
    for n in (199, 201, 221, 771, 3072, 20480):
        q = queries(n)[1]
        assert 1.0 < q < n and q != np.floor(q)         # elsewhere the high query interpolates
    x = np.sort(CASES["size_1x199"][0].reshape(-1))
    assert dv.percentile_bounds_numpy(CASES["size_1x199"][0], 0.0)[0] == np.float64(x[0])
    x = np.sort(CASES["size_1x200"][0].reshape(-1))
    assert dv.percentile_bounds_numpy(CASES["size_1x200"][0], 0.0)[0] == np.float64(x[0])


def wanted_ranks(n):
    out = []
    for q in queries(n):
        j = max(int(np.floor(q)) - 1, 0)
        out += [j, min(j + 1, n - 1)]
    return out


def test_value_cases_have_the_property_they_are_named_for(z):
    two = np.sort(CASES["two_values"][0].reshape(-1))
    r = wanted_ranks(two.size)
    assert two[r[0]] == two[r[1]] == np.float32(1.25) and two[r[2]] == two[r[3]] == np.float32(3.5)   # each tie spans a query's ranks
    assert len(np.unique(two)) == 2
    for name, side in (("shared_bits", 1), ("shared_top24", 0)):
        x = CASES[name][0].reshape(-1)
        keys = dc.key_bits(x)
        bulk = keys[(x >= 2.0) & (x < 2.5)]
        assert bulk.size >= 0.97 * x.size
        assert len(np.unique(bulk >> 21)) == 1                                   # top 11 bits agree
        order = np.argsort(keys, kind="stable")
        r = wanted_ranks(x.size)
        inside = keys[order][r[2 * side:2 * side + 2]]                           # this query's ranks lie in the shared prefix
        assert all(k >> 21 == bulk[0] >> 21 for k in inside)
        if name == "shared_top24":
            assert len(np.unique(bulk >> 8)) == 1 and all(k >> 8 == bulk[0] >> 8 for k in inside)   # top 24 (so top 22 too)
        else:
            assert (np.unique(bulk >> 10, return_counts=True)[1].max() >= x.size // 2 - 20)        # half agree in their top 22
            assert len(np.unique(bulk >> 10)) > 1
    m = CASES["mixed_signs"][0].reshape(-1)
    assert (m < 0).any() and (m > 0).any() and (np.signbit(m) & (m == 0)).sum() > 0 and (~np.signbit(m) & (m == 0)).sum() > 0
    k = dc.key_bits(m)
    assert np.array_equal(np.sort(m), m[np.argsort(k, kind="stable")])           # the key order is the value order, -0 = +0
    assert np.isinf(CASES["one_inf"][0]).sum() == 1 and np.isnan(CASES["few_nan"][0]).sum() == 3
    nan = CASES["few_nan"][0].reshape(-1)
    assert np.isnan(nan[np.argsort(dc.key_bits(nan))][-3:]).all()               # NaN last, as np.argsort places it
    a = CASES["alpha_0_1"][1]
    assert (a == 0).sum() >= 96 and (a == 1).sum() >= 384 and ((a > 0) & (a < 1)).any()
    # the constant image under the composite: 0 / 0, an all-NaN image and bounds, the whole picture table row 0
    for name in ("const_alpha", "size_1x1_alpha"):
        assert np.isnan(z[name + "_composite"]).all()
        for rule in dc.RULES:
            assert np.isnan(z["%s_%s_bounds" % (name, rule)]).all()
            rgb = z["%s_%s_rgb" % (name, rule)]
            assert (rgb == dv.byte_tables()["trunc" if rule == "fsgs" else "save_image"][0]).all()


# ------------------------------------------------------------------------------------------------- tables
def test_turbo_table_is_matplotlibs(z):
    t = dv.turbo_table()
    assert t.dtype == np.float64 and t.shape == (256, 3)
    assert np.array_equal(t, z["turbo"])    # what the generator's matplotlib held
    matplotlib = pytest.importorskip("matplotlib")
    assert np.array_equal(t, matplotlib.colormaps["turbo"](np.arange(256))[:, :3])


def test_byte_tables_follow_their_rules():
    t = torch.from_numpy(dv.turbo_table())
    tabs = dv.byte_tables()
    assert np.array_equal(tabs["save_image"], t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy())   # save_image on float64
    bgr = np.uint8(dv.turbo_table()[..., ::-1] * 255)                                                       # vis_depth's return
    assert np.array_equal(tabs["trunc"], bgr[..., ::-1])   # R, G, B: what cv2.imwrite stores on disk for that array
    assert tabs["save_image"].dtype == tabs["trunc"].dtype == np.uint8
    assert (tabs["save_image"] != tabs["trunc"]).any()


# ------------------------------------------------------------------------------------------------- the dng allowance
def test_log_allowance_is_the_measured_one_and_the_fixtures_meet_its_condition(z):
    worst = 0.0
    for name, (_, _, rules) in CASES.items():
        if "dng" not in rules:
            continue
        x = coloured_image(z, name)
        u = dc.log_ulp_error(x)
        worst = max(worst, float(u.max()) if u.size else 0.0)
        lo, hi = z[name + "_dng_bounds"]
        frac = float(dc.dng_exempt(x, z[name + "_dng_v"], lo, hi).mean())
        assert frac <= dc.MAX_EXEMPT_FRACTION, (name, frac)
    assert worst <= dc.LOG_ULP_MEASURED, worst
    assert dc.LOG_ULP_ALLOW == 2 * dc.LOG_ULP_MEASURED


def test_committed_parity_record_covers_the_dng_cases():
    """profiles/depth_vis_parity.json is one GPU run of tests/test_gpu_depth_vis.py with DEPTH_VIS_PARITY_OUT set; a normal run
    does not rewrite it, so it is held here to the case list and to the allowance the tests use."""
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "depth_vis_parity.json")))
    assert rec["log_ulp_measured_cpu"] == dc.LOG_ULP_MEASURED and rec["log_ulp_allowance"] == dc.LOG_ULP_ALLOW
    assert rec["max_exempt_fraction"] == dc.MAX_EXEMPT_FRACTION
    assert set(rec["dng_pixels_differing_on_gpu"]) == {n for n, (_, _, rules) in CASES.items() if "dng" in rules}
    for name, count in rec["dng_pixels_differing_on_gpu"].items():
        assert 0 <= count <= dc.MAX_EXEMPT_FRACTION * CASES[name][0].size, (name, count)


# ------------------------------------------------------------------------------------------------- ABI
def test_abi_names_and_argument_counts():
    from gsplat_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsplat.h")).read(), flags=re.S)
    for n in ("depth_vis_tmp_bytes", "depth_vis"):
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
        m = re.search(r"\bgs_%s\s*\(([^)]*)\)" % n, hdr)
        assert m and len(capi.PROTOTYPES[n][1]) == len([a for a in m.group(1).split(",") if a.strip()]), n
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", hdr), "additive entries: the ABI version stays"
    for rule, code in dv.RULES.items():
        assert re.search(r"#define\s+GS_DEPTH_VIS_%s\s+%d\b" % (rule.upper(), code), hdr)


def test_colour_depth_refuses_what_it_does_not_restates():
    with pytest.raises(ValueError):
        dv.colour_depth(torch.zeros((4, 4)), rule="jet")
    with pytest.raises(ValueError):
        dv.colour_depth(torch.zeros((2, 4, 4)))
    with pytest.raises(ValueError):
        dv.colour_depth(torch.zeros((4, 4)), alpha=torch.zeros((4, 5)))
    out = dv.colour_depth(torch.zeros((0, 5)))
    assert out.shape == (0, 5, 3) and out.dtype == torch.uint8
