"""Evaluation from files (gsplat_amd/imageio.py, gsplat_amd/render_set.py, csrc/gs_eval_files.hip), the parts that need no GPU:
the resize tables and the numpy resize against Pillow's recorded bytes (tests/golden/pil_resize.npz), the PNG reader against
Pillow-decoded golden files and the writer against the reader (and against Pillow where it imports), the SSIM_sk restatement
against the scipy chain where scipy imports, and the ABI's new names."""
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import eval_files_reference as fref
from gsplat_amd import imageio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
PNG = os.path.join(ROOT, "tests", "golden", "png")
CASES = fref.fixture_cases()
NAMES = ("resize_tmp_bytes", "resize_bicubic_u8", "eval_ssim_sk_tmp_bytes", "eval_ssim_sk")


def expected(z, key, a):
    """Pillow's bytes of a case; the same-size case stores none: Pillow returned a copy of the (CRC-checked) input"""
    return z[key + "_out"] if key + "_out" in z.files else a


def test_fixture_holds_every_case_of_the_list():
    z = np.load(GOLDEN)
    sizes = {(hw, hw2) for _, _, hw, hw2, _ in CASES}
    for pair in (((8, 8), (2, 2)), ((5, 4), (1, 1)), ((13, 29), (3, 7)), ((37, 64), (9, 16)), ((75, 101), (18, 25)),
                 ((300, 400), (75, 100)), ((300, 400), (77, 133)), ((300, 400), (300, 400))):
        assert pair in sizes, pair
    assert any(hw[0] == hw2[0] and hw[1] != hw2[1] for hw, hw2 in sizes) and any(hw[1] == hw2[1] and hw[0] != hw2[0] for hw, hw2 in sizes)
    for key, _, _, _, _ in CASES:
        assert key + "_crc" in z.files, key
    for kind in fref.CONTENTS:
        assert any(k.startswith(kind) for k, *_ in CASES)
    assert os.path.getsize(GOLDEN) < 128 * 1024   # (Pillow's bytes for the random cases the size list names are 73 KB that do not compress)


@pytest.mark.parametrize("n_in,n_out", sorted({(hw[i], hw2[i]) for _, _, hw, hw2, _ in CASES for i in (0, 1)}))
def test_tables_equal_the_fixtures(n_in, n_out):
    z = np.load(GOLDEN)
    b, c = imageio.resize_tables(n_in, n_out)
    assert b.dtype == np.int32 and c.dtype == np.int32
    assert np.array_equal(b, z["tab_%d_%d_b" % (n_in, n_out)]) and np.array_equal(c, z["tab_%d_%d_c" % (n_in, n_out)])
    # the runs stay inside the source axis and inside the table row; every row sums to 2^22 within its roundings
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= c.shape[1]).all()
    assert (np.abs(c.sum(axis=1) - (1 << 22)) <= c.shape[1]).all()
    assert imageio.resize_tables(n_in, n_out)[1] is c, "the tables are cached per (in, out)"


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_numpy_resize_equals_pillows_recorded_bytes(key):
    z = np.load(GOLDEN)
    _, make, (H, W), (H2, W2), C = next(c for c in CASES if c[0] == key)
    a = make()
    assert fref.crc(a) == int(z[key + "_crc"]), "the seeded input is not the generator's"
    want = expected(z, key, a)
    got = imageio.resize_u8_numpy(a, (W2, H2))
    assert got.dtype == np.uint8 and got.shape == (H2, W2, C) and np.array_equal(got, want)
    # the public entry, on a CPU tensor: the same bytes, and the planar fp32 image is bytes / 255 in fp32
    t, planar = imageio.resize_u8(torch.from_numpy(a), (W2, H2), return_planar=True)
    assert torch.equal(t, torch.from_numpy(np.ascontiguousarray(want)))
    assert torch.equal(planar, torch.from_numpy(np.ascontiguousarray(want)).permute(2, 0, 1).to(torch.float32).div(255))
    if C == 1:
        assert np.array_equal(imageio.resize_u8(a[:, :, 0], (W2, H2)), want[:, :, 0])


def test_content_cases_reach_the_clamp():
    """The fixture's content cases exercise the clamp on both sides: the unclamped accumulator of the horizontal pass leaves
    [0, 255] both ways on the mask-like image's sharp edges at a quarter scale and on the period-3 checkerboard when it is
    upscaled.  (Downscaled to a quarter, the checkerboards average out and stay inside: measured 80 .. 175.)"""
    def unclamped(img, n_out):
        b, c = imageio.resize_tables(img.shape[1], n_out)
        return [((1 << 21) + int((c[o, :b[o, 1]].astype(np.int64) * img[y, b[o, 0]:b[o, 0] + b[o, 1]]).sum())) >> 22
                for y in range(img.shape[0]) for o in range(n_out)]
    for kind, (H, W), W2 in (("masklike", (300, 400), 100), ("checker3", (12, 10), 27)):
        acc = unclamped(fref.content_u8(kind, H, W, 1)[:, :, 0].astype(np.int64), W2)
        print("unclamped range of %s's horizontal pass: %d .. %d" % (kind, min(acc), max(acc)))
        assert min(acc) < 0 and max(acc) > 255, kind


def test_numpy_resize_equals_pillow_on_fresh_sizes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2024)
    sizes = [((int(rng.integers(9, 90)), int(rng.integers(9, 90))), (int(rng.integers(1, 40)), int(rng.integers(1, 40)))) for _ in range(6)]
    sizes += [((41, 57), (41, 14)), ((41, 57), (10, 57)), ((12, 10), (30, 27))]   # one axis only (both ways), and an upscale
    for (H, W), (H2, W2) in sizes:
        for C in (1, 3):
            a = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
            want = np.asarray(Image.fromarray(a[:, :, 0] if C == 1 else a).resize((W2, H2))).reshape(H2, W2, C)
            assert np.array_equal(imageio.resize_u8_numpy(a, (W2, H2)), want), ((H, W), (H2, W2), C)


def test_resize_refusals():
    with pytest.raises(ValueError, match="uint8"):
        imageio.resize_u8(torch.zeros(4, 4, 3), (2, 2))
    with pytest.raises(ValueError, match="premultiplies"):
        imageio.resize_u8(torch.zeros(4, 4, 4, dtype=torch.uint8), (2, 2))
    with pytest.raises(ValueError):
        imageio.resize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), (0, 2))


# ------------------------------------------------------------------------------------------------------------ PNG
def golden_pngs():
    z = np.load(os.path.join(PNG, "decoded.npz"))
    return z, sorted(z.files)


@pytest.mark.parametrize("name", golden_pngs()[1])
def test_read_png_decodes_the_golden_files(name):
    z, _ = golden_pngs()
    got = imageio.read_png(os.path.join(PNG, name))
    assert got.dtype == np.uint8 and got.shape == z[name].shape and np.array_equal(got, z[name])


def test_golden_files_cover_colour_types_and_filter_types():
    _, names = golden_pngs()
    for mode in ("L", "LA", "RGB", "RGBA"):
        assert "pil_%s.png" % mode in names
        for ft in range(5):
            name = "f%d_%s.png" % (ft, mode)
            assert name in names
            raw = open(os.path.join(PNG, name), "rb").read()
            n = struct.unpack(">I", raw[33:37])[0]
            assert raw[37:41] == b"IDAT"
            rows = zlib.decompress(raw[41:41 + n])
            C = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}[mode]
            assert set(rows[::1 + 14 * C]) == {ft}, "every row of %s carries filter type %d" % (name, ft)
    assert all(os.path.getsize(os.path.join(PNG, f)) < 4096 for f in names)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 17), (17, 1), (33, 40)])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_write_then_read_round_trips(tmp_path, H, W, C):
    a = np.random.default_rng(H * 100 + W + C).integers(0, 256, size=(H, W, C), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    imageio.write_png(path, torch.from_numpy(a))
    got = imageio.read_png(path)
    assert got.shape == (H, W, C) and np.array_equal(got, a)
    if C == 1:
        imageio.write_png(path, a[:, :, 0])
        assert np.array_equal(imageio.read_png(path), a)
    try:
        from PIL import Image
    except ImportError:
        return
    pil = np.asarray(Image.open(path))
    assert np.array_equal(pil.reshape(H, W, C), a), "Pillow decodes our file to other bytes"


def test_read_png_refusals(tmp_path):
    with pytest.raises(ValueError, match="8-bit files only"):
        imageio.read_png(os.path.join(PNG, "refuse_16bit.png"))
    with pytest.raises(ValueError, match="palette"):
        imageio.read_png(os.path.join(PNG, "refuse_palette.png"))
    # an interlaced file: our own bytes with the header's interlace method set (and its checksum redone)
    data = bytearray(imageio.png_bytes(np.zeros((4, 4, 3), dtype=np.uint8)))
    data[28] = 1
    data[29:33] = struct.pack(">I", zlib.crc32(bytes(data[12:29])) & 0xFFFFFFFF)
    p = tmp_path / "interlaced.png"
    p.write_bytes(bytes(data))
    with pytest.raises(ValueError, match="interlaced"):
        imageio.read_png(str(p))
    (tmp_path / "not.png").write_bytes(b"hello")
    with pytest.raises(ValueError, match="not a PNG"):
        imageio.read_png(str(tmp_path / "not.png"))
    with pytest.raises(ValueError, match="uint8"):
        imageio.write_png(str(tmp_path / "f.png"), np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        imageio.write_png(str(tmp_path / "f.png"), np.zeros((4, 4, 5), dtype=np.uint8))


def test_save_image_bytes_on_the_host():
    import eval_reference as ref
    x = ref.seeded_pair(3, 9, 11, seed=1, spread=0.3)[0]
    assert torch.equal(imageio.save_image_bytes(x), ref.to_bytes(x).permute(1, 2, 0))
    grey = imageio.save_image_bytes(x[:1])
    assert tuple(grey.shape) == (9, 11, 3) and torch.equal(grey[:, :, 0], grey[:, :, 2])
    assert torch.equal(grey[:, :, 0], ref.to_bytes(x[0]))
    assert torch.equal(imageio.save_image_bytes(x[0]), grey)


def test_write_render_set_folders_and_depth_images(tmp_path):
    """render.py's folders from host tensors (the byte rule needs no device): names, the two grey depth images of
    DNGaussian/render.py:121,124-125, and no depth folder for views without depth and alpha."""
    import eval_reference as ref
    from gsplat_amd import render_set
    g = torch.Generator().manual_seed(3)
    views = []
    for i in range(2):
        render, gt = ref.seeded_pair(3, 10, 12, seed=20 + i, spread=0.2)
        views.append({"render": render, "gt": torch.cat([gt, torch.ones(1, 10, 12)]),   # (a 4th channel the files drop)
                      "depth": 2 + 3 * torch.rand((1, 10, 12), generator=g), "alpha": torch.rand((1, 10, 12), generator=g)})
    base = render_set.write_render_set(str(tmp_path), "test", 30000, views)
    assert base == os.path.join(str(tmp_path), "test", "ours_30000")
    assert sorted(os.listdir(base)) == ["depth", "gt", "renders"]
    assert sorted(os.listdir(os.path.join(base, "depth"))) == ["00000.png", "00001.png", "alpha_00000.png", "alpha_00001.png"]
    for i, v in enumerate(views):
        name = "%05d.png" % i
        assert np.array_equal(imageio.read_png(os.path.join(base, "renders", name)), ref.to_bytes(v["render"]).permute(1, 2, 0).numpy())
        assert np.array_equal(imageio.read_png(os.path.join(base, "gt", name)), ref.to_bytes(v["gt"][:3]).permute(1, 2, 0).numpy())
        d, a = v["depth"], v["alpha"]
        depth = (d - d.min()) / (d.max() - d.min()) + 1 * (1 - a)
        want = ref.to_bytes(1 - depth).expand(3, -1, -1).permute(1, 2, 0).numpy()   # save_image writes a grey image as three channels
        assert np.array_equal(imageio.read_png(os.path.join(base, "depth", name)), want)
        assert np.array_equal(imageio.read_png(os.path.join(base, "depth", "alpha_" + name)),
                              ref.to_bytes(a).expand(3, -1, -1).permute(1, 2, 0).numpy())
    plain = render_set.write_render_set(str(tmp_path / "b"), "train", 1, [{"render": views[0]["render"], "gt": views[0]["gt"]}])
    assert sorted(os.listdir(plain)) == ["gt", "renders"]
    with pytest.raises(ValueError, match="no `render`"):
        render_set.write_render_set(str(tmp_path / "c"), "test", 1, [{"gt": views[0]["gt"]}])


# -------------------------------------------------------------------------------------------------------- SSIM_sk
def pair(C, H, W, seed):
    rng = np.random.default_rng(seed)
    gt = rng.random((C, H, W), dtype=np.float32)
    render = np.clip(gt + 0.1 * rng.standard_normal((C, H, W)).astype(np.float32), 0, 1).astype(np.float32)
    return render, gt


@pytest.mark.parametrize("C,H,W", [(1, 7, 7), (3, 7, 8), (3, 9, 9), (3, 33, 40), (4, 38, 39)])
def test_direct_float64_form_equals_the_scipy_chain(C, H, W):
    pytest.importorskip("scipy.ndimage")
    a, b = pair(C, H, W, seed=H * W + C)
    direct, chain = fref.ssim_sk_f64(a, b), fref.ssim_sk_scipy(a, b, np.float64)
    print("direct %.17g scipy float64 chain %.17g" % (direct, chain))
    assert abs(direct - chain) <= 1e-14
    # the float32 restatement is scipy's float32 chain to float32 rounding of the means, and lies where the issue says
    f32, chain32 = fref.ssim_sk_f32(a, b), fref.ssim_sk_scipy(a, b, np.float32)
    print("float32 restated %.17g scipy float32 chain %.17g |f32 - f64| %.3g" % (f32, chain32, abs(f32 - direct)))
    assert abs(f32 - chain32) <= 1e-6 and abs(f32 - direct) <= 1e-6


def test_ssim_sk_restatement_properties():
    a, b = pair(3, 33, 40, seed=3)
    assert abs(fref.ssim_sk_f64(a, a) - 1.0) <= 1e-12 and abs(fref.ssim_sk_f32(a, a) - 1.0) <= 1e-6
    assert 0.0 < fref.ssim_sk_f64(a, b) < 1.0
    # a 7 x 7 image is one window
    x, y = pair(1, 7, 7, seed=4)
    x64, y64 = x[0].astype(np.float64), y[0].astype(np.float64)
    ux, uy = x64.mean(), y64.mean()
    vx, vy, vxy = x64.var(ddof=1), y64.var(ddof=1), ((x64 - ux) * (y64 - uy)).sum() / 48
    want = (2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    assert abs(fref.ssim_sk_f64(x, y) - want) <= 1e-12
    with pytest.raises(ValueError):
        fref.ssim_sk_f64(np.zeros((3, 6, 40), np.float32), np.zeros((3, 6, 40), np.float32))
    with pytest.raises(ValueError):
        fref.ssim_sk_f32(np.zeros((3, 40, 6), np.float32), np.zeros((3, 40, 6), np.float32))
    flat = np.full((3, 9, 9), 0.25, np.float32)
    assert fref.ssim_sk_f64(flat, flat) == 1.0


def test_committed_parity_record_covers_the_gpu_tests_cases():
    """profiles/eval_files_parity.json is one GPU run of tests/test_gpu_image_files.py with GS_EVAL_FILES_PARITY_OUT set.  It
    is not rewritten by a normal run, so it is held here to the GPU tests' case list, to their bar, and to the two figures
    DESIGN.md section 4.8.1 and gsplat_amd/evaluate.py quote from it."""
    import json
    rec = json.load(open(os.path.join(ROOT, "profiles", "eval_files_parity.json")))
    keys = {fref.sk_case_key(C, H, W, form) for H, W in fref.SK_SIZES for C in fref.SK_CHANNELS for form in fref.SK_FLAGS}
    assert keys <= set(rec), sorted(keys - set(rec))[:5]
    assert set(rec) - keys <= {"flat_0.25_vs_0.75"}, sorted(set(rec) - keys)[:5]
    for k, v in rec.items():
        assert v["abs_err"] <= max(v["bar_f32_vs_f64"], fref.SK_FLOOR), (k, v)
    assert max(v["abs_err"] for v in rec.values()) <= 1.6e-15, "the documents say: observed at most 1.6e-15"
    bars = [rec[k]["bar_f32_vs_f64"] for k in keys]
    assert 2e-10 <= min(bars) and max(bars) <= 8e-7, "the documents say: the float32 chain lies 2e-10 to 8e-7 from float64"
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "observed at most 1.6e-15" in text and "2e-10 to 8e-7" in text


# ------------------------------------------------------------------------------------------------------------ ABI
def test_abi_names_in_prototypes_device_only_and_header():
    from gsplat_amd import capi, evaluate
    header = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"#define\s+GS_ABI_VERSION\s+7\b", code)
    for n in NAMES:
        assert n in capi.PROTOTYPES and n in capi.DEVICE_ONLY, n
        m = re.search(r"\bgs_%s\s*\(([^)]*)\)" % n, code)
        assert m, n
        assert len(capi.PROTOTYPES[n][1]) == len([a for a in m.group(1).split(",") if a.strip()]), n
    assert len(capi.PROTOTYPES["eval_metrics"][1]) == 14, "gs_eval_metrics keeps its signature"
    assert (evaluate.WORDS, evaluate._SSIM_SK, evaluate.SK_WIN) == (8, 5, 7)


def test_size_queries_are_host_functions():
    from gsplat_amd._lib import hip_api
    api = hip_api()
    rt, st = api.raw("resize_tmp_bytes"), api.raw("eval_ssim_sk_tmp_bytes")
    assert api.raw("abi_version")() == 7
    assert rt(300, 400, 3, 75, 100) >= 300 * 100 * 3 and rt(300, 400, 3, 75, 100) % 256 == 0
    assert rt(300, 400, 3, 300, 100) == 0 and rt(300, 400, 3, 75, 400) == 0 and rt(300, 400, 3, 300, 400) == 0   # a pass is skipped
    assert rt(300, 400, 2, 75, 100) == 0 and rt(300, 400, 4, 75, 100) == 0 and rt(0, 400, 3, 75, 100) == 0 and rt(300, 400, 3, 75, 0) == 0
    assert st(3, 7, 7) >= 3 * 8 and st(3, 38, 38) >= 3 * 8 and st(3, 39, 38) >= 6 * 8 and st(4, 39, 39) >= 16 * 8
    assert st(3, 6, 40) == 0 and st(3, 40, 6) == 0 and st(0, 40, 40) == 0 and st(5, 40, 40) == 0


def test_evaluator_result_carries_ssim_sk_only_when_asked():
    from gsplat_amd.evaluate import Evaluator
    ev = Evaluator.__new__(Evaluator)
    ev.table = torch.tensor([[0.01, 20.0, 0.50, 0.10, 12.0, 0.25, 0, 0], [0.04, 14.0, 0.75, 0.20, 12.0, 0.75, 0, 0]], dtype=torch.float64)
    assert set(ev.result()) == {"SSIM", "PSNR", "L1", "per_view"}
    ev.ssim_sk = True
    r = ev.result(names=["a.png", "b.png"])
    assert set(r) == {"SSIM", "PSNR", "L1", "SSIM_sk", "per_view"} and r["SSIM_sk"] == 0.5
    assert set(r["per_view"]) == {"SSIM", "PSNR", "L1"}, "SSIM_sk is stored as the mean only"
    with pytest.raises(ValueError, match="no CPU path"):
        Evaluator(2, 3, 8, 8, "cpu", ssim_sk=True)
