"""Evaluation from files on the device (csrc/gs_eval_files.hip, gsplat_amd/imageio.py, gsplat_amd/render_set.py).

Resize: exact.  Every case of tests/golden/pil_resize.npz - Pillow's recorded bytes - with torch.equal, both outputs.
SSIM_sk: against the float64 restatement tests/eval_files_reference.py::ssim_sk_f64 on the same float32 pixels.  The bar of a
case is the distance of the float32 restatement of the same chain (what skimage runs on the reference's float32 arrays) from
float64 ON THAT CASE - the reference's own rounding, computed here - with a floor of 1e-12 for flat images, where that
distance is 0: three orders above float64 rounding of 1e5 terms.  The observed distances are printed, and written to the file
GS_EVAL_FILES_PARITY_OUT names when it is set (a run of that kind is kept as profiles/eval_files_parity.json).
No Pillow, scipy or matplotlib here: the fixtures carry what those produced."""
import json
import os

import numpy as np
import pytest
import torch

import eval_files_reference as fref
import eval_reference as ref
from gsplat_amd import evaluate, imageio, render_set

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
E_NULL, E_SHAPE = -1, -2
CASES = fref.fixture_cases()
GUARD, PAD = 0xA5, 256
PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def _write_parity():
    yield
    out = os.environ.get("GS_EVAL_FILES_PARITY_OUT")
    if PARITY and out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fp:
            json.dump(PARITY, fp, indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------------------ resize
def raw_resize(hip, src, H2, W2, planar=True, override=None):
    """gs_resize_bicubic_u8 itself, output and scratch between guard bytes, scratch of exactly gs_resize_tmp_bytes
    -> (status, bytes [H2,W2,C], planar or None, guards intact?)"""
    H, W, C = src.shape
    api = hip.api
    nb = int(api.raw("resize_tmp_bytes")(H, W, C, H2, W2))
    n_out = H2 * W2 * C
    obuf = torch.full((PAD + n_out + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    tbuf = torch.full((PAD + nb + PAD,), GUARD, dtype=torch.uint8, device=DEV)
    fbuf = torch.full((64 + n_out + 64,), -7.0, dtype=torch.float32, device=DEV)
    xb, xc = imageio._tables_on(DEV, W, W2) if W2 != W else (None, None)
    yb, yc = imageio._tables_on(DEV, H, H2) if H2 != H else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = dict(inp=src.data_ptr(), H=H, W=W, C=C, H2=H2, W2=W2, xb=ptr(xb), xc=ptr(xc), kx=0 if xc is None else xc.shape[1],
                yb=ptr(yb), yc=ptr(yc), ky=0 if yc is None else yc.shape[1], tmp=(tbuf.data_ptr() + PAD) if nb else None,
                tmp_bytes=nb, out=obuf.data_ptr() + PAD,
                outf=(fbuf.data_ptr() + 64 * 4) if planar else None)
    args.update(override or {})
    rc = api.raw("resize_bicubic_u8")(*[args[k] for k in ("inp", "H", "W", "C", "H2", "W2", "xb", "xc", "kx", "yb", "yc", "ky", "tmp",
                                                           "tmp_bytes", "out", "outf")], None)
    torch.cuda.synchronize()
    intact = (bool((obuf[:PAD] == GUARD).all()) and bool((obuf[PAD + n_out:] == GUARD).all())
              and bool((tbuf[:PAD] == GUARD).all()) and bool((tbuf[PAD + nb:] == GUARD).all())
              and bool((fbuf[:64] == -7.0).all()) and bool((fbuf[64 + n_out:] == -7.0).all()))
    untouched = bool((obuf == GUARD).all()) and bool((tbuf == GUARD).all()) and bool((fbuf == -7.0).all())
    return rc, obuf[PAD:PAD + n_out].reshape(H2, W2, C), fbuf[64:64 + n_out].reshape(C, H2, W2) if planar else None, intact, untouched


@pytest.mark.parametrize("key", [c[0] for c in CASES])
def test_resize_equals_pillows_recorded_bytes(hip, key):
    z = np.load(GOLDEN)
    _, make, (H, W), (H2, W2), C = next(c for c in CASES if c[0] == key)
    a = make()
    assert fref.crc(a) == int(z[key + "_crc"]), "the seeded input is not the generator's"
    want = torch.from_numpy(np.ascontiguousarray(z[key + "_out"] if key + "_out" in z.files else a))
    rc, got, planar, intact, _ = raw_resize(hip, torch.from_numpy(a).to(DEV), H2, W2)
    assert rc == 0 and intact, "a guard byte around the output or the scratch was written"
    assert torch.equal(got.cpu(), want), (got.cpu().int() - want.int()).abs().max()
    assert torch.equal(planar.cpu(), want.permute(2, 0, 1).to(torch.float32).div(255)), "planar fp32 is not bytes / 255"
    # the public entry: the same bytes, on the device, both outputs; without the planar image too
    out, pl = imageio.resize_u8(torch.from_numpy(a).to(DEV), (W2, H2), return_planar=True)
    assert out.is_cuda and out.dtype == torch.uint8 and torch.equal(out.cpu(), want) and torch.equal(pl, planar)
    rc, got, _, intact, _ = raw_resize(hip, torch.from_numpy(a).to(DEV), H2, W2, planar=False)
    assert rc == 0 and intact and torch.equal(got.cpu(), want)
    if C == 1:
        assert torch.equal(imageio.resize_u8(torch.from_numpy(a[:, :, 0]).to(DEV), (W2, H2)).cpu(), want[:, :, 0])


def test_resize_from_an_unaligned_source(hip):
    """The vertical pass reads words when it can: a source 1 byte off a word boundary, and row lengths off a multiple of 4."""
    for (H, W), (H2, W2), C in (((37, 64), (9, 64), 3), ((37, 63), (9, 63), 1), ((37, 63), (9, 17), 3)):
        a = fref.seeded_u8(H, W, C, seed=77)
        buf = torch.zeros(H * W * C + 8, dtype=torch.uint8, device=DEV)
        src = buf[1:1 + H * W * C].reshape(H, W, C)
        src.copy_(torch.from_numpy(a))
        assert src.data_ptr() % 4 == 1
        rc, got, planar, intact, _ = raw_resize(hip, src, H2, W2)
        want = torch.from_numpy(imageio.resize_u8_numpy(a, (W2, H2)))
        assert rc == 0 and intact and torch.equal(got.cpu(), want)
        assert torch.equal(planar.cpu(), want.permute(2, 0, 1).to(torch.float32).div(255))


def test_resize_status_codes(hip):
    src = torch.from_numpy(fref.seeded_u8(37, 64, 3, seed=1)).to(DEV)
    nb = int(hip.api.raw("resize_tmp_bytes")(37, 64, 3, 9, 16))
    assert nb >= 37 * 16 * 3
    for override in (dict(inp=None), dict(out=None), dict(xb=None), dict(xc=None), dict(yb=None), dict(yc=None), dict(tmp=None)):
        rc, _, _, _, untouched = raw_resize(hip, src, 9, 16, override=override)
        assert rc == E_NULL and untouched, override
    for override in (dict(C=2), dict(C=4), dict(C=0), dict(H=0), dict(W=-1), dict(H2=0), dict(W2=0), dict(kx=0), dict(ky=-3),
                     dict(tmp_bytes=nb - 1), dict(tmp_bytes=0)):
        rc, _, _, _, untouched = raw_resize(hip, src, 9, 16, override=override)
        assert rc == E_SHAPE and untouched, override
    # a skipped pass needs neither its tables nor scratch
    rc, got, _, intact, _ = raw_resize(hip, src, 37, 16, override=dict(yb=None, yc=None, tmp=None, tmp_bytes=0))
    assert rc == 0 and intact and torch.equal(got.cpu(), torch.from_numpy(imageio.resize_u8_numpy(src.cpu().numpy(), (16, 37))))
    with pytest.raises(ValueError, match="premultiplies"):
        imageio.resize_u8(torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV), (2, 2))


def test_resize_with_a_table_that_leaves_the_source_reads_nothing(hip):
    """Runs that leave the source axis give 0 for their samples and touch nothing else (the kernel checks each run)."""
    a = fref.seeded_u8(13, 29, 1, seed=3)
    src = torch.from_numpy(a).to(DEV)
    xb, xc = (t.clone() for t in imageio._tables_on(DEV, 29, 7))
    xb[2, 0] = 29            # starts beyond the row
    xb[4, 1] = xc.shape[1] + 1   # longer than the table row
    rc, got, _, intact, _ = raw_resize(hip, src, 13, 7, override=dict(xb=xb.data_ptr(), xc=xc.data_ptr()))
    want = torch.from_numpy(imageio.resize_u8_numpy(a, (7, 13)))
    want[:, 2] = 0
    want[:, 4] = 0
    assert rc == 0 and intact and torch.equal(got.cpu(), want)


# ----------------------------------------------------------------------------------------------------------- SSIM_sk
SK_SIZES, SK_FLAGS = fref.SK_SIZES, fref.SK_FLAGS   # (kept beside the restatement: a CPU test holds the committed record to them)
_sk_inputs = {}


def sk_inputs(Cn, H, W):
    key = (Cn, H, W)
    if key not in _sk_inputs:
        render, gt = ref.seeded_pair(Cn, H, W, seed=300 + 11 * H + W + Cn, spread=0.2)
        mask = ref.seeded_mask(H, W, seed=H + 2 * W)
        _sk_inputs[key] = (render, gt, mask, render.to(DEV), gt.to(DEV), mask.to(DEV))
    return _sk_inputs[key]


def sk_want(render, gt, mask, clamp, quantise):
    """-> (float64 restatement, float32 restatement) on the transformed float32 pixels"""
    a = ref.transform(render, mask, clamp, quantise).numpy()
    b = ref.transform(gt, mask, clamp, quantise).numpy()
    return fref.ssim_sk_f64(a, b), fref.ssim_sk_f32(a, b)


def raw_sk(hip, render, gt, mask, flags, tmp=None, out=None):
    Cn, H, W = render.shape
    nb = int(hip.api.raw("eval_ssim_sk_tmp_bytes")(Cn, H, W))
    if tmp is None:
        tmp = torch.empty((max(nb, 8),), dtype=torch.uint8, device=DEV)
    if out is None:
        out = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)
    rc = hip.api.raw("eval_ssim_sk")(render.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), Cn, H, W, flags,
                                     tmp.data_ptr(), nb, out[1:].data_ptr(), None)
    return rc, out


@pytest.mark.parametrize("form", list(SK_FLAGS))
@pytest.mark.parametrize("Cn", fref.SK_CHANNELS)
@pytest.mark.parametrize("H,W", SK_SIZES)
def test_ssim_sk_matches_the_float64_restatement(hip, H, W, Cn, form):
    clamp, quantise, masked = SK_FLAGS[form]
    render, gt, mask, r, g, m = sk_inputs(Cn, H, W)
    got = evaluate.image_metrics(r, g, mask=m if masked else None, clamp=clamp, quantise=quantise, ssim_sk=True)
    f64, f32 = sk_want(render, gt, mask if masked else None, clamp, quantise)
    bar = max(abs(f32 - f64), fref.SK_FLOOR)
    v = float(got["ssim_sk"])
    print("%dx%dx%d %-8s got %.17g want %.17g |got - want| %.3g bar %.3g" % (Cn, H, W, form, v, f64, abs(v - f64), bar))
    PARITY[fref.sk_case_key(Cn, H, W, form)] = {"abs_err": abs(v - f64), "bar_f32_vs_f64": abs(f32 - f64), "value": f64}
    assert got["ssim_sk"].dtype == torch.float64 and got["ssim_sk"].dim() == 0 and got["ssim_sk"].is_cuda
    assert abs(v - f64) <= bar
    # the other words are what they are without ssim_sk
    plain = evaluate.image_metrics(r, g, mask=m if masked else None, clamp=clamp, quantise=quantise)
    assert "ssim_sk" not in plain
    for k in ("mse", "psnr", "ssim", "l1", "count"):
        assert plain[k].reshape(1).view(torch.int64).item() == got[k].reshape(1).view(torch.int64).item(), k


def test_ssim_sk_flat_and_identical_images(hip):
    flat = torch.full((3, 33, 40), 0.25, device=DEV)
    got = float(evaluate.image_metrics(flat, flat.clone(), ssim_sk=True)["ssim_sk"])
    assert abs(got - 1.0) <= 1e-12
    other = torch.full((3, 33, 40), 0.75, device=DEV)
    want = fref.ssim_sk_f64(flat.cpu().numpy(), other.cpu().numpy())
    got = float(evaluate.image_metrics(flat, other, ssim_sk=True)["ssim_sk"])
    PARITY["flat_0.25_vs_0.75"] = {"abs_err": abs(got - want), "bar_f32_vs_f64": 0.0, "value": want}
    assert abs(got - want) <= 1e-12
    img = sk_inputs(3, 33, 40)[3]
    for clamp, quantise in ((False, False), (True, True)):
        got = float(evaluate.image_metrics(img, img.clone(), clamp=clamp, quantise=quantise, ssim_sk=True)["ssim_sk"])
        assert abs(got - 1.0) <= 1e-12
    # everything is white under an all-zero mask
    r, g = sk_inputs(3, 33, 40)[3:5]
    got = float(evaluate.image_metrics(r, g, mask=torch.zeros(33, 40, device=DEV), ssim_sk=True)["ssim_sk"])
    assert abs(got - 1.0) <= 1e-12


def test_ssim_sk_same_bits_on_every_run_and_from_nan_scratch(hip):
    render, gt, mask, r, g, m = sk_inputs(3, 131, 260)
    flags = evaluate.CLAMP | evaluate.QUANTISE | evaluate.MASK_DTU
    rc1, first = raw_sk(hip, r, g, m, flags)
    rc2, second = raw_sk(hip, r, g, m, flags)
    nb = int(hip.api.raw("eval_ssim_sk_tmp_bytes")(3, 131, 260))
    tmp = torch.full((nb // 8 + 4,), float("nan"), dtype=torch.float64, device=DEV)
    rc3, third = raw_sk(hip, r, g, m, flags, tmp=tmp.view(torch.uint8))
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    bits = lambda t: t.view(torch.int64).cpu()  # noqa: E731
    assert torch.equal(bits(first), bits(second)) and torch.equal(bits(first), bits(third))
    assert first[0].item() == -7.0 and first[2].item() == -7.0, "ONE double is written"
    assert bool(torch.isnan(tmp[nb // 8:]).all()), "scratch beyond the size query's bytes was written"
    f64, f32 = sk_want(render, gt, mask, True, True)
    assert abs(first[1].item() - f64) <= max(abs(f32 - f64), 1e-12)


def test_ssim_sk_status_codes(hip):
    img = torch.rand(3, 16, 16, device=DEV)
    m = torch.ones(16, 16, device=DEV)
    f = hip.api.raw("eval_ssim_sk")
    nb = int(hip.api.raw("eval_ssim_sk_tmp_bytes")(3, 16, 16))
    tmp = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    out = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    assert f(None, p(img), None, 3, 16, 16, 0, p(tmp), nb, p(out), None) == E_NULL
    assert f(p(img), None, None, 3, 16, 16, 0, p(tmp), nb, p(out), None) == E_NULL
    assert f(p(img), p(img), None, 3, 16, 16, 0, None, nb, p(out), None) == E_NULL
    assert f(p(img), p(img), None, 3, 16, 16, 0, p(tmp), nb, None, None) == E_NULL
    assert f(p(img), p(img), None, 3, 16, 16, 4, p(tmp), nb, p(out), None) == E_NULL     # MASK_DTU without a mask
    assert f(p(img), p(img), None, 3, 6, 16, 0, p(tmp), nb, p(out), None) == E_SHAPE      # H = 6: skimage raises there
    assert f(p(img), p(img), None, 3, 16, 6, 0, p(tmp), nb, p(out), None) == E_SHAPE
    assert f(p(img), p(img), None, 0, 16, 16, 0, p(tmp), nb, p(out), None) == E_SHAPE
    assert f(p(img), p(img), None, 5, 16, 16, 0, p(tmp), nb, p(out), None) == E_SHAPE
    assert f(p(img), p(img), p(m), 3, 16, 16, 8, p(tmp), nb, p(out), None) == E_SHAPE     # unknown flag bit
    assert f(p(img), p(img), None, 3, 16, 16, 0, p(tmp), nb - 1, p(out), None) == E_SHAPE
    torch.cuda.synchronize()
    assert out.item() == -7.0 and int(tmp.max()) == 0, "a refused call wrote something"
    assert f(p(img), p(img), p(m), 3, 16, 16, 7, p(tmp), nb, p(out), None) == 0
    torch.cuda.synchronize()
    assert abs(out.item() - 1.0) <= 1e-12
    small = torch.rand(3, 6, 40, device=DEV)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        evaluate.image_metrics(small, small, ssim_sk=True)
    with pytest.raises(ValueError, match="at least 7 x 7"):
        evaluate.Evaluator(2, 3, 6, 40, DEV, ssim_sk=True)
    assert float(evaluate.image_metrics(small, small)["l1"]) == 0.0   # (without ssim_sk such a view is scored as before)


def test_evaluator_word_5_is_written_only_when_asked(hip):
    Cn, H, W = 3, 33, 40
    pairs = [ref.seeded_pair(Cn, H, W, seed=40 + i, spread=0.1) for i in range(3)]
    dev = [(a.to(DEV), b.to(DEV)) for a, b in pairs]
    bits = lambda t: t.contiguous().view(torch.int64).cpu()  # noqa: E731
    plain, sk = evaluate.Evaluator(5, Cn, H, W, DEV), evaluate.Evaluator(5, Cn, H, W, DEV, ssim_sk=True)
    initial = bits(sk.table)
    for i in (2, 0, 1):
        plain.add(i, dev[i][0], dev[i][1], clamp=True, quantise=True)
        sk.add(i, dev[i][0], dev[i][1], clamp=True, quantise=True)
    tp, ts = bits(plain.table), bits(sk.table)
    assert torch.equal(tp[:, :5], ts[:, :5]) and torch.equal(tp[:, 6:], ts[:, 6:])
    assert plain.table[:3, 5].tolist() == [0.0, 0.0, 0.0], "word 5 stays reserved = 0 unless asked for"
    assert sk.table[:3, 6:].abs().sum().item() == 0.0
    assert torch.equal(ts[3:], initial[3:]) and torch.equal(tp[3:], initial[3:]), "rows no view was added to were written"
    for i in range(3):
        one = evaluate.image_metrics(dev[i][0], dev[i][1], clamp=True, quantise=True, ssim_sk=True)["ssim_sk"]
        assert one.reshape(1).view(torch.int64).item() == ts[i, 5].item()
    three = evaluate.Evaluator(3, Cn, H, W, DEV, ssim_sk=True)
    for i in range(3):
        three.add(i, dev[i][0], dev[i][1], clamp=True, quantise=True)
    res, res_plain = three.result(), evaluate.Evaluator.result(plain)
    assert set(res) == {"SSIM", "PSNR", "L1", "SSIM_sk", "per_view"} and set(res["per_view"]) == {"SSIM", "PSNR", "L1"}
    assert set(res_plain) == {"SSIM", "PSNR", "L1", "per_view"}
    assert res["SSIM_sk"] == sum(float(v) for v in sk.table[:3, 5].cpu()) / 3


# ---------------------------------------------------------------------------------------------------------- end to end
def test_write_render_set_then_evaluate_dir(hip, tmp_path):
    from gsplat_amd.trainer import render
    from test_gpu_eval_metrics import small_trainer
    tr = small_trainer(hip, W=64, H=48)
    with torch.no_grad():
        renders = [render(c, tr.model, tr.Rasterizer, tr.Settings, tr.bg, clamp=False)["render"].clone() for c in tr.cameras]
    assert tuple(renders[0].shape) == (3, 48, 64) and float(renders[0].abs().max()) > 0
    model_path = str(tmp_path / "model")
    base = render_set.write_render_set(model_path, "test", 7, [{"render": r, "gt": g} for r, g in zip(renders, tr.gts)])
    assert base == os.path.join(model_path, "test", "ours_7")
    assert sorted(os.listdir(os.path.join(base, "renders"))) == ["00000.png", "00001.png", "00002.png"]
    assert sorted(os.listdir(base)) == ["gt", "renders"], "no depth folder without depth and alpha"
    res = render_set.evaluate_dir(model_path, "test", ssim_sk=True)
    assert list(res) == ["ours_7"]
    r7 = res["ours_7"]
    sks = []
    for i, name in enumerate(["00000.png", "00001.png", "00002.png"]):
        one = evaluate.image_metrics(renders[i], tr.gts[i], clamp=True, quantise=True, return_bytes=True, ssim_sk=True)
        assert r7["per_view"]["PSNR"][name] == float(one["psnr"])
        assert r7["per_view"]["SSIM"][name] == float(one["ssim"])
        assert r7["per_view"]["L1"][name] == float(one["l1"])
        sks.append(float(one["ssim_sk"]))
        assert np.array_equal(imageio.read_png(os.path.join(base, "renders", name)), one["bytes"].cpu().numpy())
        assert np.array_equal(imageio.read_png(os.path.join(base, "gt", name)), ref.to_bytes(tr.gts[i].cpu()).permute(1, 2, 0).numpy())
    assert r7["SSIM_sk"] == sum(sks) / 3
    full = json.load(open(os.path.join(model_path, "results.json")))
    per = json.load(open(os.path.join(model_path, "per_view.json")))
    assert full == {"ours_7": {k: r7[k] for k in ("SSIM", "PSNR", "L1", "SSIM_sk")}}
    assert per == {"ours_7": r7["per_view"]}
    plain = render_set.evaluate_dir(model_path, "test")["ours_7"]
    assert set(plain) == {"SSIM", "PSNR", "L1", "per_view"} and plain["PSNR"] == r7["PSNR"]


def test_evaluate_dir_dtu_leg(hip, tmp_path):
    """A 256 x 192 render, its ground truth and a 256 x 192 mask file: evaluate_dir(mask_dir=...) equals resize -> metrics
    done by hand with the fixture-pinned pieces (the numpy resize the CPU tests hold to Pillow's bytes)."""
    H, W = 192, 256
    pairs = [ref.seeded_pair(3, H, W, seed=80 + i, spread=0.1) for i in range(2)]
    model_path, mask_dir = str(tmp_path / "scan"), str(tmp_path / "scan" / "mask")
    base = render_set.write_render_set(model_path, "eval", 6000, [{"render": a.to(DEV), "gt": b.to(DEV)} for a, b in pairs])
    os.makedirs(mask_dir)
    mask8 = ref.to_bytes(ref.seeded_mask(H, W, seed=9)).numpy()
    for i in range(2):
        imageio.write_png(os.path.join(mask_dir, "%05d.png" % i), mask8)
    res = render_set.evaluate_dir(model_path, "eval", mask_dir=mask_dir, ssim_sk=True)["ours_6000"]
    small = imageio.resize_u8_numpy(mask8[:, :, None], (W // 4, H // 4))
    m = torch.from_numpy(small[:, :, 0].astype(np.float32) / np.float32(255))
    ones = int((m == 1.0).sum())
    assert 0 < ones < m.numel() and tuple(m.shape) == (48, 64)
    sks = []
    for i in range(2):
        name = "%05d.png" % i
        planes = []
        for folder in ("renders", "gt"):
            u8 = imageio.resize_u8_numpy(imageio.read_png(os.path.join(base, folder, name)), (W // 4, H // 4))
            planes.append(torch.from_numpy(np.ascontiguousarray(u8.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)).to(DEV))
        one = evaluate.image_metrics(planes[0], planes[1], mask=m.to(DEV), ssim_sk=True)
        assert float(one["count"]) == 3 * ones, "PSNR runs over the mask elements equal to 1 after the resize"
        assert res["per_view"]["PSNR"][name] == float(one["psnr"])
        assert res["per_view"]["SSIM"][name] == float(one["ssim"])
        assert res["per_view"]["L1"][name] == float(one["l1"])
        sks.append(float(one["ssim_sk"]))
        want = ref.metrics(planes[0].cpu(), planes[1].cpu(), m)   # and the float64 restatement of that hand-made pair
        assert abs(float(one["psnr"]) - want["psnr"]) <= 1e-5 and want["count"] == 3 * ones
    assert res["SSIM_sk"] == sum(sks) / 2
    with pytest.raises(ValueError, match="alpha"):
        imageio.write_png(os.path.join(mask_dir, "00000.png"), np.repeat(mask8[:, :, None], 2, axis=2))
        render_set.evaluate_dir(model_path, "eval", mask_dir=mask_dir)
