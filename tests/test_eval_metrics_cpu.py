"""Test-set evaluation (gsplat_amd/evaluate.py, csrc/gs_eval.hip), the parts that need no GPU: the float64 restatement
against the reference's recorded values, the ABI's three names, the result files' nesting, the means of a hand-filled table,
and the refusal of CPU tensors."""
import json
import os
import re

import numpy as np
import pytest
import torch

import eval_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
NAMES = ("eval_partials_count", "eval_tmp_bytes", "eval_metrics")


def fixture_cases():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"])), json.loads(str(z["metrics"]))


def case_inputs(z, c):
    """The seeded inputs of a fixture case, checked against the checksums the generator recorded."""
    render, gt = ref.seeded_pair(3, c["H"], c["W"], c["seed"], c["spread"])
    mask = ref.seeded_mask(c["H"], c["W"], c["mask_seed"]) if c["masked"] else None
    sums = [float(render.double().sum()), float(gt.double().sum()), float(mask.double().sum()) if c["masked"] else 0.0]
    assert np.allclose(sums, z[c["key"] + "_checksum"], rtol=1e-12, atol=0), "the seeded inputs are not the generator's"
    return render, gt, mask


@pytest.mark.parametrize("key", [c["key"] for c in fixture_cases()[1]])
def test_restatement_reproduces_the_recorded_reference_values(key):
    """tests/eval_reference.py gives the float64 values the generator recorded (to float64 rounding: a different BLAS or
    thread count may reorder a convolution's sums), and so lies at the recorded distance from the reference's float32."""
    z, cases, names = fixture_cases()
    c = next(c for c in cases if c["key"] == key)
    render, gt, mask = case_inputs(z, c)
    got = ref.metrics(render, gt, mask, c["clamp"], c["quantise"])
    for i, n in enumerate(names):
        f64, r32, dist = z[key + "_f64"][i], z[key + "_ref"][i], z[key + "_dist"][i]
        assert abs(got[n] - f64) <= 1e-12 * max(1.0, abs(f64)), (n, got[n], f64)
        assert abs(got[n] - r32) <= dist + 1e-12 * max(1.0, abs(r32)), (n, got[n], r32, dist)
    # the reference's float32 cannot be further from exact than float32 sums of this many terms go: a fixture whose
    # recorded distance were large would make the GPU test's margin meaningless
    assert z[key + "_dist"][names.index("psnr")] < 1e-4 and z[key + "_dist"][names.index("ssim")] < 1e-5
    assert z[key + "_dist"][names.index("count")] == 0


def test_fixture_covers_the_forms_and_says_how_the_quantisation_was_checked():
    z, cases, _ = fixture_cases()
    assert {(c["H"], c["W"]) for c in cases} == {(37, 53), (64, 96)}
    assert any(c["spread"] > 0 for c in cases) and any(c["masked"] for c in cases)
    assert any(c["quantise"] and not c["clamp"] for c in cases) and any(c["clamp"] and not c["quantise"] for c in cases)
    assert "PNG" in str(z["notes"])
    m = ref.seeded_mask(64, 96, cases[0]["mask_seed"])
    assert 0 < int((m == 1).sum()) < m.numel() and int(((m > 0) & (m < 1)).sum()) > 0, "the mask is not grey"


def test_abi_names_in_prototypes_device_only_and_header():
    from gsplat_amd import capi
    header = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NAMES:
        assert n in capi.PROTOTYPES, n
        assert n in capi.DEVICE_ONLY, n
        assert re.search(r"\bgs_%s\s*\(" % n, code), n
    assert len(capi.PROTOTYPES["eval_metrics"][1]) == 14
    for flag, v in (("GS_EVAL_CLAMP", 1), ("GS_EVAL_QUANTISE", 2), ("GS_EVAL_MASK_DTU", 4), ("GS_EVAL_WORDS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (flag, v), code), flag
    from gsplat_amd import evaluate
    assert (evaluate.CLAMP, evaluate.QUANTISE, evaluate.MASK_DTU, evaluate.WORDS) == (1, 2, 4, 8)


def test_size_queries_are_host_functions():
    from gsplat_amd._lib import hip_api
    api = hip_api()
    n, b = api.raw("eval_partials_count"), api.raw("eval_tmp_bytes")
    assert n(3, 32, 32) == 3 and n(1, 1, 1) == 1 and n(3, 33, 65) == 3 * 2 * 3 and n(3, 131, 260) == 3 * 5 * 9
    assert n(0, 32, 32) == 0 and n(5, 32, 32) == 0 and n(3, 0, 32) == 0 and b(3, 32, 0) == 0
    assert b(3, 33, 65) >= 18 * 5 * 8 and b(3, 33, 65) % 256 == 0


def test_write_results_json_nesting(tmp_path):
    from gsplat_amd import evaluate, io
    assert evaluate.write_results_json is io.write_results_json
    result = {"SSIM": 0.9, "PSNR": 25.5, "L1": 0.03,
              "per_view": {"SSIM": {"00000.png": 0.91, "00001.png": 0.89}, "PSNR": {"00000.png": 26.0, "00001.png": 25.0},
                           "L1": {"00000.png": 0.02, "00001.png": 0.04}}}
    io.write_results_json(str(tmp_path / "model"), "ours_30000", result)
    full = json.load(open(tmp_path / "model" / "results.json"))
    per = json.load(open(tmp_path / "model" / "per_view.json"))
    assert full == {"ours_30000": {"SSIM": 0.9, "PSNR": 25.5, "L1": 0.03}}
    assert per == {"ours_30000": result["per_view"]}
    assert "LPIPS" not in full["ours_30000"] and "LPIPS" not in per["ours_30000"]
    assert list(per["ours_30000"]["PSNR"]) == ["00000.png", "00001.png"]


def test_evaluator_result_means_of_a_hand_filled_table():
    from gsplat_amd.evaluate import Evaluator
    ev = Evaluator.__new__(Evaluator)   # (no device: result() reads the table and nothing else)
    #                          mse   psnr  ssim  l1    count
    ev.table = torch.tensor([[0.01, 20.0, 0.50, 0.10, 12.0, 0, 0, 0],
                             [0.04, 14.0, 0.75, 0.20, 12.0, 0, 0, 0],
                             [0.0, float("inf"), 1.0, 0.0, 12.0, 0, 0, 0]], dtype=torch.float64)
    two = Evaluator.__new__(Evaluator)
    two.table = ev.table[:2].clone()
    r = two.result(names=["a.png", "b.png"])
    assert r["PSNR"] == 17.0 and r["SSIM"] == 0.625 and abs(r["L1"] - 0.15) < 1e-15
    assert r["per_view"] == {"SSIM": {"a.png": 0.5, "b.png": 0.75}, "PSNR": {"a.png": 20.0, "b.png": 14.0},
                             "L1": {"a.png": 0.1, "b.png": 0.2}}
    assert set(r) == {"SSIM", "PSNR", "L1", "per_view"}
    r3 = ev.result()   # default names are render.py's file names; a perfect view makes the mean infinite, as in the reference
    assert list(r3["per_view"]["PSNR"]) == ["00000.png", "00001.png", "00002.png"] and r3["PSNR"] == float("inf")
    with pytest.raises(ValueError):
        ev.result(names=["only-one"])


def test_image_metrics_refuses_cpu_and_malformed_input():
    from gsplat_amd.evaluate import Evaluator, image_metrics, psnr, ssim
    a = torch.rand(3, 8, 8)
    with pytest.raises(ValueError, match="no CPU path"):
        image_metrics(a, a)
    with pytest.raises(ValueError, match="batch 1 only"):
        image_metrics(torch.rand(2, 3, 8, 8), torch.rand(2, 3, 8, 8))
    with pytest.raises(ValueError):
        image_metrics(torch.rand(8, 8), torch.rand(8, 8))
    with pytest.raises(ValueError, match="no CPU path"):
        psnr(a[None], a[None])
    with pytest.raises(ValueError, match="window_size 11"):
        ssim(a[None], a[None], window_size=7)
    with pytest.raises(ValueError, match="no CPU path"):
        Evaluator(2, 3, 8, 8, "cpu")
