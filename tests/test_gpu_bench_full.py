"""bench.py's two kinds of run on the plumbing configuration: a plain run ends with the timed steps and what they left,
--full adds the untimed legs after them - and the timed steps compute the same in both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("reference_lists", "options", "drop_in_api", "cpu_baseline")   # the --full legs that run on the tiny config


def run_bench(out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out), *extra],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}


@pytest.mark.gpu
def test_full_adds_the_untimed_legs_after_the_timed_steps(tmp_path):
    plain, plain_out = run_bench(tmp_path / "plain")
    full, full_out = run_bench(tmp_path / "full", "--full")
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert plain[key] == full[key], key
    for line in (plain, full):
        assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    assert all(plain[k] is None for k in LEGS), {k: plain[k] is None for k in LEGS}
    assert all(full[k] is not None for k in LEGS), {k: full[k] is None for k in LEGS}
    assert full["cpu_baseline"]["value"] > 0 and full["reference_lists"]["ms_per_step"] > 0
    # a plain run: the dominant kernel as the timed region measured it, and its roofline; --full: every stage
    assert len(plain["stages"]) == 1 and plain["roofline"]["kernel"] in plain["stages"]
    assert set(full["stages"]) > set(plain["stages"]) and full["roofline"] is not None
    # the legs of --full run after the dump: both runs wrote the same step (up to the run-to-run spread of the float sums)
    assert set(plain_out) == set(full_out)
    assert abs(float(plain_out["loss"]) - float(full_out["loss"])) <= 1e-4 * abs(float(full_out["loss"]))
    for k, a in full_out.items():
        d = (plain_out[k].astype(np.float64) - a).ravel()
        assert np.sqrt(np.mean(d * d)) <= 1e-3 * max(np.sqrt(np.mean(a.astype(np.float64) ** 2)), 1e-12), k
