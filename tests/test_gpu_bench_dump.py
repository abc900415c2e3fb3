"""bench.py --dump-outputs on the plumbing configuration: the result line reports the steps asked for, and the last timed
step's loss and sampled model rows land in DIR as float32 / float64 arrays within the size bound."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "3",
                        "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
    arrays = {f[:-len(".npy")]: np.load(out / f) for f in os.listdir(out)}
    assert set(arrays) >= {"loss", "rows", "xyz", "features", "opacity", "scaling", "rotation", "exp_avg_xyz",
                           "exp_avg_sq_features", "xyz_gradient_accum", "denom", "max_radii2D"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    P = 2000  # bench.CONFIGS["tiny"]: fewer rows than bench.DUMP_ROWS, so every row is written, in order
    assert np.array_equal(arrays["rows"], np.arange(P, dtype=np.float64))
    assert arrays["xyz"].shape == (P, 3) and arrays["features"].shape == (P, 16, 3)
    assert arrays["loss"].shape == () and np.isfinite(arrays["loss"]) and float(arrays["loss"]) > 0
    assert all(np.isfinite(a).all() for a in arrays.values())
    # the timed steps moved the model: some Gaussian has a non-zero first moment
    assert np.abs(arrays["exp_avg_xyz"]).max() > 0
