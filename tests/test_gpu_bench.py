"""GPU (-m gpu): bench.py as the driver runs it -- a plain run times exactly --steps steps once and writes what its last
step computed with --dump-outputs; --full adds the repeats, the expected line, the roofline and the CPU baseline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_the_given_steps_and_dumps_the_last_one(tmp_path):
    runs = []
    for d in ("a", "b"):
        res = run_bench("--steps", "30", "--warmup", "5", "--dump-outputs", str(tmp_path / d))
        assert res["steps"] == 30 and res["repeats"] == 1 and res["full"] is False
        assert res["ms_per_step"] > 0 and abs(res["value"] - 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
        assert res["metric"] == "ELBO-steps/sec (N x M kernel + chol + flow), Power M=100 S=32" and res["dtype"] == "f64"
        assert "roofline" not in res and "cpu_baseline" not in res and "expected" not in res["config"]
        runs.append(res)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    for p in ("Z", "raw_lengthscale", "raw_outputscale", "m", "Lam", "log_var_noise", "theta"):
        assert "grad_%s.npy" % p in names and "param_%s.npy" % p in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 2 ** 20
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.isfinite(a).all(), n
        assert np.allclose(a, b, rtol=1e-12, atol=0.0), n              # same inputs, same steps: same outputs
    e = np.load(tmp_path / "a" / "elbo_ell_kl.npy")
    assert e.shape == (3,) and e[0] == runs[0]["config"]["final_elbo"]
    assert np.load(tmp_path / "a" / "param_Lam.npy").shape == (100, 100)


def test_full_run_keeps_the_extras():
    res = run_bench("--steps", "20", "--warmup", "5", "--full", "--cpu-seconds", "2")
    assert res["full"] is True and res["steps"] == 20 and res["repeats"] >= 5
    assert res["ms_per_step_min"] <= res["ms_per_step"] <= res["ms_per_step_max"]
    assert res["roofline"]["kernel_ms"] > 0 and 0 < res["roofline"]["frac"] < 1
    assert res["config"]["expected"]["measured_value"] == res["value"]
    assert res["cpu_baseline"]["value"] > 0
