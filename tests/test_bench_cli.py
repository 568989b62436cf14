"""bench.py's command line: a plain run prints the headline line only (what
takes runs of its own is behind --full), --steps sets the number of timed
steps, and --dump-outputs writes what the last timed step computed, checked
here against the CPU oracle on the same world."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import pyoracle as po
from ccka import configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_bounded():
    assert np.array_equal(bench.dump_sample(100, 256), np.arange(100))
    a, b = bench.dump_sample(100_000, 256), bench.dump_sample(100_000, 256)
    assert np.array_equal(a, b) and len(a) == 256
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 100_000


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    n, T = 1000, 120
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--n", str(n), "--T", str(T), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["metric"] == "policy-evaluated cluster-steps/sec" and out["unit"] == "cluster-steps/s"
    assert out["higher_is_better"] is True and out["dtype"] == "int32+int64+f64"
    assert out["value"] == pytest.approx(n * T / (out["ms_per_step"] * 1e-3), rel=1e-9)
    # nothing that takes a run of its own
    assert "cpu_baseline" not in out and "parity" not in out and out["totals"] is None
    assert "copy_gbs" not in out["roofline"] and out["roofline"]["traffic"] is None

    spec = configs.config2_world(n_steps=T)
    sc = configs.hpa_scenarios(n)
    ref, reft = po.rollout(spec, sc, po.gen_load(configs.trace_gen(), T, 1, n), traj=True, threads=4)
    files = sorted(os.listdir(tmp_path / "out"))
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype in (np.float64, np.float32) for a in got.values())
    assert np.array_equal(got["results_index"], np.arange(n))
    for k in ref:
        assert np.array_equal(got["results_" + k], ref[k].astype(np.float64)), k
    cols = got["trajectory_index"].astype(np.int64)
    assert np.array_equal(cols, bench.dump_sample(n, bench.DUMP_TRAJ_COLS))
    for f in reft.dtype.names:
        assert np.array_equal(got["trajectory_" + f], reft[f][:, cols].astype(np.float64)), f
