"""bench.py's plain run: the headline alone (no leg beside it), exactly --steps timed iterations, and --dump-outputs writing what
the timed run returned -- the same arrays, bit for bit, from a second process given the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("grid_path", "mfma_experiment", "surface_path", "whole_call", "c5_path", "cpu_baseline", "cpu_baseline_tiers")


def _bench(out_dir, steps):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--n-source", "120000",
           "--n-target", "100000", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    steps = 5
    d = _bench(tmp_path / "a", steps)
    assert d["metric"].startswith("ICP iterations/sec") and d["unit"] == "iterations/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == steps and d["value"] > 0
    assert abs(d["ms_per_step"] - 1e3 / d["value"]) <= 1e-9 * d["ms_per_step"]
    assert not [k for k in LEGS if k in d], [k for k in LEGS if k in d]
    assert "skipped" in d["roofline"]["measured_issue_ceiling"]["before_timed_loop"]     # the burns are --full's
    a = {f[:-4]: np.load(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a")}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["matrix_world"].shape == (4, 4) and a["matrix_world"].dtype == np.float32
    assert a["step_M"].shape == (steps, 4, 4) and a["step_K"].shape == (steps,)
    assert float(a["iters_done"]) == steps and float(a["last_K"]) == d["result"]["last_K"] == a["step_K"][-1]
    assert float(a["mean_dist"]) == d["result"]["mean_dist"]
    assert float(a["last_translation"]) == d["result"]["final_translation"]
    b_dir = tmp_path / "b"
    _bench(b_dir, steps)
    b = {f[:-4]: np.load(os.path.join(b_dir, f)) for f in os.listdir(b_dir)}
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
