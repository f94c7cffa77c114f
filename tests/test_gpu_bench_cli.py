"""bench.py's command line on the GPU: a plain run times the steps and reports only the headline
figure and its roofline, --dump-outputs writes the last timed step's outputs (the same from run
to run), --full adds the measurements beside the headline figure."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("per_step_launch", "idle_start", "host_api", "contact_cap", "one_step_err", "ls_cap", "qpos_rel_err",
             "cpu_baseline")


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--envs", "256",
           *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_only_and_dumps_are_reproducible(require_gpu, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench("--dump-outputs", str(a))
    _bench("--dump-outputs", str(b))
    assert d["steps"] == 3 and d["warmup"] == 2 and d["unit"] == "env-steps/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["value"] > 0
    # value = envs * steps / wall, ms_per_step = wall / steps (both rounded in the line)
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(256 / (d["ms_per_step"] / 1e3), rel=1e-2)
    assert not [k for k in FULL_ONLY if d.get(k) is not None]
    assert "latency" not in d["roofline"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == ["done.npy", "metrics.npy", "obs.npy", "reward.npy", "state.npy"]
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.shape[0] == 256 and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y)
    assert np.load(a / "obs.npy").shape == (256, 72) and np.abs(np.load(a / "obs.npy")).max() > 0


def test_full_adds_the_replay_and_dumps_the_same_outputs(require_gpu, tmp_path):
    p, f = tmp_path / "plain", tmp_path / "full"
    dp = _bench("--dump-outputs", str(p))
    df = _bench("--full", "--no-cpu-baseline", "--no-extras", "--no-latency-floor", "--dump-outputs", str(f))
    assert df["per_step_launch"]["bit_equal_to_rollout"] and df["per_step_launch"]["trajectory_last_row_equals_outputs"]
    assert df["state_sha16"] == dp["state_sha16"]
    for n in sorted(os.listdir(p)):
        np.testing.assert_array_equal(np.load(p / n), np.load(f / n))
