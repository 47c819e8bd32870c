"""bench.py without --full on the GPU: the lean result line, and --dump-outputs writing what the timed path
computed. The same arguments with --full give the same dumped arrays bit for bit, and that run's per-frame
checksums of the very same tensors equal the oracle-written table, so the dumped values are the checked ones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--config", "3", "--steps", "4", "--warmup", "1"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "cpu_baseline", "frame_checksums", "comm", "index_errors"}


def _bench(args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_checked_outputs(tmp_path):
    d_plain, d_full = str(tmp_path / "plain"), str(tmp_path / "full")
    plain = _bench([*ARGS, "--dump-outputs", d_plain])
    full = _bench([*ARGS, "--full", "--no-cpu-baseline", "--dump-outputs", d_full])
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain) and plain["full"] is False
    assert HEADLINE | FULL_ONLY <= set(full) and full["full"] is True
    for line in (plain, full):
        assert line["steps"] == 4 and line["warmup"] == 1 and line["unit"] == "frames/s" and line["dtype"] == "bf16"
        assert line["higher_is_better"] is True and line["metric"] == full["metric"]
        # value = frames of the timed steps / elapsed, ms_per_step = elapsed / steps (4 frames per step)
        assert line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(4 / (line["ms_per_step"] * 1e-3), rel=1e-2)
    assert full["frame_checksums"]["match_n1"] is True and full["index_errors"] == 0
    names = ["bv_fused.npy", "d_bev.npy", "d_img.npy", "img_fused.npy"]
    assert sorted(os.listdir(d_plain)) == sorted(os.listdir(d_full)) == names and sorted(plain["dumped"]) == names
    total = 0
    for n in names:
        a, b = np.load(os.path.join(d_plain, n)), np.load(os.path.join(d_full, n))
        assert a.dtype == np.float32 and a.size == plain["dumped"][n]["written"] and np.count_nonzero(a) > 0
        np.testing.assert_array_equal(a, b)
        total += os.path.getsize(os.path.join(d_plain, n))
    assert total <= 64 * 10 ** 6
