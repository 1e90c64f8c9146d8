"""bench.py's plain single-rank run: the headline line alone, without the legs that only --full runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_line_only(tmp_path):
    """Without --full the line carries the headline fields and the roofline of the timed steps, and none of the parity check,
    the CPU baselines, the config-3 timings or the exchange; --dump-outputs still writes what the last step computed."""
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(dump)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "cost-volume Mvoxels/s (5v x 384D)" and d["unit"] == "Mvoxels/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["priced_against"] == "hbm"
    assert not {"parity", "cpu_baseline", "secondary", "exchange", "per_rank"} & set(d)
    assert np.load(dump / "variance_volume_plane192.npy").shape == (32, 688, 464)
    assert np.load(dump / "variance_volume_sample.npy").dtype == np.float32
