"""bench.py's plain line and --dump-outputs: a run without --full prints the headline fields only,
and two runs with the same arguments write the same layers, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ["elevation", "elevation_angle", "num_observations", "observation_index", "ortho"]


def _bench(out_dir, steps):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "small",
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs_repeat(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench(a, 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["metric"] == "Mcells/s (DSM+ortho)" and d["dtype"] == "f64"
    for k in ("cpu_baseline", "parity_sample", "fast_mode", "launch_skips", "rough_terrain",
              "pcie_inclusive", "other_workloads"):
        assert k not in d, k
    _bench(b, 2)
    total = 0
    for name in LAYERS + [n + "_finite" for n in LAYERS]:
        x, y = np.load(str(a / (name + ".npy"))), np.load(str(b / (name + ".npy")))
        total += os.path.getsize(str(a / (name + ".npy")))
        # 2000 x 2000 cells: more than the sample, so a fixed 1-D sample of 2^20 cells
        assert x.dtype == np.float32 and x.shape == (1 << 20,), (name, x.dtype, x.shape)
        assert np.isfinite(x).all(), name
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    assert len(os.listdir(str(a))) == 2 * len(LAYERS)
    assert total <= 64 << 20
    for name in LAYERS:
        m = np.load(str(a / (name + "_finite.npy")))
        assert set(np.unique(m)) <= {0.0, 1.0}, name
        assert (np.load(str(a / (name + ".npy")))[m == 0.0] == 0.0).all(), name
    # elevation: nearly every cell has points; observation_index: NaN where no frame sees the cell
    assert np.load(str(a / "elevation_finite.npy")).mean() > 0.9
    assert np.load(str(a / "observation_index_finite.npy")).mean() > 0.5
