"""A plain bench.py run on a small configuration: --steps sets the timed steps, the line carries ms_per_step and nothing of
--full, and --dump-outputs writes the same network from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg2", "--steps", "4",
                        "--warmup", "1", "--dump-outputs", out_dir], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    a, b = _bench(str(tmp_path / "a")), _bench(str(tmp_path / "b"))
    for js in (a, b):
        assert js["steps"] == 4 and js["ms_per_step"] > 0 and not js["full"]
        assert js["other_schedule"] is None and js["cpu_baseline"] is None
    assert a["network_sha256"] == b["network_sha256"]
    src = np.load(tmp_path / "a" / "edge_src.npy")
    assert src.dtype == np.float64 and src.size == a["edges"]
    for k in ("edge_src", "edge_dst", "edge_weight", "pc_off", "pc_idx", "pc_weight", "pc_pval", "pc_tested"):
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == np.float64 and np.isfinite(got).all(), k
        np.testing.assert_array_equal(got, np.load(tmp_path / "b" / (k + ".npy")))
