"""A plain `bench.py` run does only what its headline figure needs: set-up, warm-up, the timed steps, --dump-outputs and the
line.  The legs beside it (CPU baseline, host hand-over, kernels alone, full pipeline, files) run only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_has_no_legs_beside_the_timed_steps(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "ITSX_FORCE_DIST")}
    dump = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg1", "--reads", "20000",
                        "--steps", "1", "--warmup", "1", "--dump-outputs", dump], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["value"] > 0 and rec["unit"] == "reads/s" and rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    assert rec["steps"] == 1 and rec["warmup"] == 1
    for key in ("full_pipeline", "full_pipeline_value", "host_handover", "winners_files", "paired_file_to_file"):
        assert rec[key] is None, key
    assert "cpu_baseline" not in rec and "concordance_vs_single_engine" not in rec
    assert all(k["ms_alone"] is None for k in rec["kernels"].values())
    assert rec["dump_outputs"]["reads"] == 20000
    assert np.load(os.path.join(dump, "start.npy")).shape == (20000,)
