"""bench.py's plain run (no --full) on the device: the line it prints carries the contract and no side leg, and
--dump-outputs writes the same results of the last timed step from run to run (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for line in (a, b):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "ciphertext-mul/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
        assert line["roofline"]["launches"] > 0
        assert not {"ntt", "cpu_baseline", "other_configs", "configs_multi", "gather", "full_record"} & set(line), sorted(line)
    got = np.load(tmp_path / "a" / "bfv_mul_relin_out.npy")
    idx = np.load(tmp_path / "a" / "bfv_mul_relin_out_coeff_index.npy")
    assert got.dtype == np.float64 and idx.dtype == np.float64
    assert got.shape == (8, 2, 8, 1 << 14) and np.array_equal(idx, np.arange(1 << 14))   # a batch of 8 fits whole
    assert np.all(got == np.floor(got)) and got.min() >= 0 and got.max() < 2.0**51 and np.unique(got[:, :, 0]).size > 1000
    assert np.array_equal(got, np.load(tmp_path / "b" / "bfv_mul_relin_out.npy"))
