"""bench.py without --full: the headline steps and their line, nothing else measured."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu

CONTRACT = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "conv_all", "per_kernel", "train_bf16", "inference", "augment", "cpu_baseline"}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plain_run_prints_the_headline_only(cuda, tmp_path, dtype):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dtype", dtype, "--dump-outputs", str(tmp_path)],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    assert CONTRACT <= out.keys()
    assert not FULL_ONLY & out.keys()
    assert out["metric"] == "224x224 images/sec train" and out["unit"] == "images/sec"
    assert out["higher_is_better"] is True and out["dtype"] == dtype
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 256) < 1.0   # one GPU, 256 images per step
    for name in ("probs", "loss", "params"):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.size and np.isfinite(a).all(), name
