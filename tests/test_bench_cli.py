"""bench.py command-line contract on CPU (llama-tiny): --steps sets the
number of timed steps, the result line carries ms_per_step, and
--dump-outputs writes reproducible arrays of the last timed step."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


def _bench(*extra):
    r = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--device", "cpu",
         "--model", "llama-tiny", "--batch", "2", "--seq-len", "64", "--h", "3",
         "--steps", "3", "--warmup", "1", *extra],
        cwd=REPO, capture_output=True, text=True, timeout=240,
    )
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_reproducible_and_full_flag(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"), "--full")
    for out in (a, b):
        assert out["steps"] == 3 and out["warmup"] == 1
        assert out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "tokens/s" and out["higher_is_better"] is True
        assert out["dtype"] == "fp32"
        # value and ms_per_step describe the same 3 timed steps
        tokens = 2 * 64 * 3
        assert abs(out["value"] * out["ms_per_step"] * 3 / 1000.0 - tokens) < 1e-6 * tokens

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["loss.npy", "params.npy"]
    total = 0
    for name in names:
        x = np.load(tmp_path / "a" / name)
        y = np.load(tmp_path / "b" / name)
        assert x.dtype in (np.float32, np.float64)
        assert np.isfinite(x).all()
        total += x.nbytes
        # same arguments -> same inputs -> same outputs (CPU path is deterministic)
        np.testing.assert_array_equal(x, y)
    assert total <= 64 * 1024 * 1024
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.shape == (1,) and loss[0] == a["config"]["last_loss"]
    params = np.load(tmp_path / "a" / "params.npy")
    assert params.size == min(a["config"]["model_params"], 1 << 22)
