"""bench.py on the GPU: two runs with the same arguments dump the same outputs (up to the rounding of the backward's
fp32-atomic sums), also after a chain of steps whose weights would amplify that rounding."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_dump(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return {n: np.load(os.path.join(out_dir, n + ".npy")).astype(np.float64) for n in ("loss", "y_pred", "weights")}


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(cuda, tmp_path):
    a, b = _bench_dump(tmp_path / "a"), _bench_dump(tmp_path / "b")
    assert np.isfinite(a["loss"]).all() and np.isfinite(a["y_pred"]).all() and np.isfinite(a["weights"]).all()
    for name in ("loss", "y_pred", "weights"):
        rel = np.linalg.norm(a[name] - b[name]) / np.linalg.norm(a[name])
        assert rel <= 1e-6, (name, rel)
