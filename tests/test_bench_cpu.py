"""bench.py without a GPU: the --dump-outputs writer (size bound, seeded sample, dtypes) and the argument checks."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fake:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_dump_bound_fits_64_mb():
    assert 4 * sum(bench.DUMP_MAX_ELEMENTS.values()) + 1024 <= 64e6


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", {"y_pred": 4 * 10 * 33, "weights": 1000})
    g = torch.Generator().manual_seed(0)
    y_pred = torch.randn(4, 10, 33, generator=g)
    flat = torch.randn(5000, generator=g)
    plan, model = _Fake(outputs=[_Fake(buf=y_pred)]), _Fake(flat_all=flat)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, plan, 12.5)
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy", "weights.npy", "y_pred.npy"]
    loss, yp, w = (np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "y_pred", "weights"))
    assert loss.dtype == np.float64 and loss.tolist() == [12.5]
    assert yp.dtype == np.float32 and np.array_equal(yp, y_pred.numpy())          # within its bound: whole
    assert w.dtype == np.float32 and w.shape == (1000,)                            # above it: a sample ...
    assert np.array_equal(w, np.load(tmp_path / "b" / "weights.npy"))             # ... the same one every run
    assert np.isin(w, flat.numpy()).all() and len(np.unique(w)) == 1000


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
