"""bench.py's command line and its --dump-outputs writer (CPU only: no step is run)."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_writes_every_array_as_float64(tmp_path):
    lf = np.linspace(-3.0, 3.0, 12).reshape(4, 3)
    info = np.array([0, 1, 0, 2], dtype=np.int32)
    shapes = bench.dump_outputs(str(tmp_path), {"logml_full": lf, "info": info, "mu": None,
                                                "ess": 7.5})
    assert shapes == {"logml_full": [4, 3], "info": [4], "ess": []}
    assert sorted(os.listdir(tmp_path)) == ["ess.npy", "info.npy", "logml_full.npy"]
    got = np.load(tmp_path / "logml_full.npy")
    assert got.dtype == np.float64 and np.array_equal(got, lf)
    assert np.array_equal(np.load(tmp_path / "info.npy"), info.astype(np.float64))
    assert float(np.load(tmp_path / "ess.npy")) == 7.5


def test_dump_above_the_budget_keeps_the_same_seeded_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    rng = np.random.default_rng(3)
    arrays = {"sigma": rng.standard_normal((4000, 3, 3)), "logml_full": rng.standard_normal(4000)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BUDGET_BYTES
    rows = np.load(tmp_path / "a" / "sigma_rows.npy").astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / "a" / "logml_full_rows.npy"))
    assert 0 < rows.size < 4000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "sigma.npy"), arrays["sigma"][rows])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
