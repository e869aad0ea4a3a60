"""bench.py --dump-outputs, the writer itself: dtypes, names, the 64 MB cap with its fixed seeded sample, and --steps
validation (no device needed)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_writes_float_arrays(tmp_path):
    b = _bench()
    s = np.linspace(0, 1, 100, dtype=np.float32)
    c = np.arange(100, dtype=np.int32)
    b.dump_outputs(str(tmp_path), s, c, 42, np.float32(0.75))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["best_index", "best_score", "counts", "scores"]
    assert got["scores"].dtype == np.float32 and np.array_equal(got["scores"], s)
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], c)
    assert got["best_index"].tolist() == [42.0] and got["best_score"].tolist() == [0.75]


def test_dump_samples_large_outputs_under_the_cap(tmp_path):
    b = _bench()
    b.DUMP_LIMIT_BYTES = 1 << 20
    n = 200_000                                       # 200k x (4 + 8) B = 2.4 MB > 1 MB
    s = np.arange(n, dtype=np.float32)
    c = np.arange(n, dtype=np.int32) * 2
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), s, c, 7, np.float32(1.0))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= b.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))     # the same sample every run
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), idx.astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy"), idx * 2)


def test_steps_below_one_is_refused():
    out = subprocess.run([sys.executable, "bench.py", "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr
