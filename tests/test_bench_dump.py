"""CPU test of bench.py --dump-outputs: the files, their dtypes, and the fixed seeded sample above the size limit."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gl_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench()
    rng = np.random.default_rng(3)
    dist = rng.random(1000).astype(np.float32)
    idx = rng.integers(0, 100000, 1000).astype(np.int64)
    bench.dump_outputs(str(tmp_path / "whole"), dist, idx)
    assert sorted(os.listdir(tmp_path / "whole")) == ["dist.npy", "idx.npy"]
    d, i = np.load(tmp_path / "whole" / "dist.npy"), np.load(tmp_path / "whole" / "idx.npy")
    assert d.dtype == np.float32 and i.dtype == np.float64 and np.array_equal(d, dist) and np.array_equal(i, idx)

    monkeypatch.setattr(bench, "DUMP_BYTES", 2000)                       # 100 of the 1000 queries
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), dist, idx)
    q = np.load(tmp_path / "a" / "query.npy")
    assert q.dtype == np.float64 and len(q) == 100 and np.all(np.diff(q) > 0)
    sel = q.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "dist.npy"), dist[sel]) and np.array_equal(np.load(tmp_path / "a" / "idx.npy"), idx[sel])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2000 + 3 * 128                                       # data within the limit, plus the three .npy headers
    for f in ("query.npy", "dist.npy", "idx.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
