"""bench.py --dump-outputs: what it writes, within its size budget, the same from run to run.  CPU only."""
import os

import numpy as np

import bench


def test_small_output_is_written_whole_in_float64(tmp_path):
    x = np.arange(1000, dtype=np.float64) / 3.0
    bench.dump_outputs(str(tmp_path), {"x": x})
    assert sorted(os.listdir(tmp_path)) == ["x.npy"]
    y = np.load(tmp_path / "x.npy")
    assert y.dtype == np.float64 and np.array_equal(y, x)


def test_large_output_is_a_fixed_sample_within_the_budget(tmp_path):
    x = np.random.default_rng(1).standard_normal(10000)
    budget = 8000
    bench.dump_outputs(str(tmp_path / "a"), {"x": x}, budget_bytes=budget)
    bench.dump_outputs(str(tmp_path / "b"), {"x": x}, budget_bytes=budget)
    files = [tmp_path / "a" / f for f in ("x.npy", "x_index.npy")]
    assert sum(np.load(f).nbytes for f in files) <= budget
    idx = np.load(tmp_path / "a" / "x_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), x[idx.astype(np.int64)])
    for f in ("x.npy", "x_index.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    # a later whole dump into the same directory leaves no stale index behind
    bench.dump_outputs(str(tmp_path / "a"), {"x": x[:10]}, budget_bytes=budget)
    assert sorted(os.listdir(tmp_path / "a")) == ["x.npy"]
