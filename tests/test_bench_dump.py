"""bench.py --dump-outputs, its writer alone (no GPU): arrays within the budget are written whole as float32; beyond it every
array keeps the same seeded sample of its indices along its axis, the files stay within the budget, and <name>_index.npy
names the kept indices."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    a = np.random.default_rng(1).uniform(-1, 1, (6, 1000))
    bench.dump_outputs(str(tmp_path), [("outputs", a, 1)])
    got = np.load(tmp_path / "outputs.npy")
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    assert sorted(os.listdir(tmp_path)) == ["outputs.npy"]


def test_large_outputs_are_a_seeded_sample_within_the_budget(tmp_path):
    budget = 400_000
    a = np.random.default_rng(2).uniform(-1, 1, (8, 50_000)).astype(np.float32)  # 1.6 MB
    b = np.random.default_rng(3).uniform(-1, 1, (20_000, 4)).astype(np.float32)
    for run in ("x", "y"):
        bench.dump_outputs(str(tmp_path / run), [("outputs", a, 1), ("gains", b, 0)], budget)
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x")) <= budget
    for name, src, axis in (("outputs", a, 1), ("gains", b, 0)):
        got, idx = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "x" / (name + "_index.npy"))
        assert idx.dtype == np.float64 and len(idx) > 0 and np.all(np.diff(idx) > 0)
        assert np.array_equal(got, np.take(src, idx.astype(np.int64), axis=axis))
        assert np.array_equal(got, np.load(tmp_path / "y" / (name + ".npy")))
