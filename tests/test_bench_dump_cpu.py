"""bench.py --dump-outputs without a GPU: float64 files, the size budget, and a sample of a large output that is the same
rows, in order, on every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_the_budget_and_a_fixed_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    n = 1_000_000                                           # 112 MB of MFCC rows: over the budget
    mfcc = np.random.default_rng(5).standard_normal((n, 14))
    mfcc[:, 0] = np.arange(n)                               # the row's index, to find it again
    outputs = {"mfcc": mfcc, "frame_offset": np.arange(101, dtype=np.int64) * 10000, "buf_status": np.zeros(100, np.int32)}
    bench.dump_outputs(outputs, str(tmp_path / "a"))
    bench.dump_outputs(outputs, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["buf_status.npy", "frame_offset.npy", "mfcc.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b)
    got = np.load(tmp_path / "a" / "mfcc.npy")
    rows = got[:, 0].astype(np.int64)
    assert got.shape[1] == 14 and got.shape[0] > n // 4 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(got, mfcc[rows])


def test_dump_outputs_writes_a_small_output_whole(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    mfcc = np.random.default_rng(6).standard_normal((1000, 14))
    bench.dump_outputs({"mfcc": mfcc, "frame_offset": np.array([0, 1000])}, str(tmp_path))
    np.testing.assert_array_equal(np.load(tmp_path / "mfcc.npy"), mfcc)
    np.testing.assert_array_equal(np.load(tmp_path / "frame_offset.npy"), [0.0, 1000.0])
