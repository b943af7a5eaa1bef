"""bench.py's --dump-outputs on the host: which rows of y it writes and in what form (no GPU: y is a host tensor here)."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_a_fixed_sample_of_rows(tmp_path):
    n = 5000
    y = torch.arange(n, dtype=torch.float64) * 0.5 - 7.0
    bench.dump_outputs(str(tmp_path / "a"), y, 0, n, cap=1000)
    bench.dump_outputs(str(tmp_path / "b"), y, 0, n, cap=1000)
    vals, rows = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "a" / "y_rows.npy")
    assert vals.dtype == np.float64 and rows.dtype == np.float64 and len(rows) == 1000
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(vals, y.numpy()[rows.astype(np.int64)])
    # the same rows in every run
    assert np.array_equal(rows, np.load(tmp_path / "b" / "y_rows.npy")) and np.array_equal(vals, np.load(tmp_path / "b" / "y.npy"))


def test_dump_outputs_writes_every_row_that_fits(tmp_path):
    y = torch.linspace(-1.0, 1.0, 300, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), y, 0, 300, cap=300)
    assert np.array_equal(np.load(tmp_path / "y_rows.npy"), np.arange(300)) and np.array_equal(np.load(tmp_path / "y.npy"), y.numpy())


def test_dump_outputs_fits_the_budget_at_the_benchmark_size():
    # values + row numbers, 8 bytes each, at most 64 MB
    assert 2 * 8 * bench.DUMP_ROWS <= 64e6
