"""bench.py --dump-outputs (bench.dump_rows) on the CPU: the whole output when it fits the limit, else a fixed, seeded sample of rows
with their indices -- the same files from run to run, so that two builds can be compared output for output."""
import numpy as np
import torch

import bench


def test_dump_rows_writes_the_whole_output_when_it_fits(tmp_path):
    rows = torch.randn(1000, 3, 3)
    paths = bench.dump_rows(str(tmp_path), "rotations", rows)
    assert paths == [str(tmp_path / "rotations.npy")]
    got = np.load(paths[0])
    assert got.dtype == np.float32 and np.array_equal(got, rows.numpy())


def test_dump_rows_samples_a_larger_output_the_same_way_every_time(tmp_path):
    rows = torch.randn(1000, 3, 3)
    limit = 100 * 36
    a = bench.dump_rows(str(tmp_path / "a"), "rotations", rows, limit=limit)
    b = bench.dump_rows(str(tmp_path / "b"), "rotations", rows, limit=limit)
    got, idx = np.load(a[0]), np.load(a[1])
    assert a[1].endswith("rotations_rows.npy") and got.dtype == np.float32 and idx.dtype == np.float64
    assert got.nbytes + idx.nbytes <= limit and len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got, rows.numpy()[idx.astype(np.int64)])
    assert np.array_equal(np.load(b[0]), got) and np.array_equal(np.load(b[1]), idx)
    assert bench.DUMP_BYTES <= 64_000_000
