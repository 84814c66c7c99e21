"""CPU test of bench.py's --dump-outputs writer: every record field as a float64 .npy, all files together within 64 MB,
and beyond that a fixed seeded sample of the cells whose indices are written next to them."""
import os

import numpy as np

import bench
from popscle_amd import muxgl


def _records(dtype, n):
    r = np.zeros(n, dtype=dtype)
    for name in dtype.names:
        r[name] = np.arange(n) % 1000 + (0.25 if r[name].dtype == np.float64 else 0)
    return r


def _dump(path, records, extra=None):
    bench.dump_outputs(str(path), records, extra)
    files = sorted(os.listdir(path))
    assert sum(os.path.getsize(path / f) for f in files) <= bench.DUMP_MAX_BYTES
    return files, {f[:-4]: np.load(path / f) for f in files}


def test_small_output_is_written_whole(tmp_path):
    r = _records(muxgl.DEMUX_CELL, 10_000)
    files, got = _dump(tmp_path, r)
    assert files == sorted(n + ".npy" for n in muxgl.DEMUX_CELL.names)
    for name in muxgl.DEMUX_CELL.names:
        assert got[name].dtype == np.float64 and np.array_equal(got[name], r[name].astype(np.float64)), name


def test_large_output_is_a_fixed_sample(tmp_path):
    r = _records(muxgl.FMX_CELL, 500_000)   # 24 fields x 500 k cells x 8 bytes = 96 MB whole
    extra = {"em_counters": np.array([1.0, 2.0, 3.0])}
    files, a = _dump(tmp_path / "a", r, extra)
    _, b = _dump(tmp_path / "b", r, extra)
    assert set(files) == {n + ".npy" for n in muxgl.FMX_CELL.names} | {"cell_index.npy", "em_counters.npy"}
    idx = a["cell_index"].astype(np.int64)
    assert np.array_equal(a["cell_index"], b["cell_index"]) and np.all(np.diff(idx) > 0) and idx.size > r.size // 2
    assert np.array_equal(a["em_counters"], extra["em_counters"])
    for name in muxgl.FMX_CELL.names:
        assert np.array_equal(a[name], r[name][idx].astype(np.float64)), name
