"""bench.py --dump-outputs (dump_outputs): what it writes for buffers small and large -- float32 kept, integers as
float64 without loss, one seeded ascending row sample shared by every buffer once the whole would pass DUMP_BYTES,
the same from call to call. Host stand-ins for the device buffers; only the last test, of the row download, needs a GPU."""
import os

import numpy as np
import pytest

import bench


class HostBuffer:
    """The part of DeviceBuffer dump_outputs uses."""

    def __init__(self, a):
        self.a, self.shape, self.dtype = a, a.shape, a.dtype

    def download_rows(self, rows):
        return self.a[rows]


def _bufs(n, k, seed=1):
    rng = np.random.default_rng(seed)
    return [("dists", HostBuffer(rng.random((n, k), dtype=np.float32))),
            ("ids", HostBuffer(rng.integers(0, 50_000_000, (n, k)).astype(np.uint64))),
            ("labels", HostBuffer(rng.integers(0, 1 << 40, (n, k)))),
            ("status", HostBuffer(np.full(n, k, np.int32)))]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(tmp_path):
    bufs = _bufs(37, 5)
    bench.dump_outputs(str(tmp_path / "o"), bufs)
    got = _load(tmp_path / "o")
    assert sorted(got) == ["dists", "ids", "labels", "rows", "status"]
    assert np.array_equal(got["rows"], np.arange(37)) and got["rows"].dtype == np.float64
    assert got["dists"].dtype == np.float32 and np.array_equal(got["dists"], bufs[0][1].a)
    for name, b in bufs[1:]:
        assert got[name].dtype == np.float64 and got[name].shape == b.a.shape
        assert np.array_equal(got[name].astype(b.a.dtype), b.a), name


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    n, k = 4099, 7  # row: 8 + 7 * (4 + 8 + 8) + 8 = 156 B -> 420 of the 4099 rows
    bufs = _bufs(n, k)
    bench.dump_outputs(str(tmp_path / "a"), bufs)
    bench.dump_outputs(str(tmp_path / "b"), bufs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["rows"].astype(np.int64)
    assert len(rows) == (1 << 16) // 156 and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < n
    assert sum(v.nbytes for v in a.values()) <= 1 << 16
    for name, buf in bufs:
        assert np.array_equal(a[name], b[name]), name
        assert np.array_equal(a[name].astype(buf.a.dtype), buf.a[rows]), name
    assert np.array_equal(a["rows"], b["rows"])


def test_default_budget_is_under_64_mb():
    assert bench.DUMP_BYTES <= 60 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1000,), (1000, 7), (3, 5)])
def test_device_buffer_download_rows(shape):
    """DeviceBuffer.download_rows (what dump_outputs reads with) against a whole download: chunks smaller than the
    buffer, a chunk with no wanted row, the first and the last row, and a buffer smaller than one chunk."""
    from deepreadmapper_amd.device import DeviceBuffer
    a = np.random.default_rng(3).integers(0, 1 << 40, shape)
    b = DeviceBuffer.from_host(a)
    n = shape[0]
    rows = np.unique(np.r_[0, n - 1, np.arange(n)[n // 2:n // 2 + 130:3]])  # nothing in [1, n // 2)
    for chunk in (64, 256, 1 << 16):
        assert np.array_equal(b.download_rows(rows, chunk), a[rows]), chunk
    assert np.array_equal(b.download_rows(np.arange(n), 64), b.download())
    assert b.download_rows(np.empty(0, np.int64)).shape == (0,) + shape[1:]
    b.free()
