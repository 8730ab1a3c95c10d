"""bench.py --dump-outputs, host half (CPU tier): what a run writes for the stream of its last timed step -- float arrays only,
within 64 MB, the same files for the same stream, and a sample that changes when the stream does."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _load(d):
    return {n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_of_a_long_stream_is_a_fixed_sample_within_the_budget(tmp_path):
    stream = np.random.default_rng(5).integers(0, 256, size=(28 << 20) + 12345, dtype=np.uint8).tobytes()
    bench.dump_outputs(str(tmp_path / "a"), stream)
    bench.dump_outputs(str(tmp_path / "b"), stream)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == ["compressed_bytes.npy", "compressed_sample.npy", "compressed_sha256.npy"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in a) <= 64 * 1000 * 1000
    for n in a:
        assert np.array_equal(a[n], b[n])
    assert a["compressed_bytes.npy"].tolist() == [len(stream)]
    assert bytes(a["compressed_sha256.npy"].astype(np.uint8)) == hashlib.sha256(stream).digest()
    assert len(a["compressed_sample.npy"]) == 8 << 20 and a["compressed_sample.npy"].max() <= 255
    changed = bytearray(stream)
    for k in range(0, len(changed), 4096):
        changed[k] ^= 0xFF
    bench.dump_outputs(str(tmp_path / "c"), bytes(changed))
    assert not np.array_equal(_load(str(tmp_path / "c"))["compressed_sample.npy"], a["compressed_sample.npy"])


def test_dump_of_a_short_stream_holds_all_of_it(tmp_path):
    stream = bytes(range(256)) * 7
    bench.dump_outputs(str(tmp_path), stream)
    got = np.load(str(tmp_path / "compressed_sample.npy"))
    assert got.dtype == np.float32 and bytes(got.astype(np.uint8)) == stream
