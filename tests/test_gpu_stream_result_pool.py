"""GPU tier: where orz_stream_encode's result lives -- page-locked buffers from a small process-wide pool for results of 1 MiB
or more, malloc below that, everything released through orz_free.  Bars: results held at the same time keep their own bytes,
whatever order they are freed in; both paths hand out the bytes orz_stream_encode_to_device leaves in HBM; orz_free still takes
a members result and NULL."""
import ctypes

import numpy as np
import pytest
import torch  # (ahead of the library: the process then has ONE HIP runtime, torch's)

import _data

pytestmark = pytest.mark.gpu


def _dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")


def _hip_runtime():
    """the HIP runtime the library is linked against, as this process has it mapped"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    pytest.fail("no HIP runtime is mapped into the process")


def _page_locked(hip, buf):
    flags = ctypes.c_uint()
    hip.hipHostGetFlags.argtypes = [ctypes.POINTER(ctypes.c_uint), ctypes.c_void_p]
    rc = hip.hipHostGetFlags(ctypes.byref(flags), ctypes.cast(buf._ptr, ctypes.c_void_p))
    hip.hipGetLastError()
    return rc == 0


@pytest.fixture(scope="module")
def enc():
    import orz_amd

    e = orz_amd.StreamEncoder(device=0, level=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """two inputs whose streams exceed 1 MiB (text followed by noise), one whose stream stays far below it"""
    rng = np.random.default_rng(21)
    big = [_data.text(1_500_000, seed=s) + rng.integers(0, 256, 1_300_000 + 100_000 * s, dtype=np.uint8).tobytes() for s in (1, 2)]
    return big, _data.text(600_000, seed=3)


def _in_hbm(enc, data):
    import orz_amd

    src = _dev(data)
    cap = orz_amd.stream_bound(len(data))
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    n = enc.encode_to_device(src.data_ptr(), len(data), dst.data_ptr(), cap)
    return dst[:n].cpu().numpy().tobytes()


def test_results_held_together_keep_their_bytes_in_either_order_of_release(enc, inputs):
    big, _ = inputs
    want = [_in_hbm(enc, d) for d in big]
    assert want[0] != want[1] and min(len(w) for w in want) >= 1 << 20
    srcs = [_dev(d) for d in big]
    for first in (0, 1):
        a = enc.encode_device(srcs[0].data_ptr(), len(big[0]), raw=True)
        b = enc.encode_device(srcs[1].data_ptr(), len(big[1]), raw=True)
        assert ctypes.addressof(a._ptr.contents) != ctypes.addressof(b._ptr.contents)
        assert bytes(a) == want[0] and bytes(b) == want[1]
        (a, b)[first].close()
        assert bytes((a, b)[1 - first]) == want[1 - first]  # the other one is untouched by the release
        (a, b)[1 - first].close()
        c = enc.encode_device(srcs[first].data_ptr(), len(big[first]), raw=True)  # a third call, on buffers that came back
        assert bytes(c) == want[first]
        c.close()
    # a result that outlives two later ones
    a = enc.encode_device(srcs[0].data_ptr(), len(big[0]), raw=True)
    for k in (1, 1):
        assert enc.encode_device(srcs[k].data_ptr(), len(big[k])) == want[k]
    assert bytes(a) == want[0]
    a.close()


def test_small_results_are_malloced_and_large_ones_page_locked(enc, inputs):
    big, small = inputs
    hip = _hip_runtime()
    s = enc.encode_device(_dev(small).data_ptr(), len(small), raw=True)
    assert len(s) < 1 << 20 and not _page_locked(hip, s)
    assert bytes(s) == _in_hbm(enc, small)
    s.close()
    b = enc.encode_device(_dev(big[0]).data_ptr(), len(big[0]), raw=True)
    assert len(b) >= 1 << 20 and _page_locked(hip, b)
    assert bytes(b) == _in_hbm(enc, big[0])
    b.close()
    assert enc.encode(small) == _in_hbm(enc, small)  # host input, the copying wrapper


def test_orz_free_takes_a_members_result_and_null(inputs):
    import orz_amd
    from orz_amd import _native

    _, small = inputs
    lib = _native.load()
    lib.orz_free(None)
    m = orz_amd.MemberEncoder(device=0, level=1, jobs=1)
    try:
        dst = ctypes.POINTER(ctypes.c_uint8)()
        dlen, nm = ctypes.c_size_t(), ctypes.c_size_t()
        buf = ctypes.create_string_buffer(small, len(small))
        rc = lib.orz_members_encode(m._h, ctypes.cast(buf, ctypes.c_void_p), len(small), 0, 1 << 26, ctypes.byref(dst), ctypes.byref(dlen),
                                    ctypes.byref(nm))
        assert rc == 0 and nm.value == 1 and dlen.value > 0
        got = ctypes.string_at(dst, dlen.value)
        lib.orz_free(dst)
        back, n = orz_amd.decode_members(got)
        assert back == small and n == 1
    finally:
        m.close()
