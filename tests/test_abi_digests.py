"""The C ABI of the digests: the new symbols are declared in include/orz_hip.h, exported by the library and bound in
orz_amd/_native.py with the argument types the header states (the parser of test_abi_pieces.py); what they answer without a
device -- host digests against zlib, the combine, the NULL refusals --; and the Python face."""
import ctypes
import inspect
import zlib

import pytest

import _crccases as cc
import test_abi_pieces as ap

OK, EINVAL, ENODEV, EBADMSG = 0, -22, -19, -74
NEW = ("orz_crc32_buffers", "orz_crc32_combine", "orz_decode_tensors_verified", "orz_decode_tensors_verified_host_waits")


@pytest.fixture(scope="module")
def native():
    from orz_amd import _native

    _native.load()
    return _native


def test_the_new_symbols_are_declared_exported_and_bound_as_the_header_states(native):
    protos = ap._prototypes()
    lib = native.load()
    bound = {n: (r, a) for n, r, a in native.SYMBOLS}
    for name in NEW:
        assert name in protos, name + " is not declared"
        assert hasattr(lib, name), "the library does not export " + name
        assert name in bound, "orz_amd/_native.py does not bind " + name
        ret, params = protos[name]
        assert bound[name][0] is ap._ctype(native, ret), name
        want = [ap._ctype(native, p) for p in params]
        assert len(bound[name][1]) == len(want), name
        for k, (a, b) in enumerate(zip(bound[name][1], want)):
            assert a is b, "%s: argument %d is bound as %s, the header says %s" % (name, k, a, b)
    assert len(protos["orz_decode_tensors_verified"][1]) == len(protos["orz_decode_members_planes_pieces"][1]) + 2
    text = open(ap.os.path.join(ap.ROOT, "include", "orz_hip.h")).read()
    assert ap.re.search(r"^#define ORZ_EBADMSG \(-74\)", text, flags=ap.re.M)


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def _host_crcs(lib, datas, device=0):
    keep = [ctypes.create_string_buffer(d, max(len(d), 1)) for d in datas]
    bufs = _arr(ctypes.c_void_p, [ctypes.addressof(k) if d else None for k, d in zip(keep, datas)])
    crcs = _arr(ctypes.c_uint32, [0xDEADBEEF] * len(datas))
    rc = lib.orz_crc32_buffers(device, bufs, _arr(ctypes.c_size_t, [len(d) for d in datas]), len(datas), 0, crcs)
    return rc, list(crcs[:len(datas)])


def test_host_buffers_need_no_device(native):
    lib = native.load()
    datas = [d for d, _ in cc.buffers() if len(d) <= 2000] + [cc._random(70001, 3)]
    rc, got = _host_crcs(lib, datas, device=12345)  # (no such device: nobody asks)
    assert rc == OK, native.last_error()
    assert got == [zlib.crc32(d) for d in datas] and got[datas.index(b"")] == 0
    assert lib.orz_crc32_buffers(0, None, None, 0, 0, None) == OK and lib.orz_crc32_buffers(0, None, None, 0, 1, None) == OK


def test_null_arrays_and_null_buffers_are_refused_before_the_device(native):
    lib = native.load()
    one, ln, crc = _arr(ctypes.c_void_p, [None]), _arr(ctypes.c_size_t, [4]), _arr(ctypes.c_uint32, [7])
    for on_device in (0, 1):
        for bufs, lens, crcs in ((None, ln, crc), (one, None, crc), (one, ln, None)):
            assert lib.orz_crc32_buffers(0, bufs, lens, 1, on_device, crcs) == EINVAL and "bad argument" in native.last_error()
        assert lib.orz_crc32_buffers(0, one, ln, 1, on_device, crc) == EINVAL and "buffer 0 is NULL and has bytes" in native.last_error()
    assert crc[0] == 7
    # a NULL buffer of no bytes is a buffer of no bytes
    assert lib.orz_crc32_buffers(0, one, _arr(ctypes.c_size_t, [0]), 1, 0, crc) == OK and crc[0] == 0


@pytest.mark.parametrize("len_b", (0, 1, 77, (1 << 29) - 1, 1 << 29, (1 << 32) + 5, 1 << 40))
def test_combine(native, len_b):
    lib = native.load()
    a, b = 0xCBF43926, 0x1C291CA3
    assert lib.orz_crc32_combine(a, b, len_b) == cc.np_combine(a, b, len_b)
    if len_b <= 77:
        x, y = cc._random(100, 1), cc._random(len_b, 2)
        assert lib.orz_crc32_combine(zlib.crc32(x), zlib.crc32(y), len_b) == zlib.crc32(x + y)


def test_the_verified_decode_refuses_null_arrays_without_a_device(native):
    lib = native.load()
    one = _arr(ctypes.c_uint32, [2])
    cap = _arr(ctypes.c_size_t, [64])
    dst = _arr(ctypes.c_void_p, [None])
    nm = ctypes.c_size_t()
    call = lib.orz_decode_tensors_verified
    assert call(0, None, 0, 0, None, None, 0, dst, cap, one, one, 1, None, None, None, ctypes.byref(nm), None) == EINVAL  # no digests
    assert "bad argument" in native.last_error() and lib.orz_decode_tensors_verified_host_waits() == 0
    assert call(0, None, 0, 0, None, None, 0, dst, None, one, one, 1, one, None, None, None, None) == EINVAL  # no capacities
    assert call(0, None, 5, 0, None, None, 0, dst, cap, one, one, 1, one, None, None, None, None) == EINVAL  # bytes at NULL
    assert call(0, None, 0, 0, cap, None, 1, dst, cap, one, one, 1, one, None, None, None, None) == EINVAL  # half a table
    # a sizing call ignores the digests; no elems and no pieces are layouts, not errors: nothing left to refuse without a device
    rc = call(0, None, 0, 0, None, None, 0, None, None, None, None, 0, None, None, None, ctypes.byref(nm), None)
    assert rc == (OK if lib.orz_device_count() > 0 else ENODEV), native.last_error()


def test_the_python_face_is_there():
    import orz_amd

    for name in ("encode_tensors", "encode_tensor_planes", "encode_tensor_pieces"):
        p = inspect.signature(getattr(orz_amd.MemberEncoder, name)).parameters
        assert p["digests"].default is False, name
    for f in (orz_amd.decode_members_into, orz_amd.decode_planes_into):
        assert inspect.signature(f).parameters["digests"].default is None
    assert inspect.signature(orz_amd.MemberReader.read_tensor).parameters["digest"].default is None
    assert "digest" not in inspect.signature(orz_amd.MemberReader.read_elements).parameters
    assert "nverified" in orz_amd.MemberReader.read_elements.__doc__
    assert list(inspect.signature(orz_amd.crc32_buffers).parameters) == ["tensors", "device"]
    assert list(inspect.signature(orz_amd.crc32_combine).parameters) == ["a", "b", "len_b"]
    assert issubclass(orz_amd.OrzDigestError, orz_amd.OrzError)
    e = orz_amd.OrzDigestError("text", 3, 0x11, 0x22)
    assert (e.tensor, e.expected, e.computed, str(e)) == (3, 0x11, 0x22, "text")


def test_python_digests_of_cpu_tensors_and_combine():
    import orz_amd
    import torch

    datas = [cc._random(n, n) for n in (0, 1, 4097)]
    ts = [torch.frombuffer(bytearray(d), dtype=torch.uint8) if d else torch.empty(0, dtype=torch.uint8) for d in datas]
    ts.append(torch.arange(1000, dtype=torch.int32))
    want = [zlib.crc32(t.numpy().tobytes()) for t in ts]
    assert orz_amd.crc32_buffers(ts) == want and orz_amd.crc32_buffers([]) == []
    assert orz_amd.crc32_combine(want[1], want[2], 4097) == zlib.crc32(datas[1] + datas[2])
    with pytest.raises(ValueError):
        orz_amd.crc32_buffers([torch.arange(10)[::2]])
    with pytest.raises(ValueError):
        orz_amd.crc32_combine(1 << 32, 0, 0)
