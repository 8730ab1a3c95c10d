"""The element-range entry points of the C ABI: exported, bound, and bound with the prototypes include/orz_hip.h declares (no
compute calls here; the refusals below are made before anything reaches a device)."""
import ctypes

from test_abi_segments import _header_prototypes

V, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
P64, P32 = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)

# name -> (return type, parameter types in the header's words, the ctypes they are bound with)
PROTOTYPES = {
    "orz_reader_set_planes": ("int", ["orz_reader*", "const uint32_t*", "size_t"], I, [V, P32, Z]),
    "orz_reader_tensor_info": ("int", ["orz_reader*", "uint64_t*", "uint64_t*", "uint32_t*", "size_t"], I, [V, P64, P64, P32, Z]),
    "orz_reader_read_elements": (
        "int", ["orz_reader*", "const uint64_t*", "const uint64_t*", "const uint64_t*", "size_t", "uint8_t*", "size_t", "uint64_t*", "orz_read_stats*"],
        I, [V, P64, P64, P64, Z, V, Z, P64, None]),
}


def test_header_declares_the_prototypes_of_the_issue():
    declared = _header_prototypes()
    for name, (ret, params, _, _) in PROTOTYPES.items():
        assert name in declared, name
        assert declared[name] == (ret, params), (name, declared[name])


def test_symbols_resolve_and_are_bound_with_those_prototypes():
    from orz_amd import _native

    lib = _native.load()
    bound = {n: (r, a) for n, r, a in _native.SYMBOLS}
    for name, (_, _, restype, argtypes) in PROTOTYPES.items():
        assert hasattr(lib, name), "liborz_hip.so does not export " + name
        assert name in bound, "orz_amd/_native.py does not bind " + name
        r, a = bound[name]
        assert r is restype, name
        assert len(a) == len(argtypes), name
        for got, want in zip(a, argtypes):
            assert want is None or got is want, (name, got, want)
    assert bound["orz_reader_read_elements"][1][-1] is ctypes.POINTER(_native.ReadStats)


def test_the_stats_layouts_are_what_they_were():
    """the new calls report through orz_read_stats and orz_cache_stats as they are: nine and eight fields of eight bytes"""
    from orz_amd import _native

    assert [k for k, _ in _native.ReadStats._fields_] == ["ranges", "members_decoded", "decoded_bytes", "out_bytes", "launches", "host_waits",
                                                          "kernel_ms", "gather_ms", "total_s"]
    assert ctypes.sizeof(_native.ReadStats) == 72 and ctypes.sizeof(_native.CacheStats) == 64 and ctypes.sizeof(_native.DecodeStats) == 48


def test_a_null_reader_is_refused_before_any_device_work():
    from orz_amd import _native

    lib = _native.load()
    n, dlen = ctypes.c_uint64(7), ctypes.c_uint64(99)
    elems = (ctypes.c_uint32 * 2)(2, 4)
    cols = (ctypes.c_uint64 * 1)(0)
    assert lib.orz_reader_set_planes(None, elems, 2) == -22
    assert lib.orz_reader_tensor_info(None, ctypes.byref(n), None, None, 0) == -22 and n.value == 7
    assert lib.orz_reader_read_elements(None, cols, cols, cols, 1, None, 0, ctypes.byref(dlen), None) == -22
    assert "bad argument" in _native.last_error()
