"""The segment and scatter entry points of the C ABI: exported, bound, and bound with the prototypes include/orz_hip.h declares
(no compute calls here; the refusals below are made before anything reaches a device)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
PZ = ctypes.POINTER(ctypes.c_size_t)
PV = ctypes.POINTER(ctypes.c_void_p)

# name -> (return type, parameter types in the header's words, the ctypes they are bound with)
PROTOTYPES = {
    "orz_members_bound_segments": ("size_t", ["const size_t*", "size_t"], Z, [PZ, Z]),
    "orz_members_encode_segments": (
        "int", ["orz_members*", "const void* const*", "const size_t*", "size_t", "int", "uint8_t**", "size_t*", "size_t*"],
        I, [V, PV, PZ, Z, I, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), PZ, PZ]),
    "orz_members_encode_segments_to_device": (
        "int", ["orz_members*", "const void* const*", "const size_t*", "size_t", "int", "uint8_t*", "size_t", "size_t*", "size_t*"],
        I, [V, PV, PZ, Z, I, V, Z, PZ, PZ]),
    "orz_decode_members_scatter": (
        "int", ["int", "const void*", "size_t", "int", "const size_t*", "const size_t*", "size_t", "uint8_t* const*", "const size_t*", "size_t",
                "size_t*", "size_t*", "orz_decode_stats*"],
        I, [I, V, Z, I, PZ, PZ, Z, PV, PZ, Z, PZ, PZ, None]),
    "orz_decode_members_scatter_host_waits": ("uint64_t", [], ctypes.c_uint64, []),
}


def _header_prototypes():
    text = open(os.path.join(ROOT, "include", "orz_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([a-z0-9_]+\s*\**)\s*(orz_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if p in ("void", ""):
                continue
            p = re.sub(r"\s*\b[a-z_][a-z0-9_]*$", "", p) if not p.endswith("*") else p  # (drop the parameter's name)
            types.append(re.sub(r"\s+", " ", p).replace(" *", "*"))
        out[name] = (ret.strip(), types)
    return out


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
    assert bound["orz_decode_members_scatter"][1][-1] is ctypes.POINTER(_native.DecodeStats)


def test_the_decode_stats_layout_is_what_it_was():
    """host_waits of a scatter call comes through orz_decode_members_scatter_host_waits: orz_decode_stats keeps its six fields"""
    from orz_amd import _native

    text = open(os.path.join(ROOT, "include", "orz_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} orz_decode_stats;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == [k for k, _ in _native.DecodeStats._fields_]
    assert ctypes.sizeof(_native.DecodeStats) == 48


def test_segment_calls_refuse_bad_arguments_before_any_device_work():
    """the bound is the sum of the streams' bounds; a null members object and NULL arrays are ORZ_EINVAL, found on the host"""
    from orz_amd import _native

    lib = _native.load()
    assert lib.orz_members_bound_segments(None, 0) == 0
    lens = (ctypes.c_size_t * 3)(0, 1, 70_000)
    want = sum(lib.orz_stream_bound(n) for n in (0, 1, 70_000))
    assert lib.orz_members_bound_segments(lens, 3) == want
    dst = ctypes.POINTER(ctypes.c_uint8)()
    dlen = ctypes.c_size_t(99)
    assert lib.orz_members_encode_segments(None, None, None, 0, 0, ctypes.byref(dst), ctypes.byref(dlen), None) == -22  # no object
    assert lib.orz_members_encode_segments_to_device(None, None, None, 3, 0, None, 0, None, None) == -22
    assert "null" in _native.last_error()
