"""The C ABI of planes cut into pieces: the new symbols are declared in include/orz_hip.h, exported by the library and bound in
orz_amd/_native.py with the argument types the header states; and what they answer without a device -- the bound and the member
count, NULL arrays, no segments, no destinations."""
import ctypes
import os
import re

import pytest

import _piececases as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV = 0, -22, -19
NEW = ("orz_members_bound_planes_pieces", "orz_members_encode_planes_pieces_to_device", "orz_decode_members_planes_pieces",
       "orz_decode_members_planes_pieces_host_waits", "orz_reader_set_planes_pieces")


@pytest.fixture(scope="module")
def native():
    from orz_amd import _native

    _native.load()
    return _native


def _ctype(native, c):
    """the ctypes type of a C parameter or return type as the header writes it"""
    c = re.sub(r"\s+", " ", re.sub(r"\bconst\b", "", c).strip())
    c = re.sub(r" ?\*", "*", c)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    if c in scalars:
        return scalars[c]
    if c in ("void**", "uint8_t**"):  # (an array of addresses)
        return ctypes.POINTER(ctypes.c_void_p)
    if c in ("void*", "uint8_t*", "orz_members*", "orz_reader*"):
        return ctypes.c_void_p
    if c == "orz_decode_stats*":
        return ctypes.POINTER(native.DecodeStats)
    assert c.endswith("*") and c[:-1] in scalars, c
    return ctypes.POINTER(scalars[c[:-1]])


def _prototypes():
    text = open(os.path.join(ROOT, "include", "orz_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^([a-z0-9_]+)\s+(orz_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", text, flags=re.M):
        params = [] if args.strip() == "void" else [re.sub(r"\b[a-z_0-9]+$", "", a.strip()) if not a.strip().endswith("*") else a for a in args.split(",")]
        out[name] = (ret, params)
    return out


def test_the_new_symbols_are_declared_exported_and_bound_as_the_header_states(native):
    protos = _prototypes()
    lib = native.load()
    bound = {n: (r, a) for n, r, a in native.SYMBOLS}
    for name in NEW:
        assert name in protos, name + " is not declared"
        assert hasattr(lib, name), "the library does not export " + name
        assert name in bound, "orz_amd/_native.py does not bind " + name
        ret, params = protos[name]
        assert bound[name][0] is _ctype(native, ret), name
        want = [_ctype(native, p) for p in params]
        assert len(bound[name][1]) == len(want), name
        for k, (a, b) in enumerate(zip(bound[name][1], want)):
            assert a is b, "%s: argument %d is bound as %s, the header says %s" % (name, k, a, b)
    # the parser reads the sibling calls the same way
    for name in ("orz_members_encode_planes_to_device", "orz_decode_members_planes", "orz_reader_set_planes", "orz_members_bound_planes"):
        ret, params = protos[name]
        assert [bound[name][0]] + list(bound[name][1]) == [_ctype(native, ret)] + [_ctype(native, p) for p in params], name


def test_the_python_face_is_there():
    import orz_amd

    assert callable(orz_amd.MemberEncoder.encode_tensor_pieces) and callable(orz_amd.MemberEncoder.bound_planes_pieces)
    import inspect

    assert "pieces" in inspect.signature(orz_amd.decode_planes_into).parameters
    assert "pieces" in inspect.signature(orz_amd.MemberReader.__init__).parameters
    assert "pieces" in inspect.signature(orz_amd.MemberReader.set_planes).parameters


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def test_the_bound_and_the_member_count(native):
    lib = native.load()
    nm = ctypes.c_size_t(77)
    assert lib.orz_members_bound_planes_pieces(None, None, 3, 32, ctypes.byref(nm)) == 0 and nm.value == 0
    assert lib.orz_members_bound_planes_pieces(None, None, 0, 32, None) == 0
    lens, elems = [2 * 69, 5, 0, 8 * 64, 4 * 32, 4 * 33], [2, 1, 4, 8, 4, 4]
    for P in (0, 16, 32, 4096):
        got = lib.orz_members_bound_planes_pieces(_arr(ctypes.c_size_t, lens), _arr(ctypes.c_uint32, elems), len(lens), P, ctypes.byref(nm))
        pieces = [[min(P, n // e - q * P) if pp.pieces_of(n // e, P) > 1 else n // e for q in range(pp.pieces_of(n // e, P))] for n, e in zip(lens, elems)]
        assert nm.value == sum(e * len(p) for e, p in zip(elems, pieces)), P
        assert got == sum(e * sum(lib.orz_stream_bound(x) for x in p) for e, p in zip(elems, pieces)), P
    # without pieces: the bound of the planes call
    assert lib.orz_members_bound_planes_pieces(_arr(ctypes.c_size_t, lens), _arr(ctypes.c_uint32, elems), len(lens), 0, None) == \
        lib.orz_members_bound_planes(_arr(ctypes.c_size_t, lens), _arr(ctypes.c_uint32, elems), len(lens))


def test_null_arrays_are_refused_without_a_device(native):
    lib = native.load()
    one = _arr(ctypes.c_uint32, [2])
    cap = _arr(ctypes.c_size_t, [64])
    dst = _arr(ctypes.c_void_p, [None])
    nm = ctypes.c_size_t()
    for elems, pieces in ((None, one), (one, None)):
        assert lib.orz_decode_members_planes_pieces(0, None, 0, 0, None, None, 0, dst, cap, elems, pieces, 1, None, ctypes.byref(nm), None) == EINVAL
        assert "bad argument" in native.last_error() and lib.orz_decode_members_planes_pieces_host_waits() == 0
    assert lib.orz_decode_members_planes_pieces(0, None, 5, 0, None, None, 0, dst, cap, one, one, 1, None, None, None) == EINVAL  # bytes at NULL
    assert lib.orz_decode_members_planes_pieces(0, None, 0, 0, cap, None, 1, dst, cap, one, one, 1, None, None, None) == EINVAL  # half a table
    assert lib.orz_decode_members_planes_pieces(0, None, 0, 0, None, None, 0, dst, None, one, one, 1, None, None, None) == EINVAL  # no capacities
    assert lib.orz_reader_set_planes_pieces(None, one, one, 1) == EINVAL
    # no members object: refused before the segments are looked at, whatever their number
    offs = _arr(ctypes.c_size_t, [0] * 4)
    for n_segs in (0, 1):
        assert lib.orz_members_encode_planes_pieces_to_device(None, None, None, None, n_segs, 32, 1, None, 0, offs, offs, offs) == EINVAL
        assert "null members object" in native.last_error()


def test_no_destinations_and_no_members(native):
    """an empty container and no destinations: nothing to refuse and nothing to decode -- ORZ_OK where a device is, ORZ_ENODEV without one"""
    lib = native.load()
    nm = ctypes.c_size_t(9)
    rc = lib.orz_decode_members_planes_pieces(0, None, 0, 0, None, None, 0, None, None, None, None, 0, None, ctypes.byref(nm), None)
    assert rc == (OK if lib.orz_device_count() > 0 else ENODEV), native.last_error()
    assert nm.value == (0 if rc == OK else 9)
