"""The C ABI of the delta layout: the new symbols are declared in include/orz_hip.h, exported by the library and bound in
orz_amd/_native.py with the argument types the header states; and what they refuse before anything reaches a device -- NULL arrays,
bytes at NULL, half a member table -- and answer for no segments and no destinations."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENODEV = 0, -22, -19
NEW = ("orz_members_encode_deltas_to_device", "orz_decode_tensors_delta", "orz_decode_tensors_delta_host_waits", "orz_plane_delta_move_time")


@pytest.fixture(scope="module")
def native():
    from orz_amd import _native

    _native.load()
    return _native


def _ctype(native, c):
    """the ctypes type of a C parameter or return type as the header writes it"""
    c = re.sub(r"\s+", " ", re.sub(r"\bconst\b", "", c).strip())
    c = re.sub(r" ?\*", "*", c)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    if c in scalars:
        return scalars[c]
    if c in ("void**", "uint8_t**"):  # (an array of addresses)
        return ctypes.POINTER(ctypes.c_void_p)
    if c in ("void*", "uint8_t*", "orz_members*"):
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
    # the delta calls are their siblings with one more array of addresses
    enc, pieces = list(bound["orz_members_encode_deltas_to_device"][1]), list(bound["orz_members_encode_planes_pieces_to_device"][1])
    assert enc[:2] + enc[3:] == pieces and enc[2] is ctypes.POINTER(ctypes.c_void_p)
    dec, verified = list(bound["orz_decode_tensors_delta"][1]), list(bound["orz_decode_tensors_verified"][1])
    assert dec[:9] + dec[10:] == verified and dec[9] is ctypes.POINTER(ctypes.c_void_p)


def test_the_python_face_is_there():
    import inspect

    import orz_amd

    sig = inspect.signature(orz_amd.MemberEncoder.encode_tensor_deltas)
    assert list(sig.parameters)[1:] == ["tensors", "bases", "piece_elems", "out", "digests"]
    assert sig.parameters["piece_elems"].default == 0 and sig.parameters["digests"].default is False
    assert inspect.signature(orz_amd.decode_planes_into).parameters["bases"].default is None
    for text in (orz_amd.MemberEncoder.encode_tensor_deltas.__doc__, orz_amd.MemberReader.__doc__):
        assert "MemberReader" in text or "reader" in text
        assert "DELTA" in text and "digest=" in text  # what a reader returns of a delta container, and that digest= raises


def _arr(ctype, values):
    return (ctype * max(len(values), 1))(*values)


def test_the_decode_refuses_null_arrays_without_a_device(native):
    lib = native.load()
    one = _arr(ctypes.c_uint32, [2])
    cap = _arr(ctypes.c_size_t, [64])
    dst = _arr(ctypes.c_void_p, [None])
    nm = ctypes.c_size_t()

    def call(src_n=0, offs=None, lens=None, n_table=0, dsts=dst, caps=cap, bases=dst, elems=one, pieces=one, n_dsts=1, crcs=None):
        rc = lib.orz_decode_tensors_delta(0, None, src_n, 0, offs, lens, n_table, dsts, caps, bases, elems, pieces, n_dsts, crcs, None, None,
                                          ctypes.byref(nm), None)
        return rc, native.last_error(), lib.orz_decode_tensors_delta_host_waits()

    assert call(bases=None) == (EINVAL, "bad argument", 0)  # a NULL d_bases with n_dsts > 0
    assert call(bases=None, dsts=None) == (EINVAL, "bad argument", 0)  # ... in a sizing call too
    assert call(src_n=5)[:2] == (EINVAL, "bad argument")  # bytes at NULL
    assert call(offs=cap, n_table=1)[:2] == (EINVAL, "bad argument")  # half a table
    assert call(caps=None)[:2] == (EINVAL, "bad argument")  # no capacities
    # crcs, elems and pieces are optional: with them NULL the call gets past the argument check, to the device
    rc, err, _ = call(crcs=None, elems=None, pieces=None, n_dsts=0, bases=None, dsts=None, caps=None)
    assert rc == (OK if lib.orz_device_count() > 0 else ENODEV), err


def test_the_encode_refuses_null_arrays_without_a_device(native):
    lib = native.load()
    offs = _arr(ctypes.c_size_t, [0] * 4)
    ptrs = _arr(ctypes.c_void_p, [None])
    lens = _arr(ctypes.c_size_t, [0])
    el = _arr(ctypes.c_uint32, [2])
    # a NULL seg_base, or a NULL pieces_out, with segments: refused before the members object is looked at
    assert lib.orz_members_encode_deltas_to_device(None, ptrs, None, lens, el, 1, 32, 1, None, 0, offs, offs, offs) == EINVAL
    assert "bad argument" in native.last_error()
    assert lib.orz_members_encode_deltas_to_device(None, ptrs, ptrs, lens, el, 1, 32, 1, None, 0, offs, offs, None) == EINVAL
    assert "bad argument" in native.last_error()
    # no members object: what the pieces call answers, whatever the number of segments
    for n_segs in (0, 1):
        assert lib.orz_members_encode_deltas_to_device(None, ptrs, ptrs, lens, el, n_segs, 32, 1, None, 0, offs, offs, offs) == EINVAL
        assert "null members object" in native.last_error()
    ms = ctypes.c_double()
    assert lib.orz_plane_delta_move_time(0, ctypes.c_void_p(16), None, ctypes.c_void_p(16), 16, 2, 0, 1, ctypes.byref(ms)) == EINVAL  # no base
    assert lib.orz_plane_delta_move_time(0, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 16, 3, 0, 1, ctypes.byref(ms)) == EINVAL
