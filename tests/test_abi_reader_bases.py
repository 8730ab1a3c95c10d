"""The C ABI of base-aware reads: orz_reader_set_bases is declared in include/orz_hip.h, exported by the library and bound in
orz_amd/_native.py with the argument types the header states; what it refuses without a reader; and the Python face."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
NEW = ("orz_reader_set_bases", "orz_element_gather_time")


@pytest.fixture(scope="module")
def native():
    from orz_amd import _native

    _native.load()
    return _native


def _ctype(c):
    """the ctypes type of a C parameter or return type as the header writes it"""
    c = re.sub(r"\s+", " ", re.sub(r"\bconst\b", "", c).strip())
    c = re.sub(r" ?\*", "*", c)
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    if c in scalars:
        return scalars[c]
    if c == "void**":  # (an array of addresses)
        return ctypes.POINTER(ctypes.c_void_p)
    if c in ("void*", "orz_reader*"):
        return ctypes.c_void_p
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


def test_the_new_symbol_is_declared_exported_and_bound_as_the_header_states(native):
    protos = _prototypes()
    lib = native.load()
    bound = {n: (r, a) for n, r, a in native.SYMBOLS}
    for name in NEW:
        assert name in protos, name + " is not declared"
        assert hasattr(lib, name), "the library does not export " + name
        assert name in bound, "orz_amd/_native.py does not bind " + name
        ret, params = protos[name]
        assert bound[name][0] is _ctype(ret), name
        want = [_ctype(p) for p in params]
        assert len(bound[name][1]) == len(want), name
        for k, (a, b) in enumerate(zip(bound[name][1], want)):
            assert a is b, "%s: argument %d is bound as %s, the header says %s" % (name, k, a, b)
    # the reader, an array of addresses, their number -- the shape of orz_reader_set_planes with addresses for element sizes
    assert list(bound["orz_reader_set_bases"][1]) == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    assert len(bound["orz_reader_set_bases"][1]) == len(bound["orz_reader_set_planes"][1])


def test_the_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "orz_hip.h")).read()
    for words in ("orz_reader_set_bases:", "orz_reader_read_elements WITH BASES", "IN PLACE", "bases for Y tensors", "wrap the address space",
                  "the same launches and the same host waits"):
        assert words in text, words


def test_no_reader_is_refused_without_a_device(native):
    lib = native.load()
    addrs = (ctypes.c_void_p * 2)(None, None)
    assert lib.orz_reader_set_bases(None, addrs, 2) == EINVAL and native.last_error() == "bad argument"
    assert lib.orz_reader_set_bases(None, None, 0) == EINVAL and native.last_error() == "bad argument"
    # the measuring hook: no planes, a count that is no multiple of 16, an element size that has no planes, no repetitions
    ms = ctypes.c_double()
    at = ctypes.c_void_p(16)
    for planes, count, elem, reps in ((None, 16, 2, 1), (at, 17, 2, 1), (at, 0, 2, 1), (at, 16, 3, 1), (at, 16, 2, 0)):
        assert lib.orz_element_gather_time(0, planes, None, at, count, elem, reps, ctypes.byref(ms)) == EINVAL
        assert native.last_error() == "bad argument"


def test_the_python_face_is_there():
    import orz_amd

    sig = inspect.signature(orz_amd.MemberReader.__init__)
    assert list(sig.parameters)[1:] == ["src", "device", "members", "cache_bytes", "elems", "pieces", "bases"]
    assert sig.parameters["bases"].default is None
    assert list(inspect.signature(orz_amd.MemberReader.set_bases).parameters) == ["self", "bases"]
    for text in (orz_amd.MemberReader.__doc__, orz_amd.MemberReader.set_bases.__doc__, orz_amd.MemberReader.read_tensor.__doc__):
        assert "bases" in text
    assert "beyond the reader" not in orz_amd.MemberReader.__doc__ and "IN PLACE" in orz_amd.MemberReader.read_tensor.__doc__
