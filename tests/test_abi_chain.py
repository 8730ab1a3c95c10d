"""The C ABI of the chain decode: the new symbols are declared in include/orz_hip.h, exported by the library and bound in
orz_amd/_native.py with the argument types the header states; and what they refuse before anything reaches a device -- no links,
bytes at NULL, half a member table, no capacities -- and answer for no destinations."""
import ctypes
import inspect

import pytest

from test_abi_delta import _arr, _ctype, _prototypes

OK, EINVAL, ENODEV = 0, -22, -19
NEW = ("orz_decode_tensors_chain", "orz_decode_tensors_chain_host_waits", "orz_plane_chain_move_time")


@pytest.fixture(scope="module")
def native():
    from orz_amd import _native

    _native.load()
    return _native


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
    # the chain call is the delta call with the number of links behind the digests
    chain, delta = list(bound["orz_decode_tensors_chain"][1]), list(bound["orz_decode_tensors_delta"][1])
    assert chain[:14] + chain[15:] == delta and chain[14] is ctypes.c_uint32
    # the hook is the delta hook with the number of links where that one has the direction
    hook, dhook = list(bound["orz_plane_chain_move_time"][1]), list(bound["orz_plane_delta_move_time"][1])
    assert hook[:6] + hook[7:] == dhook[:6] + dhook[7:] and hook[6] is ctypes.c_uint32


def test_the_python_face_is_there():
    import orz_amd

    assert inspect.signature(orz_amd.decode_planes_into).parameters["links"].default is None
    assert list(inspect.signature(orz_amd.join_links).parameters) == ["links"]
    for text in (orz_amd.MemberEncoder.encode_tensor_deltas.__doc__, orz_amd.decode_planes_into.__doc__):
        assert "order of the links does not matter" in " ".join(text.split())
        assert "staging memory" in " ".join(text.split()) and "still sees single links" in " ".join(text.split())


def test_the_decode_refuses_before_anything_reaches_a_device(native):
    lib = native.load()
    one = _arr(ctypes.c_uint32, [2])
    cap = _arr(ctypes.c_size_t, [64])
    dst = _arr(ctypes.c_void_p, [None])
    nm = ctypes.c_size_t()

    def call(src_n=0, offs=None, lens=None, n_table=0, dsts=dst, caps=cap, bases=dst, elems=one, pieces=one, n_dsts=1, crcs=None, links=2):
        rc = lib.orz_decode_tensors_chain(0, None, src_n, 0, offs, lens, n_table, dsts, caps, bases, elems, pieces, n_dsts, crcs, links, None, None,
                                          ctypes.byref(nm), None)
        return rc, native.last_error(), lib.orz_decode_tensors_chain_host_waits()

    assert call(links=0) == (EINVAL, "invalid argument: a chain of 0 links", 0)
    assert call(links=0, dsts=None, bases=None) == (EINVAL, "invalid argument: a chain of 0 links", 0)  # ... in a sizing call too
    assert call(src_n=5) == (EINVAL, "bad argument", 0)  # bytes at NULL
    assert call(src_n=5, links=0) == (EINVAL, "bad argument", 0)  # (the arguments every call checks come first)
    assert call(offs=cap, n_table=1)[:2] == (EINVAL, "bad argument")  # half a table
    assert call(caps=None)[:2] == (EINVAL, "bad argument")  # no capacities
    # d_bases, crcs, elems and pieces are optional: with them NULL the call gets past the argument check, to the device
    for links in (1, 3):
        rc, err, _ = call(bases=None, crcs=None, elems=None, pieces=None, n_dsts=0, dsts=None, caps=None, links=links)
        assert rc == (OK if lib.orz_device_count() > 0 else ENODEV), err


def test_the_hook_refuses_bad_arguments_without_a_device(native):
    lib = native.load()
    ms = ctypes.c_double()
    at = ctypes.c_void_p(16)
    good = dict(inter=at, base=at, planes=at, count=16, elem=2, links=2, reps=1, ms=ctypes.byref(ms))

    def call(**kw):
        a = dict(good, **kw)
        return lib.orz_plane_chain_move_time(0, a["inter"], a["base"], a["planes"], a["count"], a["elem"], a["links"], a["reps"], a["ms"])

    for bad in (dict(inter=None), dict(planes=None), dict(count=0), dict(elem=3), dict(links=0), dict(reps=0), dict(ms=None)):
        assert call(**bad) == EINVAL and native.last_error() == "bad argument", bad
