"""GPU tier: element ranges of plane-encoded tensors through orz_amd.MemberReader (orz_reader_set_planes, orz_reader_read_elements).
Bars: every read equals the slice of the tensor that was encoded, into fresh tensors and into tensors carved from a poisoned
arena that is compared whole, at destinations that take each store tier of ElementGather; a mixed batch equals the numpy
restatement; bytes, statistics and the text of every refusal equal those of the emulation twin (tests/emu/emu_elements.cpp) on
the container's bytes; a walk under a cursor budget decodes as the twin's does.  Planes are a few KB: a member decodes on one lane."""
import ctypes

import pytest

import _cachecases as cc
import _elemcases as ec
import _planecases as pc

pytestmark = pytest.mark.gpu

POISON, GUARD = pc.POISON, pc.GUARD
KEYS = ("ranges", "members_decoded", "decoded_bytes", "out_bytes", "launches", "host_waits")


def _originals(torch):  # (tests/test_gpu_planes.py::_originals)
    g = torch.Generator().manual_seed(5)

    def ints(n, dt):
        return torch.randint(0, 50, (n,), generator=g, dtype=dt)

    return [
        (torch.randn(4097, generator=g) * 0.02).to(torch.bfloat16),
        torch.randn(1029, generator=g) * 0.02,
        torch.arange(333, dtype=torch.int64) * 3 + ints(333, torch.int64),
        ints(640, torch.int16),
        ints(2500, torch.uint8),
        torch.empty(0, dtype=torch.int64),
        ints(1, torch.int32), ints(1, torch.int64), ints(1, torch.uint8),
        (torch.randn(17, generator=g)).to(torch.bfloat16), torch.randn(17, generator=g), ints(17, torch.int64),
        ints(16, torch.int16), ints(15, torch.int64),
    ]


def _bytes_of(torch, t):
    return bytes(t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy())


def _host(t):
    return bytes(t.cpu().numpy())


@pytest.fixture(scope="module")
def packed():
    """(tensors on the device, container, members, elems, [(bytes, element size)]) of the tensors, encoded by three workers"""
    import orz_amd
    import torch

    tensors = [t.to("cuda:0") for t in _originals(torch)]
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    try:
        container, members, elems = enc.encode_tensor_planes(tensors)
    finally:
        enc.close()
    assert elems == [t.element_size() for t in tensors]
    return tensors, container, members, elems, [(_bytes_of(torch, t), e) for t, e in zip(tensors, elems)]


@pytest.fixture(scope="module")
def reader(packed):
    import orz_amd

    _, container, members, elems, _ = packed
    rd = orz_amd.MemberReader(container, device=0, members=members, elems=elems)
    yield rd
    rd.close()


@pytest.fixture(scope="module")
def twin(packed):
    """the emulation's reader on the container's bytes, declared alike"""
    _, container, members, elems, _ = packed
    rd = ec.ElemReader(ec.emu_lib(), _host(container), table=members)
    assert rd.h, rd.err
    assert rd.set_planes(elems) == (0, "")
    yield rd
    rd.close()


# ------------------------------------------------------------------------------------------------ reads
def test_whole_tensors_and_slices(reader, packed):
    import torch

    tensors = packed[0]
    assert reader.tensors == [(t.numel(), t.element_size()) for t in tensors]
    for j, t in enumerate(tensors):
        n = t.numel()
        got = reader.read_tensor(j, dtype=t.dtype)
        assert got.dtype == t.dtype and torch.equal(got.view(torch.uint8), t.view(torch.uint8)), j
        # a fresh tensor lies at a multiple of 16: the heads before the first full unit put the units' destinations at every tier
        for first, count in ((1, n - 1), (14, 40), (15, 33), (16, 16), (17, 50)):
            if first > n:
                continue
            count = min(count, n - first)
            got = reader.read_tensor(j, first, count, dtype=t.dtype)
            assert torch.equal(got.view(torch.uint8), t[first:first + count].view(torch.uint8)), (j, first, count)
        assert reader.read_tensor(j, n, dtype=t.dtype).numel() == 0


@pytest.mark.parametrize("rem", [0, 4, 8, "e"])
def test_slices_into_tensors_carved_from_a_poisoned_arena(reader, packed, rem):
    """the first unit's destination at 0, 4, 8 and the element size modulo 16: 16-byte stores, dword stores, and for elements of
    one and two bytes at `e` the byte path"""
    import torch

    tensors = packed[0]
    for j in (0, 1, 2, 3, 4, 9, 13):
        t = tensors[j]
        e, n = t.element_size(), t.numel()
        r = e % 16 if rem == "e" else rem
        if r % e:
            continue  # (a typed tensor lies at a multiple of its element size)
        for first, count in ((0, n), (16, 64), (3, 30)):
            if first >= n:
                continue
            count = min(count, n - first)
            (at,), alen = pc.layout([count * e], [r])
            arena = torch.full((alen + 16,), POISON, dtype=torch.uint8, device="cuda:0")
            at += (-arena.data_ptr()) % 16
            out = arena[at:at + count * e].view(t.dtype)
            assert out.data_ptr() % 16 == r
            got = reader.read_tensor(j, first, count, out=out)
            assert got.data_ptr() == out.data_ptr() and got.numel() == count
            want = _bytes_of(torch, t[first:first + count])
            pc.same(_host(arena), pc.expect_arena(alen + 16, [(at, want)]), "the arena (tensor %d, first %d, count %d)" % (j, first, count))


def _batch():
    """a mixed batch over the round trip's tensors: out of order, repeated, overlapping, empty, the byte tensor in the middle"""
    return [(2, 300, 33), (0, 3, 4000), (12, 0, 16), (1, 0, 0), (0, 3, 4000), (4, 1, 2499), (1, 15, 34), (1, 31, 3), (5, 0, 0), (11, 16, 1),
            (8, 0, 1), (3, 17, 1), (2, 0, 17), (1, 1029, 0), (10, 1, 16), (13, 0, 15), (6, 0, 1)]


def test_a_mixed_batch_equals_the_restatement_and_the_emulation(reader, twin, packed):
    ts = packed[4]
    ranges = _batch()
    want = ec.np_elements(ts, ranges)
    got, st = reader.read_elements(ranges, stats=True)
    assert _host(got) == want
    e = twin.read_elements(ranges, len(want))
    assert e.rc == 0 and e.out == want, e.err
    assert {k: st[k] for k in KEYS} == {k: getattr(e, k) for k in KEYS}, (st, {k: getattr(e, k) for k in KEYS})
    assert st["host_waits"] == 3 and st["launches"] == 1 and st["kernel_ms"] > 0 and st["gather_ms"] > 0
    assert st["members_decoded"] == sum(ts[j][1] for j in {j for j, _, c in ranges if c})
    # nothing: no launch, no wait
    for nothing in ([], [(0, 7, 0), (5, 0, 0)]):
        got, st = reader.read_elements(nothing, stats=True)
        assert got.numel() == 0 and st["launches"] == 0 and st["host_waits"] == 0


def test_refusals_equal_the_emulations(reader, twin, packed):
    import orz_amd
    import torch

    tensors, container, members, elems, ts = packed
    T = len(ts)

    def message(call):
        with pytest.raises(orz_amd.OrzError) as info:
            call()
        text = str(info.value)
        return int(text.split("(", 1)[1].split(")", 1)[0]), text.split("): ", 1)[1]

    for ranges in ([(0, 0, 4), (T, 0, 0)], [(1, 0, 4), (1, 1026, 4)], [(1, 1030, 0)], [(1, (1 << 64) - 1, 2)], [(1, 2, (1 << 64) - 1)]):
        e = twin.read_elements(ranges, 64)
        assert e.rc == ec.EINVAL and e.launches == 0 and e.untouched
        assert message(lambda: reader.read_elements(ranges)) == (ec.EINVAL, e.err)
    # a buffer one byte short: nothing is written
    arena = torch.full((GUARD + 27 + GUARD,), POISON, dtype=torch.uint8, device="cuda:0")
    e = twin.read_elements([(1, 0, 4), (1, 9, 3)], cap=27)
    assert e.rc == ec.ENOMEM and e.dst_len == 28 and e.untouched
    assert message(lambda: reader.read_elements([(1, 0, 4), (1, 9, 3)], out=arena[GUARD:GUARD + 27])) == (ec.ENOMEM, e.err)
    assert _host(arena) == bytes([POISON]) * arena.numel()
    # the output inside the container
    before = _host(container)
    e = twin.read_elements([(1, 0, 4)], raw=(ctypes.addressof(twin.src) + 3, 16))
    assert e.rc == ec.EINVAL
    assert message(lambda: reader.read_elements([(1, 0, 4)], out=container[3:19])) == (ec.EINVAL, e.err)
    assert _host(container) == before
    # NULL arrays, by the library's own call
    lib = reader._lib
    dlen = ctypes.c_uint64()
    e = twin.read_elements([(0, 0, 1)], 64, null_arrays=True)
    assert lib.orz_reader_read_elements(reader._h, None, None, None, 1, None, 0, ctypes.byref(dlen), None) == ec.EINVAL == e.rc
    assert orz_amd._native.last_error() == e.err
    # what set_planes refuses, on readers of their own: the declaration stays what it was
    rd = orz_amd.MemberReader(container, device=0, members=members)
    tw = ec.ElemReader(ec.emu_lib(), before, table=members)
    try:
        e = tw.read_elements([(0, 0, 1)], 64)
        assert e.rc == ec.EINVAL and message(lambda: rd.read_elements([(0, 0, 1)])) == (ec.EINVAL, e.err)
        rd.set_planes(elems)
        assert tw.set_planes(elems) == (0, "")
        wrong, unequal = list(elems), list(elems)
        wrong[0], wrong[1] = 1, 1  # 4 planes fewer
        unequal[0], unequal[1] = 4, 2  # bf16 x 4097 and fp32 x 1029 read as 4 + 2 planes: members 0 (4097 bytes) and 2 (1029) differ
        for bad in (elems[:4] + [3] + elems[5:], wrong, unequal):
            rc_, err = tw.set_planes(bad)
            assert rc_ == ec.EINVAL and message(lambda: rd.set_planes(bad)) == (ec.EINVAL, err)
            assert rd.tensors == tw.tensor_info() == [(len(d) // e, e) for d, e in ts]
        assert "tensor 0 " in err and "member 2 " in err
        rc_, err = tw.set_planes([2, 4], null=True)
        assert lib.orz_reader_set_planes(rd._h, None, 2) == ec.EINVAL == rc_ and orz_amd._native.last_error() == err
        assert _host(rd.read_tensor(9)) == ts[9][0]
        rd.set_planes(None)
        assert rd.tensors == []
    finally:
        rd.close()
        tw.close()
    assert _host(reader.read_tensor(9)) == ts[9][0]  # the shared reader serves on


# ------------------------------------------------------------------------------------------------ cursors
def test_a_walk_under_a_cursor_budget(packed):
    import orz_amd
    import torch

    n = 20_000
    g = torch.Generator().manual_seed(11)
    weights = (torch.randn(n, generator=g) * 0.02).to("cuda:0")
    ids = torch.randint(0, 50, (33,), generator=g, dtype=torch.uint8).to("cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    try:
        container, members, elems = enc.encode_tensor_planes([ids, weights])
    finally:
        enc.close()
    ts = [(_bytes_of(torch, ids), 1), (_bytes_of(torch, weights), 4)]
    budget = 4 * cc.cost(n, orz_amd.MemberReader.cursor_state_bytes())
    rd = orz_amd.MemberReader(container, device=0, members=members, cache_bytes=budget, elems=elems)
    tw = ec.ElemReader(ec.emu_lib(), _host(container), table=members)
    try:
        assert tw.set_planes(elems) == (0, "")
        tw.set_cache(budget)
        windows = [[(1, k * 4000, 4000)] for k in range(5)]
        decoded = 0
        for again in (False, True):
            for k, w in enumerate(windows):
                got, st = rd.read_elements(w, stats=True)
                e = tw.read_elements(w, 16_000)
                assert _host(got) == e.out == ec.np_elements(ts, w)
                assert {key: st[key] for key in KEYS} == {key: getattr(e, key) for key in KEYS}
                cs = rd.cache_stats()
                assert cs == tw.cache_stats()
                assert (cs["hits"], cs["resumed"], cs["fresh"]) == ((4, 0, 0) if again else (0, 4, 0) if k else (0, 0, 4))
                assert st["host_waits"] == 2 and st["launches"] == (0 if again else 1)
                decoded += st["decoded_bytes"]
        assert 4 * n <= decoded <= 4 * n + 4 * (ec.rc.SLACK - 1)
        got = rd.read_tensor(1, 19_990, 10, dtype=torch.float32)
        assert torch.equal(got, weights[19_990:]) and rd.cache_stats()["hits"] == 4
    finally:
        rd.close()
        tw.close()


# ------------------------------------------------------------------------------------------------ the Python face
def test_declaring_at_open_equals_declaring_later(reader, packed):
    import orz_amd

    _, container, members, elems, ts = packed
    rd = orz_amd.MemberReader(container, device=0, members=members)
    try:
        assert rd.tensors == []
        rd.set_planes(elems)
        assert rd.tensors == reader.tensors
        ranges = _batch()
        a, sa = rd.read_elements(ranges, stats=True)
        b, sb = reader.read_elements(ranges, stats=True)
        assert _host(a) == _host(b) and {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}
        whole = rd.read(0, rd.total)  # byte ranges are served as before
        assert _host(whole) == b"".join(pc.planes_of(ts))
    finally:
        rd.close()
    with pytest.raises(orz_amd.OrzError, match=r"\(-22\).*planes for"):
        orz_amd.MemberReader(container, device=0, members=members, elems=elems[:-1])


def test_what_python_refuses(reader, packed):
    import torch

    for ranges in ([(-1, 0, 0)], [(0, -1, 0)], [(0, 0, -1)], [(1 << 64, 0, 0)], [(0, 0, 1 << 64)]):
        with pytest.raises(ValueError):
            reader.read_elements(ranges)
    for args in ((-1,), (0, -1), (0, 0, -1), (1 << 64,), (0, 1 << 64), (0, 0, 1 << 64)):
        with pytest.raises(ValueError):
            reader.read_tensor(*args)
    with pytest.raises(ValueError):
        reader.set_planes([2, -1])
    with pytest.raises(ValueError):
        reader.set_planes([1 << 32])
    dev = torch.zeros(64, dtype=torch.int16, device="cuda:0")
    for out in (dev, torch.zeros(64, dtype=torch.uint8), dev.view(torch.uint8)[::2]):
        with pytest.raises(ValueError):
            reader.read_elements([(0, 0, 4)], out=out)
    # read_tensor: tensor 0 has elements of two bytes
    for out in (dev.view(torch.uint8), dev.view(torch.int32), torch.zeros(64, dtype=torch.int16), dev[::2], [0] * 8):
        with pytest.raises(ValueError):
            reader.read_tensor(0, 0, 4, out=out)
    assert reader.read_tensor(0, 0, 4, out=dev).numel() == 4
