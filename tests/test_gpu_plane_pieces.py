"""GPU tier: planes cut into pieces (orz_members_encode_planes_pieces_to_device, orz_decode_members_planes_pieces,
orz_reader_set_planes_pieces) through the Python face.  Bars: every piece's stream is byte for byte what the same encoder writes for
the piece cut in numpy as a segment of its own, and the oracle decodes it to that piece; without pieces the members are those of
encode_tensor_planes; the one-shot decode and the reader give the tensors' bytes and agree with their emulation twin
(tests/emu/emu_plane_pieces.cpp) on sizes, statistics, host waits and the text of every refusal.  Pieces are a few KB at most: a
member decodes on one lane."""
import random

import pytest

import _cachecases as cc
import _elemcases as ec
import _piececases as pp
import _planecases as pc
import _rangecases as rc

pytestmark = pytest.mark.gpu

POISON, GUARD = pc.POISON, pc.GUARD
KEYS = ("ranges", "members_decoded", "decoded_bytes", "out_bytes", "launches", "host_waits")
SIZES = (16, 4096)


@pytest.fixture(scope="module")
def enc():
    import orz_amd
    import torch

    torch.cuda.init()  # (torch opens the device before the library does, as in the other GPU tests)
    e = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    yield e
    e.close()


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0") if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")


def _typed(torch, data, e):
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e]
    return _dev(torch, data).view(dt) if data else torch.empty(0, dtype=dt, device="cuda:0")


def _host(t):
    return bytes(t.cpu().numpy())


def _streams(container, members):
    host = _host(container)
    return [host[o:o + ln] for o, ln in members]


def _message(call):
    """(code, text) of the OrzError a call raises"""
    import orz_amd

    with pytest.raises(orz_amd.OrzError) as info:
        call()
    text = str(info.value)
    return int(text.split("(", 1)[1].split(")", 1)[0]), text.split("): ", 1)[1]


@pytest.fixture(scope="module", params=SIZES)
def packed(request, enc):
    """(S, [(bytes, element size)], tensors on the device, container, members, elems, pieces) of the small counts at a piece size"""
    import torch

    S = request.param
    ts = pp.tensors(S, seed=1)
    tensors = [_typed(torch, d, e) for d, e in ts]
    container, members, elems, pieces = enc.encode_tensor_pieces(tensors, S)
    return S, ts, tensors, container, members, elems, pieces


# ------------------------------------------------------------------------------------------------ streams
def test_each_piece_is_a_member_of_its_own(enc, oracle, packed):
    import torch

    S, ts, tensors, container, members, elems, pieces = packed
    want, qs = pp.members_of(ts, S)
    assert elems == [e for _, e in ts] and pieces == qs and max(qs) == 4 and len(members) == len(want) <= 100
    lengths = [len(d) for d, _ in ts]
    bound, count = enc.bound_planes_pieces(lengths, elems, S)
    assert count == len(members) and bound >= container.numel()
    spans = sorted((o, o + ln) for o, ln in members)
    assert all(ln > 0 for _, ln in members) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    # the pieces cut in numpy, each a segment of its own, in ONE call of the same encoder
    alone, table = enc.encode_tensors([_dev(torch, m) for m in want])
    for k, (s, a, m) in enumerate(zip(_streams(container, members), _streams(alone, table), want)):
        assert s == a, "member %d (a piece of %d bytes) differs from the piece encoded alone" % (k, len(m))
        assert oracle.decode(s) == (m, len(s)), k


def test_host_tensors_and_no_pieces(enc, packed):
    S, ts, tensors, container, members, elems, pieces = packed
    b, mb, _, qb = enc.encode_tensor_pieces([t.cpu() for t in tensors], S)
    assert qb == pieces and _streams(b, mb) == _streams(container, members)
    # a piece size of 0, and one no tensor reaches: the members of encode_tensor_planes, byte for byte
    whole, mw, ew = enc.encode_tensor_planes(tensors)
    for P in (0, 1 << 20):
        c, mc, ec_, qc = enc.encode_tensor_pieces(tensors, P)
        assert qc == [1] * len(ts) and ec_ == ew and _streams(c, mc) == _streams(whole, mw)
    assert enc.encode_tensor_pieces([], 32)[1:] == ([], [], []) and enc.encode_planes_pieces_to_device([], [], [], 32, 0, 0) == ([], [])


def test_what_the_encode_refuses(enc):
    import torch

    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
    for P in (8, 17, 4095):
        code, text = _message(lambda: enc.encode_planes_pieces_to_device([buf.data_ptr()], [4096], [4], P, out.data_ptr(), out.numel()))
        assert code == pp.EINVAL and "%d elements are no multiple of 16" % P in text
    for lens, elems in (([30], [3]), ([30], [4]), ([32, 7], [4, 2])):  # what the planes call refuses
        assert _message(lambda: enc.encode_planes_pieces_to_device([buf.data_ptr()] * len(lens), lens, elems, 16, out.data_ptr(), out.numel()))[0] == pp.EINVAL
    assert _message(lambda: enc.encode_planes_pieces_to_device([out.data_ptr() + 64], [64], [4], 16, out.data_ptr(), out.numel()))[0] == pp.EINVAL
    with pytest.raises(ValueError):
        enc.encode_tensor_pieces([buf], 24)
    assert not out.any()


# ------------------------------------------------------------------------------------------------ round trip
def _destinations(torch, tensors, room=0):
    """a tensor like each of `tensors`, carved in REVERSE order out of one poisoned arena with guard gaps: (arena, outs, offsets, sizes)"""
    sizes = [t.numel() * t.element_size() for t in tensors]
    at, offs = GUARD, [0] * len(tensors)
    for k in reversed(range(len(tensors))):
        offs[k] = at
        at += (sizes[k] + room + GUARD + 15) // 16 * 16
    arena = torch.full((at,), POISON, dtype=torch.uint8, device="cuda:0")
    return arena, [arena[o:o + s].view(t.dtype) for o, s, t in zip(offs, sizes, tensors)], offs, sizes


@pytest.mark.parametrize("how", ["device container and table", "host concatenation"])
def test_tensors_round_trip_as_on_the_emulation(packed, how):
    import orz_amd
    import torch

    S, ts, tensors, container, members, elems, pieces = packed
    arena, outs, offs, sizes = _destinations(torch, tensors)
    if how == "host concatenation":
        src, table = b"".join(_streams(container, members)), None
    else:
        src, table = container, members
    got, st = orz_amd.decode_planes_into(src, outs, device=0, members=table, pieces=pieces, stats=True)
    assert got == sizes
    pc.same(_host(arena), pc.expect_arena(arena.numel(), [(o, d) for o, (d, _) in zip(offs, ts)]), "the arena")
    eo, total = pc.layout(sizes, [0] * len(sizes), reverse=True)
    emu = pp.decode_pieces(pp.emu_lib(), bytes(src) if table is None else _host(container), table, list(zip(eo, sizes)), elems, pieces, total,
                           on_device=table is not None)
    assert emu.rc == 0 and emu.out_lens == got, emu.err
    assert (st["launches"], st["host_waits"], st["members"]) == (emu.launches, emu.host_waits, emu.members) == (1, 5, len(members))
    assert st["out_bytes"] == sum(sizes)


def test_refusals_equal_the_emulations(packed):
    import orz_amd
    import torch

    S, ts, tensors, container, members, elems, pieces = packed
    blob = _host(container)
    sizes = [len(d) for d, _ in ts]
    cut = pieces.index(4)
    short = list(sizes)
    short[cut] -= 1
    fewer, none = list(pieces), list(pieces)
    fewer[cut], none[cut] = 3, 0
    # the tensor of three pieces to a plane read as elements of half the size, six pieces to a plane: as many members, but the
    # third of them is the short last piece
    j3 = pieces.index(3)
    halves, six = list(elems), list(pieces)
    halves[j3], six[j3] = elems[j3] // 2, 6
    for caps, el, pcs, code in ((short, elems, pieces, pp.ENOMEM), (sizes, elems, fewer, pp.EINVAL), (sizes, elems, none, pp.EINVAL),
                                (sizes, halves, six, pp.EINVAL)):
        arena, outs, offs, _ = _destinations(torch, tensors, room=16)
        views = [arena[o:o + c] for o, c in zip(offs, caps)]
        eo, total = pc.layout(caps, [0] * len(caps), reverse=True)
        emu = pp.decode_pieces(pp.emu_lib(), blob, members, list(zip(eo, caps)), el, pcs, total)
        assert emu.rc == code and emu.launches == 0, emu.err
        assert _message(lambda: orz_amd.decode_planes_into(container, views, device=0, members=members, elems=el, pieces=pcs)) == (code, emu.err)
        assert _host(arena) == bytes([POISON]) * arena.numel()
    assert "pieces of destination %d differ in size" % j3 in emu.err
    with pytest.raises(ValueError):
        orz_amd.decode_planes_into(container, [t.view(torch.uint8) for t in tensors], device=0, members=members, elems=elems, pieces=pieces[:-1])


# ------------------------------------------------------------------------------------------------ the reader
def _ranges_of(count, S):
    """tests/test_plane_pieces_emu.py::_ranges_of"""
    out = [(3, S // 2), (S - 7, 7), (S, 9), (S - 5, 10), (S - 1, S + 2), (1, 2 * S + 3), (0, count), (count, 0), (S, 0), (2 * S, count - 2 * S),
           (S - 5, 10), (3, S // 2)]
    out += [(S + a, n) for a in (-17, -16, -1, 0, 1, 15) for n in (1, 4, 15, 16, 17, 33) if S + a + n <= count]
    return [(f, n) for f, n in out if f >= 0 and f + n <= count]


@pytest.fixture(scope="module")
def readers(packed):
    """(the reader on the GPU, its emulation twin on the container's bytes), declared alike"""
    import orz_amd

    S, ts, tensors, container, members, elems, pieces = packed
    rd = orz_amd.MemberReader(container, device=0, members=members, elems=elems, pieces=pieces)
    tw = pp.PieceReader(pp.emu_lib(), _host(container), table=members)
    assert tw.h, tw.err
    assert tw.set_planes_pieces(elems, pieces) == (0, "")
    yield rd, tw
    rd.close()
    tw.close()


def test_ranges_equal_the_tensors_and_the_emulation(packed, readers):
    import torch

    S, ts, tensors, container, members, elems, pieces = packed
    rd, tw = readers
    assert rd.tensors == tw.tensor_info() == [(len(d) // e, e) for d, e in ts]
    ranges = [(j, f, n) for j, (d, e) in enumerate(ts) if len(d) // e >= 2 * S + 5 for f, n in _ranges_of(len(d) // e, S)]
    ranges += [(j, 0, len(d) // e) for j, (d, e) in enumerate(ts)]
    random.Random(7).shuffle(ranges)
    want = ec.np_elements(ts, ranges)
    for rem in (0, 4, 1):
        arena = torch.full((len(want) + 2 * GUARD + 16,), POISON, dtype=torch.uint8, device="cuda:0")
        at = GUARD + (rem - arena.data_ptr() - GUARD) % 16
        got, st = rd.read_elements(ranges, out=arena[at:at + len(want)], stats=True)
        assert got.numel() == len(want)
        pc.same(_host(arena), pc.expect_arena(arena.numel(), [(at, want)]), "the arena (destination at %d modulo 16)" % rem)
        e = tw.read_elements(ranges, len(want), rem=rem)
        assert e.rc == 0 and e.out == want, e.err
        assert {k: st[k] for k in KEYS} == {k: getattr(e, k) for k in KEYS}
        assert st["host_waits"] == 3 and st["launches"] == 1 and st["members_decoded"] == sum(e_ * q for (d, e_), q in zip(ts, pieces) if d)


def test_the_last_rows_cost_the_last_pieces(packed, readers):
    import torch

    S, ts, tensors, container, members, elems, pieces = packed
    rd, tw = readers
    for j, (d, e) in enumerate(ts):
        count = len(d) // e
        if pieces[j] < 3:
            continue
        first = (pieces[j] - 1) * S + 2
        got = rd.read_tensor(j, first, out=torch.empty(count - first, dtype=tensors[j].dtype, device="cuda:0"))
        assert torch.equal(got, tensors[j][first:])
        for ranges in ([(j, first, count - first)], [(j, S - 1, 2)], [(j, 2 * S - 3, count - 2 * S + 3), (j, 0, 1)]):
            got, st = rd.read_elements(ranges, stats=True)
            w = tw.read_elements(ranges, got.numel())
            assert _host(got) == w.out == ec.np_elements(ts, ranges)
            assert {k: st[k] for k in KEYS} == {k: getattr(w, k) for k in KEYS}
        got, st = rd.read_elements([(j, first, count - first)], stats=True)
        assert st["members_decoded"] == e and st["decoded_bytes"] == e * (count - (pieces[j] - 1) * S) < e * count


def test_reader_refusals_equal_the_emulations(packed, readers):
    import orz_amd

    S, ts, tensors, container, members, elems, pieces = packed
    rd, tw = readers
    cut = next(j for j, q in enumerate(pieces) if q == 4)
    count = len(ts[cut][0]) // elems[cut]
    for ranges in ([(cut, count - 3, 4)], [(len(ts), 0, 0)], [(cut, count + 1, 0)]):
        e = tw.read_elements(ranges, 64)
        assert e.rc == pp.EINVAL and e.launches == 0 and e.untouched
        assert _message(lambda: rd.read_elements(ranges)) == (pp.EINVAL, e.err)
    fewer, none = list(pieces), list(pieces)
    fewer[cut], none[cut] = 3, 0
    for bad in (fewer, none):
        code, err = tw.set_planes_pieces(elems, bad)
        assert code == pp.EINVAL and _message(lambda: rd.set_planes(elems, bad)) == (pp.EINVAL, err)
        assert rd.tensors == tw.tensor_info() == [(len(d) // e, e) for d, e in ts]  # nothing changed
    with pytest.raises(ValueError):
        rd.set_planes(elems, pieces[:-1])
    assert _host(rd.read_tensor(cut, S - 1, 2)) == ts[cut][0][(S - 1) * elems[cut]:(S + 1) * elems[cut]]


def test_a_walk_under_a_cursor_budget(enc):
    import orz_amd
    import torch

    S, n = 4096, 3 * 4096 + 16
    g = torch.Generator().manual_seed(11)
    weights = (torch.randn(n, generator=g) * 0.02).to("cuda:0")
    ids = torch.randint(0, 50, (33,), generator=g, dtype=torch.uint8).to("cuda:0")
    container, members, elems, pieces = enc.encode_tensor_pieces([ids, weights], S)
    assert pieces == [1, 4]
    ts = [(_host(ids), 1), (_host(weights.view(torch.uint8)), 4)]
    budget = 16 * cc.cost(S, orz_amd.MemberReader.cursor_state_bytes())
    rd = orz_amd.MemberReader(container, device=0, members=members, cache_bytes=budget, elems=elems, pieces=pieces)
    tw = pp.PieceReader(pp.emu_lib(), _host(container), table=members)
    try:
        assert tw.set_planes_pieces(elems, pieces) == (0, "")
        tw.set_cache(budget)
        windows = [[(1, k * 2048, min(2048, n - k * 2048))] for k in range(7)]
        decoded = 0
        for again in (False, True):
            for k, w in enumerate(windows):
                got, st = rd.read_elements(w, stats=True)
                e = tw.read_elements(w, got.numel())
                assert _host(got) == e.out == ec.np_elements(ts, w)
                assert {key: st[key] for key in KEYS} == {key: getattr(e, key) for key in KEYS}
                cs = rd.cache_stats()
                assert cs == tw.cache_stats()
                assert (cs["hits"], cs["resumed"], cs["fresh"]) == ((4, 0, 0) if again else (0, 4, 0) if k % 2 else (0, 0, 4))
                assert st["host_waits"] == 2 and st["launches"] == (0 if again else 1)
                decoded += st["decoded_bytes"]
        assert 4 * n <= decoded <= 4 * n + 12 * (rc.SLACK - 1)
        got = rd.read_tensor(1, n - 10, 10, dtype=torch.float32)
        assert torch.equal(got, weights[n - 10:]) and rd.cache_stats()["hits"] == 4
    finally:
        rd.close()
        tw.close()


def test_a_damaged_piece_fails_only_the_reads_that_reach_it(oracle):
    """the damaged member of _rangecases (payload bits flipped in the last tenth of its last chunk: the decoder reports it by status)
    as piece 0 of a tensor of bytes; piece 1 is sixteen bytes"""
    import orz_amd

    data, good, bad = rc.damaged_text_member(oracle)
    S = len(data)
    assert S % 16 == 0
    tail = pc.tensor_bytes(1, 16, 3)
    ts = [(data + tail, 1)]
    blob = bad + oracle.encode(tail, 1)
    rd = orz_amd.MemberReader(blob, device=0, elems=[1], pieces=[2])
    try:
        assert rd.tensors == [(S + 16, 1)]
        for ranges in ([(0, S, 16)], [(0, 100, 5000), (0, S + 3, 4)]):  # piece 1 alone; piece 0 far in front of the damage
            got, st = rd.read_elements(ranges, stats=True)
            assert _host(got) == ec.np_elements(ts, ranges) and st["members_decoded"] == len(ranges)
        code, text = _message(lambda: rd.read_elements([(0, S - 64, 72)]))
        assert code == pp.EINVAL and "member 0," in text, text
        assert _host(rd.read_elements([(0, S, 16)])) == tail  # the reader serves on
    finally:
        rd.close()
