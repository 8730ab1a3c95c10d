"""Planes cut into pieces (orz_amd/csrc/orz_planes.h, orz_read_elements.h) on the emulation backend, on containers the ORACLE's
encoder made of pieces cut in numpy: the one-shot decode inside poisoned arenas with guard gaps -- bytes, launches and host waits
against decode_members_scatter's, every refusal before a byte is written --, the plan kernel alone on invented size columns of
more than 2^32 elements, the gather alone against numpy slices, and the reader: what a read costs, damage, cursors, declarations."""
import random
import re

import pytest

import _data
import _elemcases as ec
import _piececases as pp
import _planecases as pc
import _rangecases as rc
import _scattercases as sc
from _piececases import EINVAL, ENOMEM, MASK, POISON, SIZES

REMS = ("0", "1", "e", "8")


@pytest.fixture(scope="module")
def lib():
    return pp.emu_lib()


@pytest.fixture(scope="module")
def stream(oracle):
    """the oracle's stream of some bytes at level 1, remembered"""
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


def _places(ts, how, room=9):
    """destinations in REVERSE order in the arena, at addresses that are 0, 1, the element size or 8 modulo 16, `room` bytes of
    capacity behind each size"""
    caps = [len(d) + room for d, _ in ts]
    offs, total = pc.layout(caps, [{"0": 0, "1": 1, "e": e % 16, "8": 8}[how] for _, e in ts], reverse=True)
    return offs, caps, total


def _scatter_twin(blob, table, members):
    """decode_members_scatter on the same container, a destination per member: (launches, host_waits)"""
    caps = [len(m) for m in members]
    offs, total = sc.reverse_layout(caps, guard=3)
    r = sc.scatter(sc.emu_lib(), blob, table, [(o if c else None, c) for o, c in zip(offs, caps)], total)
    assert r.rc == 0, r.err
    return r.launches, r.host_waits


# ------------------------------------------------------------------------------------------------ the cases
def test_the_cases_cover_what_they_claim():
    for S in SIZES:
        assert set(pp.counts_for(S)) == {0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S, 2 * S + 5, 3 * S + 16}
        seen = set()
        for seed in range(4):
            ts = pp.tensors(S, seed=seed)
            members, qs = pp.members_of(ts, S)
            seen |= {(e, len(d) // e) for d, e in ts}
            assert len(members) == sum(e * q for (_, e), q in zip(ts, qs))
            # tensors of one piece and of several interleave
            assert any(a == 1 and b > 1 for a, b in zip(qs, qs[1:])) and max(qs) == 4
        assert seen == {(e, c) for e in pp.ELEMS for c in pp.counts_for(S)}
    assert [pp.pieces_of(c, 16) for c in (0, 1, 16, 17, 32, 33)] == [1, 1, 1, 2, 2, 3] and pp.pieces_of(100, 0) == 1
    assert pp.cut(bytes(range(80)), 2, 16) == [bytes(range(0, 32, 2)), bytes(range(32, 64, 2)), bytes(range(64, 80, 2)),
                                               bytes(range(1, 32, 2)), bytes(range(33, 64, 2)), bytes(range(65, 80, 2))]


# ------------------------------------------------------------------------------------------------ the decode driver
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("S", SIZES)
def test_pieces_decode_into_the_original_bytes(lib, stream, S, seed):
    ts = pp.tensors(S, seed=seed)
    blob, table, _, qs = pp.container(stream, ts, S)
    elems = [e for _, e in ts]
    offs, caps, total = _places(ts, REMS[seed])
    r = pp.decode_pieces(lib, blob, table, list(zip(offs, caps)), elems, qs, total)
    assert r.rc == 0, r.err
    assert r.members == sum(e * q for e, q in zip(elems, qs)) and r.out_lens == [len(d) for d, _ in ts]
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations")
    assert (r.launches, r.host_waits) == _scatter_twin(blob, table, pp.members_of(ts, S)[0]) == (1, 4)


@pytest.mark.parametrize("layout", ["permuted table", "host container"])
def test_other_containers(lib, stream, layout):
    S = 32
    ts = pp.tensors(S, seed=2)
    blob, table, _, qs = pp.container(stream, ts, S, "table" if layout == "permuted table" else "concatenation")
    offs, caps, total = _places(ts, "e")
    r = pp.decode_pieces(lib, blob, table, list(zip(offs, caps)), [e for _, e in ts], qs, total, on_device=layout != "host container", fill=0)
    assert r.rc == 0, r.err
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)], fill=0), "the zeroed arena")
    launches, waits = _scatter_twin(blob, table, pp.members_of(ts, S)[0])
    assert r.launches == launches == 1 and r.host_waits == waits + (layout == "host container") == 5


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("S", [16, 32])
def test_few_members_in_flight_give_the_same_bytes(lib, stream, S, slots):
    """a plane's pieces fall into different rounds of decode launches; the merge still comes behind all of them"""
    ts = pp.tensors(S, seed=1)
    blob, table, _, qs = pp.container(stream, ts, S)
    offs, caps, total = _places(ts, "0")
    r = pp.decode_pieces(lib, blob, table, list(zip(offs, caps)), [e for _, e in ts], qs, total, slots=slots)
    assert r.rc == 0, r.err
    assert r.launches == -(-r.members // slots) > max(qs) and r.host_waits == 4
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations")


def test_one_piece_everywhere_is_decode_members_planes(lib, stream):
    ts = pc.mixed_tensors(counts=(0, 17, 1029))
    blob = b"".join(stream(pl) for pl in pc.planes_of(ts))
    elems = [e for _, e in ts]
    offs, caps, total = _places(ts, "e")
    a = pp.decode_pieces(lib, blob, None, list(zip(offs, caps)), elems, [1] * len(ts), total)
    b = pc.decode_planes(pc.emu_lib(), blob, None, list(zip(offs, caps)), elems, total)
    assert a.rc == b.rc == 0 and a.arena == b.arena and a.out_lens == b.out_lens
    assert (a.launches, a.host_waits, a.members) == (b.launches, b.host_waits, b.members)


def test_sizing_call_decodes_nothing(lib, stream):
    ts = pp.tensors(16, seed=3)
    blob, table, _, qs = pp.container(stream, ts, 16, "table")
    r = pp.decode_pieces(lib, blob, table, [(None, 0)] * len(ts), [e for _, e in ts], qs, 64, sizing=True)
    assert r.rc == 0, r.err
    assert r.out_lens == [len(d) for d, _ in ts] and r.launches == 0 and r.arena == bytes([POISON]) * 64
    e = pp.decode_pieces(lib, b"", None, [], [], [], 16)
    assert e.rc == 0 and e.members == 0 and e.launches == 0


# ------------------------------------------------------------------------------------------------ refusals
HEAD, TAIL = (pc.tensor_bytes(1, 5, 1), 1), (pc.tensor_bytes(4, 16, 2), 4)
GOOD = (32, 32, 5, 32, 32, 5)  # destination 1: int16 x 69 at S = 32 -- members 1 .. 6; member 0 before it, members 7 .. 10 behind


def _sized(stream, sizes):
    """a container of 11 members: 5 bytes | members that decode to `sizes` bytes | the four planes of int32 x 16"""
    members = [HEAD[0]] + [pc.tensor_bytes(1, n, 30 + k) for k, n in enumerate(sizes)] + pc.np_split(*TAIL)
    return b"".join(stream(m) for m in members)


# (sizes of members 1 .. 6, pieces, what the message says)
BAD_PIECES = [
    (GOOD, [1, 0, 1], r"%s 1 has no pieces"),
    (GOOD, [1, 2, 1], r"9 pieces of planes for 11 members"),
    (GOOD, [1, 3, 2], r"15 pieces of planes for 11 members"),
    ((32, 16, 5, 32, 16, 5), [1, 3, 1], r"pieces of %s 1 differ in size: member 2 decodes to 16 bytes, member 1 to 32"),
    ((24, 24, 5, 24, 24, 5), [1, 3, 1], r"pieces of %s 1 are no multiple of 16 elements: member 1 decodes to 24 bytes"),
    ((32, 32, 0, 32, 32, 0), [1, 3, 1], r"last piece of %s 1 has not 1 .. 32 bytes: member 3 decodes to 0 bytes"),
    ((32, 32, 33, 32, 32, 33), [1, 3, 1], r"last piece of %s 1 has not 1 .. 32 bytes: member 3 decodes to 33 bytes"),
    ((32, 32, 5, 32, 32, 4), [1, 3, 1], r"planes of %s 1 differ in size: member 6 decodes to 4 bytes, member 3 to 5"),
    ((32, 32, 5, 32, 16, 5), [1, 3, 1], r"planes of %s 1 differ in size: member 5 decodes to 16 bytes, member 2 to 32"),
]


@pytest.mark.parametrize("case", range(len(BAD_PIECES)))
def test_what_the_decode_refuses_of_pieces(lib, stream, case):
    sizes, pieces, pattern = BAD_PIECES[case]
    ts = [HEAD, (b"\0" * 2 * 69, 2), TAIL]
    offs, caps, total = _places(ts, "0", room=64)
    r = pp.decode_pieces(lib, _sized(stream, sizes), None, list(zip(offs, caps)), [1, 2, 4], pieces, total)
    assert r.rc == EINVAL and re.search(pattern.replace("%s", "destination"), r.err), r.err
    assert r.launches == 0 and r.arena == bytes([POISON]) * total


def test_a_capacity_one_byte_short_writes_nothing(lib, stream):
    ts = [HEAD, (b"\0" * 2 * 69, 2), TAIL]
    for short in range(3):
        offs, caps, total = _places(ts, "0", room=0)
        caps[short] -= 1
        r = pp.decode_pieces(lib, _sized(stream, GOOD), None, list(zip(offs, caps)), [1, 2, 4], [1, 3, 1], total)
        assert r.rc == ENOMEM and "destination %d " % short in r.err, r.err
        assert r.launches == 0 and r.arena == bytes([POISON]) * total
        assert r.out_lens == [5, 138, 64]  # (the sizes come back with the refusal)


def test_null_arrays_and_no_destinations(lib, stream):
    r = pp.decode_pieces(lib, _sized(stream, GOOD), None, [], [], [], 16)
    assert r.rc == EINVAL and "0 pieces of planes for 11 members" in r.err and r.launches == 0


# ------------------------------------------------------------------------------------------------ the plan kernel alone
def _check_plan(lib, dsts, caps, elems, pieces, out_len, base, stage):
    got, want = pp.plan(lib, dsts, caps, elems, pieces, out_len, base, stage), pp.np_plan(dsts, caps, elems, pieces, out_len, base, stage)
    for key in want:
        assert got[key] == want[key], key
    return got


def test_the_plan_counts_beyond_32_bits(lib):
    """size columns nobody decodes: S = 2^31 and Q = 3 make 2^32 + 5 elements to a plane, 8 bytes each; the offsets, the pitch,
    the units and the verdict are 64-bit sums of 32-bit sizes"""
    S = 1 << 31
    elems, pieces = [2, 8, 1, 4], [1, 3, 3, 2]
    out_len = [17, 17] + [S, S, 5] * 8 + [S, S, S] + [S, 16] * 4
    count = [17, 2 * S + 5, 3 * S, S + 16]
    dsts = [0x7F00_0000_0010, 0x7E00_0000_0001, 0x7D00_0000_0008, 0x7C00_0000_0004]
    caps = [c * e for c, e in zip(count, elems)]
    stage = 0x1000_0000_0100
    got = _check_plan(lib, dsts, caps, elems, pieces, out_len, stage, stage)
    assert got["count"] == [17, 2 * S + 5, 0, S + 16] and got["count"][1] > 1 << 32
    assert got["pitch"][1] == 2 * S + 16 and got["units"] == [2, (2 * S + 5 + 15) // 16, 0, (S + 16) // 16]
    assert not got["status"] and got["bad"] == 4 and got["total_units"] == sum(got["units"])
    # the tensor of bytes takes its pieces S apart in its destination; every staged plane lies inside plane_stage_bound
    assert [(o + stage) & MASK for o in got["out_off"][26:29]] == [dsts[2], dsts[2] + S, dsts[2] + 2 * S]
    bound = lib.emu_plane_stage_bound(pp.ctypes.c_uint64(sum(out_len)), pp.ctypes.c_uint64(len(out_len)))
    for j in (0, 1, 3):
        assert got["plane0"][j] % 16 == 0 and got["plane0"][j] + elems[j] * got["pitch"][j] <= stage + bound
    assert got["plane0"][0] + 2 * got["pitch"][0] <= got["plane0"][1] and got["plane0"][1] + 8 * got["pitch"][1] <= got["plane0"][3]
    # one byte short of 8 x (2^32 + 5): the verdict needs all 64 bits too
    for short in (1, 3, 2):
        less = list(caps)
        less[short] -= 1
        got = _check_plan(lib, dsts, less, elems, pieces, out_len, 0, stage)
        assert got["status"] and got["bad"] == short and got["verdict"] == [j == short for j in range(4)]


def test_the_plan_of_small_pieces(lib):
    for S in SIZES:
        ts = pp.tensors(S, seed=1)
        members, qs = pp.members_of(ts, S)
        dsts = [0x5000_0000 + 0x10_0000 * j + (j % 3) for j in range(len(ts))]
        _check_plan(lib, dsts, [len(d) for d, _ in ts], [e for _, e in ts], qs, [len(m) for m in members], 0x4000_0000, 0x4000_0000)


# ------------------------------------------------------------------------------------------------ the gather alone
def _ranges_of(count, S):
    """(first, count) over a tensor of `count` elements in pieces of S: inside one piece, up to a boundary, from one, across one
    and two, every alignment of first and count modulo 16 near a boundary, overlapping, repeated and empty ones"""
    out = [(3, S // 2), (S - 7, 7), (S, 9), (S - 5, 10), (S - 1, S + 2), (1, 2 * S + 3), (0, count), (count, 0), (S, 0), (2 * S, count - 2 * S),
           (S - 5, 10), (3, S // 2)]
    out += [(S + a, n) for a in (-17, -16, -1, 0, 1, 15) for n in (1, 4, 15, 16, 17, 33) if S + a + n <= count]
    return [(f, n) for f, n in out if f >= 0 and f + n <= count]


@pytest.mark.parametrize("how", REMS)
@pytest.mark.parametrize("S", SIZES)
def test_gather_equals_the_numpy_slice(lib, S, how):
    count = 3 * S + 16
    ts = [(pc.tensor_bytes(e, count if e != 1 else 2 * S + 5, 40 + e), e) for e in (4, 1, 8, 2)] + [(pc.tensor_bytes(2, 15, 9), 2)]
    ranges = [(j, f, n) for j, (d, e) in enumerate(ts[:4]) for f, n in _ranges_of(len(d) // e, S)] + [(4, 0, 15), (4, 3, 0), (4, 14, 1)]
    random.Random(S).shuffle(ranges)
    rem = {"0": 0, "1": 1, "e": 4, "8": 8}[how]
    units, arena, at, before, after = pp.gather(lib, ts, S, ranges, rem)
    assert units == sum(ec.units_of(f, n) for _, f, n in ranges)
    pc.same(arena, pc.expect_arena(len(arena), [(at, ec.np_elements(ts, ranges))]), "the arena")
    assert after == before


def test_gather_skips_the_units_of_a_failed_piece_only(lib):
    S = 32
    ts = [(pc.tensor_bytes(4, 3 * S + 16, 1), 4)]
    ranges = [(0, 0, 3 * S + 16)]
    bad = 2 * 4 + 1  # plane 2, piece 1: elements S .. 2 S - 1
    units, arena, at, _, _ = pp.gather(lib, ts, S, ranges, 0, bad_member=bad)
    d = ts[0][0]
    pc.same(arena, pc.expect_arena(len(arena), [(at, d[:4 * S]), (at + 8 * S, d[8 * S:])]), "the arena")


# ------------------------------------------------------------------------------------------------ the reader
@pytest.fixture(scope="module", params=SIZES)
def opened(request, lib, stream):
    """(reader, tensors, S, [Q]): a concatenation in "device" memory, declared with its pieces"""
    S = request.param
    ts = pp.tensors(S, seed=2) + pp.tensors(S, seed=0)
    blob, _, _, qs = pp.container(stream, ts, S)
    rd = pp.PieceReader(lib, blob)
    assert rd.h, rd.err
    assert rd.set_planes_pieces([e for _, e in ts], qs) == (0, "")
    yield rd, ts, S, qs
    rd.close()


def _check_read(r, ts, ranges):
    want = ec.np_elements(ts, ranges)
    assert r.rc == 0, r.err
    assert r.dst_len == len(want) == r.out_bytes and r.ranges == len(ranges)
    pc.same(r.arena, pc.expect_arena(r.arena_len, [(r.at, want)]), "the arena")


def test_info_reports_whole_tensors(opened):
    rd, ts, S, qs = opened
    assert rd.members == sum(e * q for (_, e), q in zip(ts, qs))
    assert rd.tensor_info() == [(len(d) // e, e) for d, e in ts]


@pytest.mark.parametrize("how", ["0", "1", "4"])
def test_ranges_over_pieces_in_one_call(opened, how):
    rd, ts, S, qs = opened
    ranges = [(j, f, n) for j, (d, e) in enumerate(ts) if len(d) // e >= 2 * S + 5 for f, n in _ranges_of(len(d) // e, S)]
    ranges += [(j, 0, len(d) // e) for j, (d, e) in enumerate(ts)]
    random.Random(7).shuffle(ranges)
    r = rd.read_elements(ranges, len(ec.np_elements(ts, ranges)), rem=int(how))
    _check_read(r, ts, ranges)
    assert r.members_decoded == sum(e * q for (d, e), q in zip(ts, qs) if d) and r.launches == 1 and r.host_waits == 3


def test_whole_tensors_equal_the_one_shot_decode(opened, lib, stream):
    rd, ts, S, qs = opened
    blob, _, _, _ = pp.container(stream, ts, S)
    offs, caps, total = _places(ts, "0", room=0)
    whole = pp.decode_pieces(lib, blob, None, list(zip(offs, caps)), [e for _, e in ts], qs, total)
    assert whole.rc == 0, whole.err
    ranges = [(j, 0, len(d) // e) for j, (d, e) in enumerate(ts)]
    r = rd.read_elements(ranges, sum(caps))
    _check_read(r, ts, ranges)
    assert r.out == b"".join(whole.arena[o:o + c] for o, c in zip(offs, caps))


def test_a_read_costs_the_pieces_it_touches(opened):
    """a range in the last piece of the longest tensors: e members, each up to the furthest byte asked of it and less than an item
    further -- what the byte-range read of those pieces costs, not what the tensor costs"""
    rd, ts, S, qs = opened
    lengths = [len(m) for m in pp.members_of(ts, S)[0]]
    for j, (d, e) in enumerate(ts):
        count = len(d) // e
        if count != 3 * S + 16:
            continue
        # (ranges, the pieces of a plane they touch, the byte ranges of a plane they become)
        for ranges, touched, parts in (([(j, 3 * S + 2, 10)], 1, 1), ([(j, 2 * S + 1, S + 3)], 2, 2), ([(j, S - 1, 2 * S + 2), (j, 5, 1)], 4, 5)):
            r = rd.read_elements(ranges, len(ec.np_elements(ts, ranges)))
            _check_read(r, ts, ranges)
            assert r.members_decoded == e * touched and r.host_waits == 3 and r.launches == 1
            expanded = pp.expand(ts, qs, S, ranges, rd.member_offsets)
            assert len(expanded) == e * parts
            rc.check_decoded_bytes(r.decoded_bytes, expanded, lengths)
            b = rd.read(expanded)
            assert b.rc == 0
            assert (r.launches, r.members_decoded, r.host_waits, r.decoded_bytes) == (b.launches, b.members_decoded, b.host_waits, b.decoded_bytes)
        r = rd.read_elements([(j, 3 * S + 2, 10)], 10 * e)
        assert r.decoded_bytes <= 16 * e < e * count


def test_few_slots_give_the_same_bytes(opened):
    rd, ts, S, qs = opened
    ranges = [(j, 1, len(d) // e - 1) for j, (d, e) in enumerate(ts) if d]
    r = rd.read_elements(ranges, len(ec.np_elements(ts, ranges)), slots=3)
    _check_read(r, ts, ranges)
    assert r.launches == -(-r.members_decoded // 3) > 1 and r.host_waits == 3


def test_declarations_and_what_they_refuse(lib, stream):
    rd = pp.PieceReader(lib, _sized(stream, GOOD))
    ts = [HEAD, (pc.np_merge([b"".join(pc.tensor_bytes(1, n, 30 + 3 * p + k) for k, n in enumerate(GOOD[:3])) for p in range(2)]), 2), TAIL]
    try:
        assert rd.members == 11
        assert rd.set_planes_pieces([1, 2, 4], [1, 3, 1]) == (0, "")
        info = rd.tensor_info()
        assert info == [(5, 1), (69, 2), (16, 4)]
        rd.set_cache(9 * ec.cc.cost(32, rd.state_bytes))
        probe = [(1, 30, 10), (0, 0, 5), (2, 3, 9)]  # (elements 30 .. 39: pieces 0 and 1 of both planes)
        _check_read(rd.read_elements(probe, 61), ts, probe)
        held = rd.cache_stats()["cursors"]
        assert held == 2 * 2 + 1 + 4
        for got in (rd.set_planes_pieces([1, 2, 4], [1, 0, 1]), rd.set_planes_pieces([1, 2, 4], [1, 2, 1]), rd.set_planes_pieces([1, 2, 4], [1, 3, 1], null=True),
                    rd.set_planes_pieces([1, 3, 4], [1, 2, 1]), rd.set_planes_pieces([2, 1, 4], [3, 1, 1]), rd.set_planes([1, 2, 4])):
            assert got[0] == EINVAL and got[1], got
            assert rd.tensor_info() == info and rd.cache_stats()["cursors"] == held  # nothing changed
            r = rd.read_elements(probe, 61)
            _check_read(r, ts, probe)
            assert rd.cache_stats()["hits"] == held and r.launches == 0
        assert "tensor 1 has no pieces" in rd.set_planes_pieces([1, 2, 4], [1, 0, 1])[1]
        assert "9 pieces of planes for 11 members" in rd.set_planes_pieces([1, 2, 4], [1, 2, 1])[1]
        assert "7 planes for 11 members" in rd.set_planes([1, 2, 4])[1]
        # the declaration without pieces and the byte ranges do what they did
        assert rd.set_planes([1] * 11) == (0, "") and rd.tensor_info() == [(n, 1) for n in (5,) + GOOD + (16,) * 4]
        flat = [(j, 0, n) for j, n in enumerate((5,) + GOOD)]
        _check_read(rd.read_elements(flat, 5 + sum(GOOD)), [(ts[0][0], 1)] + [(m, 1) for m in pp.cut(ts[1][0], 2, 32)], flat)
        b = rd.read([(3, 40), (0, rd.total)])
        whole = ts[0][0] + b"".join(pp.cut(ts[1][0], 2, 32)) + b"".join(pc.np_split(*TAIL))
        assert b.rc == 0 and b.out == whole[3:43] + whole
        assert rd.set_planes([]) == (0, "") and rd.tensor_info() == []
    finally:
        rd.close()


@pytest.mark.parametrize("case", range(3, len(BAD_PIECES)))
def test_what_a_declaration_refuses_of_sizes(lib, stream, case):
    sizes, pieces, pattern = BAD_PIECES[case]
    rd = pp.PieceReader(lib, _sized(stream, sizes))
    try:
        got, err = rd.set_planes_pieces([1, 2, 4], pieces)
        assert got == EINVAL and re.search(pattern.replace("%s", "tensor"), err), err
        assert rd.tensor_info() == []
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ cursors
def test_cursors_walk_a_tensor_piece_by_piece(lib, stream):
    S, e = 4096, 4
    count = 3 * S + 16
    ts = [(pc.tensor_bytes(1, 33, 5), 1), (pc.tensor_bytes(e, count, 6), e)]
    blob, _, _, qs = pp.container(stream, ts, S)
    rd = pp.PieceReader(lib, blob)
    try:
        assert qs == [1, 4] and rd.set_planes_pieces([1, e], qs) == (0, "")
        rd.set_cache(e * 4 * ec.cc.cost(S, rd.state_bytes))
        windows = [[(1, k * 2048, min(2048, count - k * 2048))] for k in range(7)]
        decoded = 0
        for k, w in enumerate(windows):
            r = rd.read_elements(w, w[0][2] * e, rem=4 * (k % 2))
            _check_read(r, ts, w)
            cs = rd.cache_stats()
            # an even window opens a piece of each plane, an odd one goes on where the even one stopped
            assert (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == ((0, 0, e, 0) if k % 2 == 0 else (0, e, 0, 0)), (k, cs)
            assert r.host_waits == 2 and r.members_decoded == e and r.launches == 1
            decoded += r.decoded_bytes
        assert e * count <= decoded <= e * count + 3 * e * (rc.SLACK - 1), decoded  # every byte once
        assert rd.cache_stats()["cursors"] == 4 * e
        for w in windows:  # the second pass: all hits
            r = rd.read_elements(w, w[0][2] * e)
            _check_read(r, ts, w)
            cs = rd.cache_stats()
            assert (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == (e, 0, 0, 0), cs
            assert r.launches == 0 and r.host_waits == 2 and r.decoded_bytes == 0
        across = [(1, S - 8, 16)]  # two pieces of each plane
        _check_read(rd.read_elements(across, 16 * e), ts, across)
        assert rd.cache_stats()["hits"] == 2 * e
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ damage
def _damaged(lib, oracle, data):
    """(good stream, stream with payload bits flipped in the last tenth of its last chunk whose whole decode FAILS)"""
    good = oracle.encode(data, 1)
    _, p, t = rc.chunks(good)[-1]
    for seed in range(32):
        rng = random.Random(seed)
        bad = bytearray(good)
        for _ in range(40):
            bad[p + t - 1 - rng.randrange(0, t // 10)] ^= 1 << rng.randrange(8)
        rd = rc.EmuReader(lib, bytes(bad))
        try:
            if rd.h and rd.total == len(data) and rd.read([(0, len(data))]).rc == EINVAL:
                return good, bytes(bad)
        finally:
            rd.close()
    raise AssertionError("no seed damages the stream so that its decode fails")


def test_a_damaged_piece_fails_only_the_reads_that_reach_it(lib, oracle, stream):
    n = 60_000  # S: a multiple of 16
    text = _data.text(n, seed=6)
    plane0 = _data.mixed(n, seed=1) + text + _data.random_bytes(16)
    hurt = [(pc.tensor_bytes(8, 17, 9), 8), (pc.np_merge([plane0, _data.random_bytes(2 * n + 16)]), 2)]
    members, qs = pp.members_of(hurt, n)
    assert qs == [1, 3] and members[9] == text
    good, bad = _damaged(lib, oracle, text)
    blobs = [stream(m) for m in members]
    assert blobs[9] == good
    blobs[9] = bad  # plane 0, piece 1 of tensor 1: elements n .. 2 n - 1
    rd = pp.PieceReader(lib, b"".join(blobs))
    try:
        assert rd.h, rd.err
        assert rd.set_planes_pieces([8, 2], qs) == (0, "")
        for ok in ([(1, 100, 900), (0, 3, 14)], [(1, 2 * n, 16), (1, 2 * n + 3, 5)], [(1, n - 8, 16 + n // 2)], [(1, n - 8, 8), (1, 2 * n, 1)]):
            _check_read(rd.read_elements(ok, len(ec.np_elements(hurt, ok)), rem=4), hurt, ok)
        late = [(0, 0, 17), (1, 2 * n - 64, 80)]
        want = len(ec.np_elements(hurt, late))
        r = rd.read_elements(late, want)
        assert r.rc == EINVAL and "member 9," in r.err, r.err
        assert r.dst_len == want
        # the units of the damaged piece are not written; the other tensor and the next piece are
        a, c = ec.np_elements(hurt, late[:1]), ec.np_elements(hurt, [(1, 2 * n, 16)])
        pc.same(r.arena, pc.expect_arena(r.arena_len, [(r.at, a), (r.at + want - len(c), c)]), "the arena")
        ok = [(1, 100, 900), (1, 2 * n + 1, 15)]
        _check_read(rd.read_elements(ok, len(ec.np_elements(hurt, ok))), hurt, ok)
    finally:
        rd.close()
