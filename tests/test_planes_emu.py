"""Tensors as byte planes (orz_amd/csrc/orz_planes.h) on the emulation backend: PlaneSplit and PlaneMerge against a restatement
in numpy inside poisoned arenas with guard gaps, and decode_members_planes on containers the ORACLE's encoder made of the numpy
planes -- the bytes, the launches and host waits against decode_members_scatter's, and every refusal made before a byte of any
destination is written."""
import random

import pytest

import _data
import _planecases as pc
import _scattercases as sc
from _planecases import EINVAL, ENOMEM, GUARD, POISON


@pytest.fixture(scope="module")
def lib():
    return pc.emu_lib()


@pytest.fixture(scope="module")
def mixed():
    return pc.mixed_tensors()


@pytest.fixture(scope="module")
def stream(oracle):
    """the oracle's stream of some bytes at level 1, remembered"""
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


def _rems(tensors, how):
    """the interleaved buffers' addresses modulo 16: all 0, all 1, each its element size, all 8"""
    return [{"0": 0, "1": 1, "e": e % 16, "8": 8}[how] for _, e in tensors]


# ------------------------------------------------------------------------------------------------ the kernels
def test_the_shared_cases_cover_what_they_claim(mixed):
    assert {(e, len(d) // e) for d, e in mixed} >= {(e, c) for e in pc.ELEMS for c in pc.COUNTS}
    assert sum(1 for d, _ in mixed if not d) >= len(pc.COUNTS)
    for data, e in mixed:
        assert pc.np_merge(pc.np_split(data, e)) == data
    assert pc.np_split(bytes(range(8)), 4) == [bytes([0, 4]), bytes([1, 5]), bytes([2, 6]), bytes([3, 7])]


@pytest.mark.parametrize("how", ["0", "1", "e", "8"])
def test_split_equals_the_numpy_planes(lib, mixed, how):
    sizes = [len(d) for d, _ in mixed]
    inter_offs, inter_len = pc.layout(sizes, _rems(mixed, how))
    inter = pc.Arena(inter_len, align=16)
    for (d, _), o in zip(mixed, inter_offs):
        inter.write(o, d)
    assert all((inter.base + o) % 16 == r for o, r in zip(inter_offs, _rems(mixed, how)))
    before = inter.bytes()
    stage_offs, stage_len = pc.staging_layout(mixed)
    stage = pc.Arena(stage_len, align=256)
    units = pc.move(lib, False, mixed, inter, inter_offs, stage, stage_offs)
    assert units == sum((len(d) // e + 15) // 16 for d, e in mixed if e > 1)
    pieces = []
    for (d, e), so in zip(mixed, stage_offs):
        if e > 1:
            assert lib.emu_plane_pitch(len(d) // e) == pc.pitch(len(d) // e)
            pieces += [(so + p * pc.pitch(len(d) // e), pl) for p, pl in enumerate(pc.np_split(d, e))]
    # nothing but the planes' `count` bytes changes in the staging buffer: the padding up to the pitch stays poison too
    pc.same(stage.bytes(), pc.expect_arena(stage_len, pieces), "the staging buffer")
    assert inter.bytes() == before


@pytest.mark.parametrize("how", ["0", "1", "e", "8"])
def test_merge_is_the_inverse_of_split(lib, mixed, how):
    stage_offs, stage_len = pc.staging_layout(mixed)
    stage = pc.Arena(stage_len, align=256)
    for (d, e), so in zip(mixed, stage_offs):
        if e > 1:
            for p, pl in enumerate(pc.np_split(d, e)):
                stage.write(so + p * pc.pitch(len(d) // e), pl)
    before = stage.bytes()
    caps = [len(d) + 9 for d, _ in mixed]  # (room behind each destination's size: it must stay poison)
    offs, total = pc.layout(caps, _rems(mixed, how), reverse=True)
    arena = pc.Arena(total, align=16)
    pc.move(lib, True, mixed, arena, offs, stage, stage_offs)
    pc.same(arena.bytes(), pc.expect_arena(total, [(o, d) for (d, e), o in zip(mixed, offs) if e > 1]), "the arena of destinations")
    assert stage.bytes() == before


def test_an_empty_table_launches_nothing(lib):
    only_bytes = [(b"abc", 1), (b"", 1)]
    stage = pc.Arena(512)
    assert pc.move(lib, False, only_bytes, stage, [0, 0], stage, [None, None]) == 0
    assert stage.bytes() == bytes([POISON]) * 512


# ------------------------------------------------------------------------------------------------ the decode driver
def _container(stream, tensors, layout):
    blobs = [stream(pl) for pl in pc.planes_of(tensors)]
    if layout == "concatenation":
        return b"".join(blobs), None, blobs
    order = list(range(len(blobs)))
    random.Random(len(blobs)).shuffle(order)
    blob, table = pc.table_of(blobs, order=order)
    return blob, table, blobs


def _places(tensors, room=9):
    """destinations carved in REVERSE order out of the arena at multiples of 16 plus the element size (only tensors of bytes are
    unaligned for their type), `room` bytes of capacity behind each size"""
    caps = [len(d) + room for d, _ in tensors]
    offs, total = pc.layout(caps, [0 if k % 2 else e % 16 for k, (_, e) in enumerate(tensors)], reverse=True)
    return offs, caps, total


def _scatter_twin(blob, table, blobs_planes):
    """decode_members_scatter on the same container, a destination per member: (launches, host_waits)"""
    caps = [len(p) for p in blobs_planes]
    offs, total = sc.reverse_layout(caps, guard=3)
    r = sc.scatter(sc.emu_lib(), blob, table, [(o if c else None, c) for o, c in zip(offs, caps)], total)
    assert r.rc == 0, r.err
    return r.launches, r.host_waits


@pytest.mark.parametrize("layout", ["concatenation", "permuted table", "host container"])
def test_planes_decode_into_the_original_bytes(lib, mixed, stream, layout):
    blob, table, _ = _container(stream, mixed, "concatenation" if layout == "concatenation" else "table")
    elems = [e for _, e in mixed]
    offs, caps, total = _places(mixed)
    r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), elems, total, on_device=layout != "host container")
    assert r.rc == 0, r.err
    assert r.members == sum(elems) and r.out_lens == [len(d) for d, _ in mixed]
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(mixed, offs)]), "the arena of destinations")
    launches, waits = _scatter_twin(blob, table, pc.planes_of(mixed))
    assert r.launches == launches == 1
    assert r.host_waits == waits + (layout == "host container") == 4 + (table is not None) + (layout == "host container")
    # the output does not depend on what the buffers held
    z = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), elems, total, fill=0x00)
    pc.same(z.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(mixed, offs)], fill=0x00), "the zeroed arena")


def test_host_waits_do_not_grow_with_the_tensors(lib, stream):
    waits = {}
    for n in (3, 40):
        tensors = [(pc.tensor_bytes(pc.ELEMS[k % 4], 5 + k % 7, k), pc.ELEMS[k % 4]) for k in range(n)]
        blob, table, _ = _container(stream, tensors, "table")
        offs, caps, total = _places(tensors, room=0)
        r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), [e for _, e in tensors], total)
        assert r.rc == 0, r.err
        pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(tensors, offs)]), "the arena of %d tensors" % n)
        waits[n] = r.host_waits
        assert _scatter_twin(blob, table, pc.planes_of(tensors)) == (r.launches, r.host_waits)
    assert waits[3] == waits[40] == 5


def test_two_members_in_flight_give_the_same_bytes(lib, stream):
    tensors = [t for t in pc.mixed_tensors(counts=(17, 1029))]
    blob, table, _ = _container(stream, tensors, "table")
    elems = [e for _, e in tensors]
    offs, caps, total = _places(tensors)
    r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), elems, total, slots=2)
    assert r.rc == 0, r.err
    assert r.launches == (sum(elems) + 1) // 2 > 1
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(tensors, offs)]), "the arena of destinations")


def test_sizing_call_decodes_nothing(lib, mixed, stream):
    elems = [e for _, e in mixed]
    for layout in ("concatenation", "table"):
        blob, table, _ = _container(stream, mixed, layout)
        r = pc.decode_planes(lib, blob, table, [(None, 0)] * len(mixed), elems, 64, sizing=True)
        assert r.rc == 0, r.err
        assert r.members == sum(elems) and r.out_lens == [len(d) for d, _ in mixed] and r.launches == 0
        assert r.arena == bytes([POISON]) * 64
    e = pc.decode_planes(lib, b"", None, [], [], 16)
    assert e.rc == 0 and e.members == 0 and e.launches == 0


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def small(stream):
    """(tensors, container, table): int16 x 17, bytes x 5, int64 x 16, empty int32, int32 x 33 -- 2 + 1 + 8 + 4 + 4 members"""
    tensors = [(pc.tensor_bytes(e, c, 70 + k), e) for k, (e, c) in enumerate([(2, 17), (1, 5), (8, 16), (4, 0), (4, 33)])]
    blob, table = pc.table_of([stream(pl) for pl in pc.planes_of(tensors)])
    return tensors, blob, table


def _untouched(r, total):
    return r.launches == 0 and r.arena == bytes([POISON]) * total


def test_a_wrong_plane_count_is_refused(lib, small):
    tensors, blob, table = small
    offs, caps, total = _places(tensors)
    for elems in ([2, 1, 8, 4, 2], [2, 1, 8, 4, 8], [2, 1, 8, 4]):
        r = pc.decode_planes(lib, blob, table, list(zip(offs, caps))[:len(elems)], elems, total)
        assert r.rc == EINVAL and "%d planes for 19 members" % sum(elems) in r.err and _untouched(r, total), r.err


def test_an_element_size_of_three_is_refused(lib, small):
    tensors, blob, table = small
    offs, caps, total = _places(tensors)
    for bad in (3, 0, 16):
        r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), [2, 1, 8, 4, bad], total)
        assert r.rc == EINVAL and "destination 4" in r.err and " %d bytes" % bad in r.err and _untouched(r, total), r.err


def test_planes_of_unequal_size_are_refused(lib, small, stream):
    tensors, blob, table = small
    offs, caps, total = _places(tensors, room=64)
    # the int64 tensor's plane 5 (member 3 + 5) one byte longer than its fellows
    blobs = [stream(pl) for pl in pc.planes_of(tensors)]
    blobs[8] = stream(pc.planes_of(tensors)[8] + b"x")
    blob2, table2 = pc.table_of(blobs)
    r = pc.decode_planes(lib, blob2, table2, list(zip(offs, caps)), [e for _, e in tensors], total)
    assert r.rc == EINVAL and "destination 2" in r.err and "member 8 " in r.err and _untouched(r, total), r.err
    # the same members read as other element sizes: 2 + 1 + 8 + 4 + 4 as 1 + 2 + ...: members 1 (17 bytes) and 2 (5 bytes) differ
    r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), [1, 2, 8, 4, 4], total)
    assert r.rc == EINVAL and "destination 1" in r.err and "member 2 " in r.err and _untouched(r, total), r.err


def test_a_capacity_one_byte_short_writes_nothing(lib, small):
    tensors, blob, table = small
    elems = [e for _, e in tensors]
    for short in (0, 1, 2, 4):
        offs, caps, total = _places(tensors, room=0)
        caps[short] -= 1
        r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), elems, total)
        assert r.rc == ENOMEM and "destination %d " % short in r.err and _untouched(r, total), r.err
        assert r.out_lens == [len(d) for d, _ in tensors]  # (the sizes come back with the refusal)
    offs, caps, total = _places(tensors, room=0)
    r = pc.decode_planes(lib, blob, table, [(o, max(c - 1, 0)) for o, c in zip(offs, caps)], elems, total)
    assert r.rc == ENOMEM and "destination 0 " in r.err and _untouched(r, total)  # the FIRST short one is named


def test_overlapping_destinations_are_refused(lib, small):
    tensors, blob, table = small
    elems = [e for _, e in tensors]
    offs, caps, total = _places(tensors)
    for a, b in ((0, 2), (2, 4), (1, 0)):
        o = list(offs)
        o[a] = offs[b] + caps[b] - 1  # the last byte of b's capacity
        r = pc.decode_planes(lib, blob, table, list(zip(o, caps)), elems, total + max(caps))
        assert r.rc == EINVAL and "overlap" in r.err and _untouched(r, total + max(caps)), (a, b, r.err)
    o = list(offs)
    o[3] = offs[0] + 5  # the empty tensor's destination may lie anywhere
    r = pc.decode_planes(lib, blob, table, list(zip(o, caps)), elems, total)
    assert r.rc == 0, r.err


def test_a_destination_inside_the_container_is_refused(lib, small):
    tensors, blob, table = small
    elems = [e for _, e in tensors]
    offs, caps, total = _places(tensors)
    src_at = total + max(caps)
    for k, o1 in ((2, src_at + 10), (1, src_at - caps[1] + 1), (0, src_at + len(blob) - 1)):
        o = list(offs)
        o[k] = o1
        r = pc.decode_planes(lib, blob, table, list(zip(o, caps)), elems, src_at + len(blob) + max(caps), src_at=src_at)
        assert r.rc == EINVAL and "container" in r.err and "destination %d " % k in r.err and r.launches == 0, r.err
        assert r.arena[:total] == bytes([POISON]) * total and r.arena[src_at:src_at + len(blob)] == blob
    r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), elems, src_at + len(blob) + GUARD, src_at=src_at)
    assert r.rc == 0, r.err


def test_a_damaged_plane_is_named(lib, stream):
    tensors = [(pc.tensor_bytes(2, 40, 1), 2), (bytes(_data.text(4 * 4097, seed=2)), 4), (pc.tensor_bytes(1, 100, 3), 1)]
    blobs = [stream(pl) for pl in pc.planes_of(tensors)]
    bad = bytearray(blobs[4])  # plane 2 of the second tensor
    rng = random.Random(4)
    for _ in range(40):  # payload bits in the last tenth of the stream, in front of its EOF byte: the framing stays whole
        bad[len(bad) - 6 - rng.randrange(len(bad) // 10)] ^= 1 << rng.randrange(8)
    blobs[4] = bytes(bad)
    blob, table = pc.table_of(blobs)
    offs, caps, total = _places(tensors, room=300)
    r = pc.decode_planes(lib, blob, table, list(zip(offs, caps)), [e for _, e in tensors], total)
    assert r.rc == EINVAL and "(member 4," in r.err, r.err
    # the guards, and what lies behind each destination's size, are intact; the undamaged tensors hold their bytes
    want = pc.expect_arena(total, [(o, d) for (d, _), o in zip(tensors, offs)])
    lo, hi = offs[1], offs[1] + len(tensors[1][0])
    assert r.arena[:lo] == want[:lo] and r.arena[hi:] == want[hi:]
