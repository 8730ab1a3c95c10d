"""Element ranges of DELTA containers read against their bases (orz_amd/csrc/orz_read_elements.h: set_bases, ElementGatherDelta,
ElementGatherDeltaPieces) on the emulation backend: the two kernels alone against a restatement in numpy -- the slice of the delta
XOR the slice of the base, which is the slice of the tensor -- inside poisoned arenas with guard gaps that hold the output AND the
base slices, out of place and in place; and the reader with bases on containers the ORACLE's encoder made of the numpy planes of the
deltas: the bytes, what a read costs against the same read with the bases withdrawn, cursors that outlive a change of bases, and
every refusal, made before anything is launched."""
import ctypes
import re

import pytest

import _basecases as bc
import _deltacases as dc
import _elemcases as ec
import _piececases as pp
import _planecases as pc
from _basecases import EINVAL, LONG, PIECE

FIRSTS = (0, 1, 15, 16, 17)
COUNTS = (0, 1, 15, 16, 17, 33)
REMS = ("0", "4", "8", "e", "1")


@pytest.fixture(scope="module")
def lib():
    return bc.emu_lib()


@pytest.fixture(scope="module")
def stream(oracle):
    """the oracle's stream of some bytes at level 1, remembered"""
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


@pytest.fixture(scope="module")
def mixed():
    return dc.mixed()


def _one(e):
    """one tensor of LONG elements and its base"""
    return [(pc.tensor_bytes(e, LONG, 70 + e), e)], [pc.tensor_bytes(e, LONG, 170 + e)]


def _check(g, ts, ranges, what, skip=()):
    pc.same(g.arena, bc.expect(g, ts, ranges, skip), what)
    assert g.members_after == g.members_before


# ------------------------------------------------------------------------------------------------ the gather alone
def test_the_restatement_and_the_cases():
    ts, bases = _one(2)
    d = dc.deltas(ts, bases)
    assert dc.xor(ec.np_elements(d, [(0, 3, 40)]), ec.np_elements([(bases[0], 2)], [(0, 3, 40)])) == ec.np_elements(ts, [(0, 3, 40)])
    assert d[0][0] != ts[0][0] and LONG == 64 * 16 + 5


@pytest.mark.parametrize("how", REMS)
@pytest.mark.parametrize("e", pc.ELEMS)
def test_gather_equals_the_numpy_slice_xor_the_base_slice(lib, e, how):
    """destination and base at every remainder, independently: 16-byte, dword and byte accesses on either side; planes at 0 and at 1"""
    ts, bases = _one(e)
    for base_how in REMS:
        for plane_rem in (0, 1):
            for first in FIRSTS:
                for count in COUNTS + (LONG - first,):
                    ranges = [(0, first, count)]
                    g = bc.gather(lib, ts, bases, ranges, bc.rem_of(how, e), bc.rem_of(base_how, e), plane_rem)
                    assert g.units == ec.units_of(first, count), (first, count)
                    _check(g, ts, ranges, "the arena (base at %s, planes at %d, first %d, count %d)" % (base_how, plane_rem, first, count))


@pytest.mark.parametrize("how", ["0", "4", "e", "1"])
@pytest.mark.parametrize("e", pc.ELEMS)
def test_gather_in_place(lib, e, how):
    """the arena holds the base slice where the range's bytes go: afterwards the restored elements, and nothing else has changed"""
    ts, bases = _one(e)
    for first in FIRSTS:
        for count in (1, 15, 16, 17, 33, LONG - first):
            ranges = [(0, first, count)]
            g = bc.gather(lib, ts, bases, ranges, bc.rem_of(how, e), in_place=(0,))
            assert g.slices == [(g.at, bc.slice_of([(bases[0], e)], ranges[0]))] and g.before[g.at:g.at + count * e] == g.slices[0][1]
            _check(g, ts, ranges, "the arena (first %d, count %d)" % (first, count))


def _batch(ts, bases, S=0):
    """ec.mixed_batch and, of every tensor, ranges off the unit borders -- and across the pieces' --: with and without a base side
    by side, duplicates among them"""
    ranges = ec.mixed_batch(ts)
    for j, (d, e) in enumerate(ts):
        c = len(d) // e
        if c >= 17:
            ranges += [(j, 1, 16)]
        if c > 1000:
            ranges += [(j, 15, 1000), (j, 30, 5), (j, 16, 64), (j, 15, 1000)]
    assert {(ts[j][1], bases[j] is not None) for j, f, c in ranges if c >= 64} == {(e, h) for e in pc.ELEMS for h in (False, True)}
    assert len(set(ranges)) < len(ranges)
    if S:
        assert any(f // S != (f + c - 1) // S for _, f, c in ranges if c)
    return ranges


@pytest.mark.parametrize("S, plane_rem", [(0, 0), (0, 1), (PIECE, 0)])
def test_gather_of_a_mixed_batch_in_one_launch(lib, mixed, S, plane_rem):
    ts, bases = mixed
    ranges = _batch(ts, bases, S)
    for rem, base_rem in ((0, 0), (4, 8), (2, 0), (0, 3)):
        g = bc.gather(lib, ts, bases, ranges, rem, base_rem, plane_rem, S=S)
        assert g.units == sum(ec.units_of(f, c) for _, f, c in ranges)
        _check(g, ts, ranges, "the arena (output at %d, bases at %d)" % (rem, base_rem))


@pytest.mark.parametrize("S", [0, PIECE])
def test_gather_of_a_batch_with_its_based_ranges_in_place(lib, mixed, S):
    ts, bases = mixed
    ranges = sorted(set(_batch(ts, bases, S)))
    inp = tuple(k for k, (j, f, c) in enumerate(ranges) if bases[j] is not None and c)
    assert len(inp) > 8 and len(inp) < len(ranges)
    g = bc.gather(lib, ts, bases, ranges, 4, S=S, in_place=inp)
    _check(g, ts, ranges, "the arena")


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("S", [0, PIECE])
def test_gather_skips_the_units_of_a_failed_member(lib, mixed, S, in_place):
    """a failed plane (with pieces: a failed piece): its units write nothing -- in place the base slice stays --, the rest is right"""
    ts, bases = mixed
    i, j = (next(k for k, ((d, e), b) in enumerate(zip(ts, bases)) if e == want and len(d) // e > 1000 and b is not None) for want in (2, 4))
    _, qs = pp.members_of(ts, S)
    fm = pp.first_members(ts, qs)
    ranges = [(i, 0, 50), (j, 5, 40), (i, 7, 9), (j, 40, 8)]
    inp = (0, 1, 3) if in_place else ()  # (ranges 0 and 2 overlap: one of them in place)
    if not S:
        g = bc.gather(lib, ts, bases, ranges, 0, 4, bad_member=fm[j] + 2, in_place=inp)
        _check(g, ts, ranges, "the arena", skip=(1, 3))
        return
    # piece 1 of plane 2 holds elements 32 .. 63: range 3 lies in it, and of range 1 the unit of elements 32 .. 44
    g = bc.gather(lib, ts, bases, ranges, 0, 4, S=S, bad_member=fm[j] + 2 * qs[j] + 1, in_place=inp)
    want = bytearray(bc.expect(g, ts, ranges, skip=(3,)))
    o = g.at + g.offs[1] + (32 - 5) * 4
    want[o:o + 13 * 4] = g.before[o:o + 13 * 4]
    pc.same(g.arena, bytes(want), "the arena")
    assert g.members_after == g.members_before


def test_no_ranges_launch_nothing(lib, mixed):
    ts, bases = mixed
    g = bc.gather(lib, ts, bases, [], 0)
    assert g.units == 0 and g.arena == g.before == bytes([pc.POISON]) * len(g.arena)


# ------------------------------------------------------------------------------------------------ the reader
def _open(lib, stream, ts, bases, S=0, cache=0):
    """a reader of the deltas' container, declared, and the bases held out of place at remainders of their own (not yet set)"""
    deltas = dc.deltas(ts, bases)
    if S:
        blob, _, _, qs = pp.container(stream, deltas, S)
    else:
        blob, _, _ = ec.container(stream, deltas)
    rd = bc.BaseReader(lib, blob)
    assert rd.h, rd.err
    if cache:
        rd.set_cache(cache)
    assert (rd.set_planes_pieces([e for _, e in ts], qs) if S else rd.set_planes([e for _, e in ts])) == (0, "")
    return rd


def _cases(S):
    if not S:
        return dc.mixed()
    ts, n = pp.tensors(S), 3 * S + 21  # and of every element size a tensor of four pieces with a base, and one without
    more = [(e, h) for e in pc.ELEMS for h in (False, True)]
    return (ts + [(pc.tensor_bytes(e, n, 40 + 2 * e + h), e) for e, h in more],
            dc.with_bases(ts, seed=31) + [pc.tensor_bytes(e, n, 300 + e) if h else None for e, h in more])


@pytest.fixture(scope="module", params=[0, PIECE])
def opened(request, lib, stream):
    S = request.param
    ts, bases = _cases(S)
    assert {(e, b is not None) for (d, e), b in zip(ts, bases) if len(d) // e > 2 * S + 4} == {(e, h) for e in pc.ELEMS for h in (False, True)}
    rd = _open(lib, stream, ts, bases, S)
    yield S, ts, bases, rd
    rd.close()


def _read(rd, ts, ranges, rem=0):
    return rd.read_elements(ranges, len(ec.np_elements(ts, ranges)), rem=rem)


def _windows(ts, S):
    """of every tensor: all of it, and a window that starts and ends off the unit borders (and the pieces')"""
    out = []
    for j, (d, e) in enumerate(ts):
        c = len(d) // e
        out += [(j, 0, c)] + ([(j, 15, c - 15 - 3)] if c > 40 else [(j, 1, c - 1)] if c > 1 else [])
    return out


@pytest.mark.parametrize("rem", [0, 4, 1])
def test_reads_return_restored_elements_at_the_cost_of_the_read_without_bases(opened, rem):
    S, ts, bases, rd = opened
    deltas = dc.deltas(ts, bases)
    held = bc.Held(ts, bases, rem="e" if rem else 0)
    for ranges in (_windows(ts, S), ec.mixed_batch(ts) if not S else _windows(ts, S)[::-2]):
        assert rd.set_bases(held.addrs) == (0, "") and rd.bases() == held.addrs
        r = _read(rd, ts, ranges, rem)
        assert r.rc == 0, r.err
        assert r.dst_len == r.out_bytes == len(r.out)
        pc.same(r.arena, pc.expect_arena(r.arena_len, [(r.at, ec.np_elements(ts, ranges))]), "the arena")
        assert rd.set_bases([]) == (0, "") and rd.bases() == []
        plain = _read(rd, ts, ranges, rem)
        assert plain.rc == 0 and plain.out == ec.np_elements(deltas, ranges) != r.out
        assert (r.launches, r.host_waits, r.members_decoded, r.decoded_bytes) == (plain.launches, plain.host_waits, plain.members_decoded, plain.decoded_bytes)
        assert r.host_waits == 3 and r.launches == 1
    assert held.untouched()


def test_ranges_of_tensors_without_a_base_read_as_without_bases(opened):
    S, ts, bases, rd = opened
    held = bc.Held(ts, bases)
    ranges = [r for r in _windows(ts, S) if bases[r[0]] is None]
    assert {ts[j][1] for j, _, c in ranges if c} == set(pc.ELEMS)
    assert rd.set_bases(held.addrs) == (0, "")
    r = _read(rd, ts, ranges)
    assert rd.set_bases([]) == (0, "")
    plain = _read(rd, ts, ranges)
    assert r.rc == plain.rc == 0 and r.out == plain.out == ec.np_elements(dc.deltas(ts, bases), ranges) == ec.np_elements(ts, ranges)
    assert (r.launches, r.host_waits, r.decoded_bytes) == (plain.launches, plain.host_waits, plain.decoded_bytes)


def test_a_read_in_place_restores_the_rows_where_the_base_has_them(opened):
    S, ts, bases, rd = opened
    j = max((k for k, b in enumerate(bases) if b is not None), key=lambda k: len(bases[k]))
    e, c = ts[j][1], len(ts[j][0]) // ts[j][1]
    for rem in (0, e):
        (at,), alen = pc.layout([len(bases[j])], [rem])
        arena = pc.Arena(alen, align=16)
        arena.write(at, bases[j])
        addrs = [0] * len(ts)
        addrs[j] = arena.base + at
        assert rd.set_bases(addrs) == (0, "")
        first, count = 17, c - 17 - 2
        r = rd.read_elements([(j, first, count)], raw=(arena.base + at + first * e, count * e))
        assert r.rc == 0 and r.dst_len == count * e and r.untouched, r.err
        want = bases[j][:first * e] + ts[j][0][first * e:(first + count) * e] + bases[j][(first + count) * e:]
        pc.same(arena.bytes(), pc.expect_arena(alen, [(at, want)]), "the arena of the base")
    assert rd.set_bases([]) == (0, "")


def test_cursors_outlive_a_change_of_bases(lib, stream):
    ts = [(pc.tensor_bytes(1, 33, 5), 1), (pc.tensor_bytes(4, 20_000, 6), 4)]
    a, b = pc.tensor_bytes(4, 20_000, 7), pc.tensor_bytes(4, 20_000, 8)
    bases = [None, a]
    rd = _open(lib, stream, ts, bases, cache=0)
    try:
        rd.set_cache(4 * ec.cc.cost(20_000, rd.state_bytes))
        first, second = bc.Held(ts, [None, a]), bc.Held(ts, [None, b], rem="e")
        rg = [(1, 4001, 3000)]
        assert rd.set_bases(first.addrs) == (0, "")
        r = _read(rd, ts, rg)
        assert r.rc == 0 and r.out == ec.np_elements(ts, rg) and r.members_decoded == 4 and r.host_waits == 2
        assert rd.cache_stats()["fresh"] == 4
        assert rd.set_bases(second.addrs) == (0, "")  # (launches nothing, keeps the cursors)
        assert rd.cache_stats()["cursors"] == 4
        r = _read(rd, ts, rg, rem=4)
        cs = rd.cache_stats()
        assert r.rc == 0 and (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == (4, 0, 0, 0)
        assert r.launches == 0 and r.decoded_bytes == 0 and r.members_decoded == 0 and r.host_waits == 2
        assert r.out == dc.xor(dc.xor(ec.np_elements(ts, rg), ec.np_elements([(b"", 1), (a, 4)], rg)), ec.np_elements([(b"", 1), (b, 4)], rg))
        assert first.untouched() and second.untouched()
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ refusals
def _refused_read(r, pattern):
    assert r.rc == EINVAL and re.search(pattern, r.err), (r.rc, r.err)
    assert r.untouched and r.launches == 0 and r.host_waits == 0


def test_what_set_bases_refuses(lib, stream, opened):
    S, ts, bases, rd = opened
    T = len(ts)
    held = bc.Held(ts, bases)
    blob = b"".join(stream(m) for m in pp.members_of(dc.deltas(ts[:3], bases[:3]), 0)[0])
    plain = bc.BaseReader(lib, blob)
    try:
        assert plain.set_bases([0] * 3) == (EINVAL, "invalid argument: the container is not declared as planes of tensors")
        assert plain.set_bases([]) == (0, "")  # (nothing to withdraw)
    finally:
        plain.close()
    assert rd.set_bases(held.addrs) == (0, "")
    for addrs, null, pattern in ((held.addrs[:-1], False, r"%d bases for %d tensors" % (T - 1, T)), (held.addrs + [0], False, r"%d bases for %d tensors" % (T + 1, T)),
                                 (held.addrs, True, r"bases without their array")):
        got, err = rd.set_bases(addrs, null=null)
        assert got == EINVAL and re.search(pattern, err), err
        assert rd.bases() == held.addrs  # nothing changed
    # a base whose bytes wrap the address space; one that ends with it does not; that of a tensor of no elements is not looked at
    j = max((k for k, b in enumerate(bases) if b is not None), key=lambda k: len(bases[k]))
    empty = next(k for k, (d, _) in enumerate(ts) if not d)
    wrap = list(held.addrs)
    wrap[j] = (1 << 64) - len(bases[j]) + 1
    got, err = rd.set_bases(wrap)
    assert got == EINVAL and re.search(r"the base of tensor %d \(%d bytes\) wraps the address space" % (j, len(bases[j])), err), err
    assert rd.bases() == held.addrs
    wrap[j] -= 1
    wrap[empty] = (1 << 64) - 1
    assert rd.set_bases(wrap) == (0, "")
    assert rd.bases() == [0 if k == empty else a for k, a in enumerate(wrap)]
    # a refused declaration keeps the bases, a successful one withdraws them
    elems = [e for _, e in ts]
    assert rd.set_bases(held.addrs) == (0, "")
    assert rd.set_planes(elems + [1])[0] == EINVAL and rd.bases() == held.addrs
    assert rd.set_planes_pieces(elems, [0] * T)[0] == EINVAL and rd.bases() == held.addrs
    r = _read(rd, ts, [(j, 0, 5)])
    assert r.rc == 0 and r.out == ts[j][0][:5 * ts[j][1]]
    qs = pp.members_of(ts, S)[1]
    assert (rd.set_planes_pieces(elems, qs) if S else rd.set_planes(elems)) == (0, "")
    assert rd.bases() == []
    r = _read(rd, ts, [(j, 0, 5)])
    assert r.rc == 0 and r.out == dc.deltas(ts, bases)[j][0][:5 * ts[j][1]]


def test_a_base_slice_may_overlap_the_output_only_as_its_own_destination(opened):
    S, ts, bases, rd = opened
    j = max((k for k, b in enumerate(bases) if b is not None), key=lambda k: len(bases[k]))
    i = next(k for k, b in enumerate(bases) if b is None and len(ts[k][0]) >= 64)
    e, c = ts[j][1], len(ts[j][0]) // ts[j][1]
    (at,), alen = pc.layout([len(bases[j]) + 64], [0])
    arena = pc.Arena(alen, align=16)
    arena.write(at, bases[j])
    before = arena.bytes()
    addrs = [0] * len(ts)

    def refused(ranges, base_at, dst_at, k):
        addrs[j] = arena.base + base_at
        assert rd.set_bases(addrs) == (0, "")
        r = rd.read_elements(ranges, raw=(arena.base + dst_at, len(ec.np_elements(ts, ranges))))
        _refused_read(r, r"the base slice of range %d \(tensor %d\) overlaps the output buffer other than as the range's own destination" % (k, j))
        assert arena.bytes() == before and rd.bases() == addrs

    first, count = 16, 20
    # shifted by one element, either way
    refused([(j, first, count)], at, at + (first + 1) * e, 0)
    refused([(j, first, count)], at, at + (first - 1) * e, 0)
    # the slice is another range's destination: the range in front of it takes its place
    refused([(i, 0, 8), (j, first, count)], at, at + first * e, 1)
    # two identical ranges cannot both be read in place
    refused([(j, first, count), (j, first, count)], at, at + first * e, 1)
    # a slice inside the output's capacity that begins where the bytes written end is no overlap; the reader is as usable as before
    addrs[j] = arena.base + at
    assert rd.set_bases(addrs) == (0, "")
    r = rd.read_elements([(j, 2 * first, first)], raw=(arena.base + at + first * e, (c - first) * e))
    assert r.rc == 0 and r.dst_len == first * e, r.err
    want = bases[j][:first * e] + ts[j][0][2 * first * e:3 * first * e] + bases[j][2 * first * e:]
    pc.same(arena.bytes(), pc.expect_arena(alen, [(at, want)]), "the arena")
    assert rd.set_bases([]) == (0, "")
