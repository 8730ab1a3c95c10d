"""Element ranges of plane-encoded tensors (orz_amd/csrc/orz_read_elements.h) on the emulation backend: ElementGather alone
against a restatement in numpy inside poisoned arenas with guard gaps, and the reader's new calls on containers the ORACLE's
encoder made of the numpy planes -- the bytes, what a read costs against the byte-range read of the same planes, the cursors, and
every refusal made before anything is launched.

One refusal of the contract has no case here: lengths whose sum overflows 64 bits.  A plane holds less than 2^32 bytes, so a valid
range asks for less than 2^35 bytes and the sum needs 2^29 ranges to overflow."""
import random

import pytest

import _data
import _elemcases as ec
import _planecases as pc
import _rangecases as rc
from _elemcases import EINVAL, ENOMEM, LONG, POISON

FIRSTS = (0, 1, 15, 16, 17)
COUNTS = (0, 1, 15, 16, 17, 33)
REMS = ("0", "1", "e", "4", "8")


@pytest.fixture(scope="module")
def lib():
    return ec.emu_lib()


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
def ts():
    return ec.tensors()


@pytest.fixture(scope="module")
def reader(lib, stream, ts):
    """the shared cases as one concatenation in "device" memory, declared"""
    blob, _, _ = ec.container(stream, ts)
    rd = ec.ElemReader(lib, blob)
    assert rd.h, rd.err
    assert rd.set_planes([e for _, e in ts]) == (0, "")
    yield rd
    rd.close()


def _rem(how, e):
    return {"0": 0, "1": 1, "e": e % 16, "4": 4, "8": 8}[how]


def _check_read(r, ts, ranges):
    """a successful read: the bytes, and nothing else in the arena"""
    want = ec.np_elements(ts, ranges)
    assert r.rc == 0, r.err
    assert r.dst_len == len(want) == r.out_bytes and r.ranges == len(ranges)
    pc.same(r.arena, pc.expect_arena(r.arena_len, [(r.at, want)]), "the arena")


# ------------------------------------------------------------------------------------------------ the gather alone
def test_the_shared_cases_cover_what_they_claim(ts):
    assert {(e, len(d) // e) for d, e in ts} >= {(e, c) for e in pc.ELEMS for c in (0, 1, 15, 16, 17)} | {(e, LONG) for e in (2, 4, 8)}
    assert sum(1 for d, _ in ts if not d) >= 5
    batch = ec.mixed_batch(ts)
    assert {ts[j][1] for j, _, _ in batch} == {1, 2, 4, 8} and any(c == 0 for _, _, c in batch)
    assert len(set(batch)) < len(batch) and [j for j, _, _ in batch] != sorted(j for j, _, _ in batch)
    assert ec.np_elements([(bytes(range(12)), 4)], [(0, 1, 2)]) == bytes(range(4, 12))


@pytest.mark.parametrize("how", REMS)
@pytest.mark.parametrize("e", pc.ELEMS)
def test_gather_equals_the_numpy_slice(lib, e, how):
    one = [(pc.tensor_bytes(e, LONG, 70 + e), e)]
    rem = _rem(how, e)
    for first in FIRSTS:
        for count in COUNTS + (LONG - first,):
            ranges = [(0, first, count)]
            units, arena, at, before, after = ec.gather(lib, one, ranges, rem)
            assert units == ec.units_of(first, count), (first, count)
            pc.same(arena, pc.expect_arena(len(arena), [(at, ec.np_elements(one, ranges))]), "the arena (first %d, count %d)" % (first, count))
            assert after == before


@pytest.mark.parametrize("plane_rem", [0, 1, 8])
def test_gather_of_many_ranges_and_tensors_in_one_launch(lib, ts, plane_rem):
    """every first and count of every long tensor, the mixed batch between them: the destinations' addresses fall as they fall;
    planes at other addresses than multiples of 16 go byte by byte"""
    ranges = ec.mixed_batch(ts)
    for e in (2, 4, 8):
        j = ec.index_of(ts, e, LONG)
        ranges += [(j, first, count) for first in FIRSTS for count in COUNTS + (LONG - first,)]
    random.Random(3).shuffle(ranges)
    units, arena, at, before, after = ec.gather(lib, ts, ranges, 0, plane_rem=plane_rem)
    assert units == sum(ec.units_of(f, c) for _, f, c in ranges)
    pc.same(arena, pc.expect_arena(len(arena), [(at, ec.np_elements(ts, ranges))]), "the arena")
    assert after == before


def test_gather_skips_a_tensor_with_a_failed_plane(lib, ts):
    j4, j2 = ec.index_of(ts, 4, LONG), ec.index_of(ts, 2, LONG)
    ranges = [(j2, 0, 50), (j4, 5, 40), (j2, 7, 9)]
    units, arena, at, _, _ = ec.gather(lib, ts, ranges, 0, bad_plane=ec.first_members(ts)[j4] + 2)
    assert units == 4 + 3 + 1
    a, c = ec.np_elements(ts, ranges[:1]), ec.np_elements(ts, ranges[2:])
    pc.same(arena, pc.expect_arena(len(arena), [(at, a), (at + len(a) + 160, c)]), "the arena")


def test_no_ranges_launch_nothing(lib, ts):
    units, arena, _, _, _ = ec.gather(lib, ts, [], 0)
    assert units == 0 and arena == bytes([POISON]) * len(arena)


# ------------------------------------------------------------------------------------------------ reads
def test_info(reader, ts):
    assert reader.members == sum(e for _, e in ts)
    assert reader.tensor_info() == [(len(d) // e, e) for d, e in ts]


@pytest.mark.parametrize("how", ["0", "1", "4"])
def test_a_mixed_batch_in_one_call(reader, ts, how):
    ranges = ec.mixed_batch(ts)
    r = reader.read_elements(ranges, len(ec.np_elements(ts, ranges)), rem=_rem(how, 1))
    _check_read(r, ts, ranges)
    touched = {j for j, _, c in ranges if c}
    assert r.members_decoded == sum(ts[j][1] for j in touched) and r.launches == 1 and r.host_waits == 3


def test_a_tensor_of_single_bytes_between_others(reader, ts):
    b17 = ec.index_of(ts, 1, 17)
    ranges = [(ec.index_of(ts, 4, LONG), 100, 20), (b17, 0, 17), (ec.index_of(ts, 8, 17), 0, 17), (b17, 16, 1)]
    _check_read(reader.read_elements(ranges, len(ec.np_elements(ts, ranges)), rem=8), ts, ranges)


def test_whole_tensors_equal_decode_members_planes(reader, stream, ts):
    blob, _, _ = ec.container(stream, ts)
    sizes = [len(d) for d, _ in ts]
    offs, total = pc.layout(sizes, [0] * len(ts))
    whole = pc.decode_planes(pc.emu_lib(), blob, None, list(zip(offs, sizes)), [e for _, e in ts], total)
    assert whole.rc == 0, whole.err
    ranges = [(j, 0, len(d) // e) for j, (d, e) in enumerate(ts)]
    r = reader.read_elements(ranges, sum(sizes))
    _check_read(r, ts, ranges)
    assert r.out == b"".join(whole.arena[o:o + s] for o, s in zip(offs, sizes))
    assert r.members_decoded == sum(e for d, e in ts if d)


@pytest.mark.parametrize("e", [2, 4, 8])
def test_the_cost_follows_what_is_asked(reader, ts, e):
    """a range that ends at element 40 of LONG: e planes, each decoded up to byte 40 and less than one item further -- exactly what
    the byte-range read of the same planes costs"""
    j = ec.index_of(ts, e, LONG)
    ranges = [(j, 8, 32)]
    r = reader.read_elements(ranges, 32 * e)
    _check_read(r, ts, ranges)
    assert r.members_decoded == e
    lengths = [len(pl) for pl in pc.planes_of(ts)]
    expanded = ec.expand(ts, ranges, reader.member_offsets)
    assert len(expanded) == e
    rc.check_decoded_bytes(r.decoded_bytes, expanded, lengths)
    assert r.decoded_bytes < e * LONG
    b = reader.read(expanded)
    assert b.rc == 0 and b.out == b"".join(pl[8:40] for pl in pc.np_split(ts[j][0], e))
    assert (r.launches, r.members_decoded, r.host_waits, r.decoded_bytes) == (b.launches, b.members_decoded, b.host_waits, b.decoded_bytes)
    assert r.host_waits == 3


@pytest.mark.parametrize("how", ["concatenation", "permuted table", "host container"])
def test_other_containers(lib, stream, ts, how):
    blob, table, _ = ec.container(stream, ts, "table" if how == "permuted table" else "concatenation")
    rd = ec.ElemReader(lib, blob, table=table, on_device=how != "host container")
    try:
        assert rd.h, rd.err
        assert rd.set_planes([e for _, e in ts]) == (0, "")
        ranges = ec.mixed_batch(ts)
        r = rd.read_elements(ranges, len(ec.np_elements(ts, ranges)), rem=4)
        _check_read(r, ts, ranges)
        assert r.host_waits == 3
    finally:
        rd.close()


def test_two_slots_give_the_same_bytes_over_several_launches(reader, ts):
    ranges = ec.mixed_batch(ts)
    r = reader.read_elements(ranges, len(ec.np_elements(ts, ranges)), slots=2)
    _check_read(r, ts, ranges)
    assert r.launches == (r.members_decoded + 1) // 2 > 1 and r.host_waits == 3


def test_declaring_planes_leaves_byte_reads_as_they_were(lib, stream, reader, ts):
    blob, _, _ = ec.container(stream, ts)
    plain = ec.ElemReader(lib, blob)
    try:
        total = reader.total
        ranges = [(0, total), (total - 5000, 4000), (17, 0), (3, 1000)]
        a, b = reader.read(ranges), plain.read(ranges)
        assert a.rc == b.rc == 0 and a.out == b.out == b"".join(b"".join(pc.planes_of(ts))[o:o + n] for o, n in ranges)
        assert (a.launches, a.members_decoded, a.decoded_bytes, a.host_waits) == (b.launches, b.members_decoded, b.decoded_bytes, b.host_waits)
        assert a.host_waits == 3
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------------ cursors
WALK = 20_000


@pytest.fixture(scope="module")
def walked(stream):
    return [(pc.tensor_bytes(1, 33, 5), 1), (pc.tensor_bytes(4, WALK, 6), 4)]


def test_cursors_walk_a_tensor_once(lib, stream, walked):
    blob, _, _ = ec.container(stream, walked)
    rd = ec.ElemReader(lib, blob)
    try:
        assert rd.set_planes([1, 4]) == (0, "")
        rd.set_cache(4 * ec.cc.cost(WALK, rd.state_bytes))
        windows = [[(1, k * 4000, 4000)] for k in range(5)]
        decoded = 0
        for k, w in enumerate(windows):
            r = rd.read_elements(w, 16_000, rem=4 * (k % 2))
            _check_read(r, walked, w)
            cs = rd.cache_stats()
            assert (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == ((0, 0, 4, 0) if k == 0 else (0, 4, 0, 0)), cs
            assert r.host_waits == 2 and r.members_decoded == 4 and r.launches == 1
            decoded += r.decoded_bytes
        assert 4 * WALK <= decoded <= 4 * WALK + 4 * (rc.SLACK - 1), decoded  # each plane once, at most one item further
        for w in windows:  # the second pass: all hits
            r = rd.read_elements(w, 16_000)
            _check_read(r, walked, w)
            cs = rd.cache_stats()
            assert (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == (4, 0, 0, 0), cs
            assert r.launches == 0 and r.host_waits == 2 and r.decoded_bytes == 0 and r.members_decoded == 0
        # the byte tensor has no cursor yet and the budget no room: it is decoded and nothing is kept
        r = rd.read_elements([(0, 1, 30), (1, 19_990, 10)], 70)
        _check_read(r, walked, [(0, 1, 30), (1, 19_990, 10)])
        cs = rd.cache_stats()
        assert (cs["hits"], cs["uncached"], cs["cursors"]) == (4, 1, 4) and r.host_waits == 2
        rd.set_cache(0)  # read()'s behaviour again
        r = rd.read_elements(windows[1], 16_000)
        _check_read(r, walked, windows[1])
        assert r.host_waits == 3 and r.members_decoded == 4 and r.launches == 1
        assert rd.cache_stats() == dict.fromkeys(ec.cc.STAT_NAMES, 0)
        rc.check_decoded_bytes(r.decoded_bytes, ec.expand(walked, windows[1], rd.member_offsets), [len(p) for p in pc.planes_of(walked)])
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ refusals
def _refused(r, code, pattern):
    import re

    assert r.rc == code and re.search(pattern, r.err), (r.rc, r.err)
    assert r.untouched and r.launches == 0 and r.host_waits == 0


def test_refusals_come_before_any_launch(lib, stream, reader, ts):
    j4 = ec.index_of(ts, 4, LONG)
    T = len(ts)
    _refused(reader.read_elements([(0, 0, 1)], 64, null_arrays=True), EINVAL, "arrays")
    _refused(reader.read_elements([(j4, 0, 4), (T, 0, 0)], 64), EINVAL, r"range 1 names tensor %d of %d" % (T, T))
    _refused(reader.read_elements([(j4, 0, 4), (j4, 0, 4), (j4, LONG - 3, 4)], 64), EINVAL, r"range 2 \(tensor %d, first %d, count 4\).*%d elements" % (j4, LONG - 3, LONG))
    _refused(reader.read_elements([(j4, LONG + 1, 0)], 64), EINVAL, "range 0 ")
    _refused(reader.read_elements([(j4, (1 << 64) - 1, 2)], 64), EINVAL, "range 0 ")
    _refused(reader.read_elements([(j4, 2, (1 << 64) - 1)], 64), EINVAL, "range 0 ")
    inside = (ec.ctypes.addressof(reader.src) + 3, 16)
    _refused(reader.read_elements([(j4, 0, 4)], 64, raw=inside), EINVAL, "overlap")
    r = reader.read_elements([(j4, 0, 4), (j4, 9, 3)], cap=27)
    _refused(r, ENOMEM, "27 bytes is too small for 28")
    assert r.dst_len == 28
    for ranges in ([], [(j4, 5, 0), (0, 0, 0), (j4, LONG, 0)]):
        r = reader.read_elements(ranges, 64)
        assert r.rc == 0 and r.dst_len == 0 and r.untouched and r.launches == 0 and r.host_waits == 0
    # the reader is as usable as before
    _check_read(reader.read_elements([(j4, 9, 3)], 12), ts, [(j4, 9, 3)])
    # no declaration: a reader of its own, and this one after the declaration is withdrawn
    blob, _, _ = ec.container(stream, ts)
    plain = ec.ElemReader(lib, blob)
    try:
        assert plain.tensor_info() == []
        _refused(plain.read_elements([(0, 0, 0)], 64), EINVAL, "not declared")
        assert plain.set_planes([e for _, e in ts]) == (0, "")
        _check_read(plain.read_elements([(j4, 9, 3)], 12), ts, [(j4, 9, 3)])
        assert plain.set_planes([]) == (0, "") and plain.tensor_info() == []
        _refused(plain.read_elements([(j4, 9, 3)], 64), EINVAL, "not declared")
    finally:
        plain.close()


def test_what_set_planes_refuses(lib, stream):
    small = [(pc.tensor_bytes(2, 16, 1), 2), (pc.tensor_bytes(4, 17, 2), 4), (pc.tensor_bytes(1, 5, 3), 1)]  # members of 16, 16, 17 x 4, 5 bytes
    blob, _, _ = ec.container(stream, small)
    rd = ec.ElemReader(lib, blob)
    try:
        assert rd.members == 7
        assert rd.set_planes([2, 4, 1]) == (0, "")
        info = rd.tensor_info()
        assert info == [(16, 2), (17, 4), (5, 1)]
        for elems, null, pattern in (([2, 3, 1, 1], False, r"tensor 1 has elements of 3 bytes"), ([2, 4, 16], False, r"tensor 2 has elements of 16 bytes"),
                                     ([0, 2, 4, 1], False, r"tensor 0 has elements of 0 bytes"), ([2, 4], False, r"6 planes for 7 members"),
                                     ([2, 4, 1, 1], False, r"8 planes for 7 members"), ([4, 2, 1], False, r"tensor 0 differ.*member 2 decodes to 17 bytes, member 0 to 16"),
                                     ([2, 4, 1], True, r"without element sizes")):
            got, err = rd.set_planes(elems, null=null)
            import re

            assert got == EINVAL and re.search(pattern, err), (elems, err)
            assert rd.tensor_info() == info  # nothing changed
            _check_read(rd.read_elements([(1, 1, 16), (2, 0, 5)], 69), small, [(1, 1, 16), (2, 0, 5)])
        assert rd.set_planes([1] * 7) == (0, "")  # every member a tensor of bytes
        assert rd.tensor_info() == [(16, 1), (16, 1), (17, 1), (17, 1), (17, 1), (17, 1), (5, 1)]
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ damage
def _damaged(lib, oracle, data):
    """(good stream, stream with payload bits flipped in the last tenth of its last chunk whose whole decode FAILS): the flips of
    rc.damaged_text_member, the seed searched for"""
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


def test_damage_behind_the_stop_is_not_seen_and_before_it_names_the_member(lib, oracle, stream):
    n = 60_000
    text = _data.text(n, seed=6)
    planes = [_data.mixed(n, seed=1), _data.periodic(n, 3), text, _data.random_bytes(n)]
    hurt = [(pc.tensor_bytes(2, 40, 8), 2), (pc.np_merge(planes), 4), (pc.tensor_bytes(8, 17, 9), 8)]
    good, bad = _damaged(lib, oracle, text)
    blobs = [stream(pl) for pl in pc.planes_of(hurt)]
    assert blobs[4] == good
    blobs[4] = bad  # plane 2 of tensor 1
    rd = ec.ElemReader(lib, b"".join(blobs))
    try:
        assert rd.h, rd.err
        assert rd.set_planes([2, 4, 8]) == (0, "")
        early = [(1, 100, 900), (0, 3, 30), (1, n // 2, 16)]
        _check_read(rd.read_elements(early, len(ec.np_elements(hurt, early)), rem=4), hurt, early)
        late = [(0, 0, 40), (1, n - 64, 64), (2, 0, 17)]
        want = len(ec.np_elements(hurt, late))
        r = rd.read_elements(late, want)
        assert r.rc == EINVAL and "member 4," in r.err, r.err
        assert r.dst_len == want
        pc.same(r.arena[:r.at] + r.arena[r.at + want:], bytes([POISON]) * (r.arena_len - want), "the guards")
        # the units of the damaged tensor are not written; the other ranges' tensors decoded as ever
        a, c = ec.np_elements(hurt, late[:1]), ec.np_elements(hurt, late[2:])
        pc.same(r.arena, pc.expect_arena(r.arena_len, [(r.at, a), (r.at + want - len(c), c)]), "the arena")
        for ranges in ([(0, 0, 40), (2, 0, 17)], early):
            _check_read(rd.read_elements(ranges, len(ec.np_elements(hurt, ranges))), hurt, ranges)
    finally:
        rd.close()
