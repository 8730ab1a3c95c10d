"""The range reader's cursor cache (orz_amd/csrc/orz_decode_range.h, DecodeMember's suspend and resume) on the emulation backend:
a reader that keeps cursors decodes every byte of a member at most once however the reads walk through it, returns the bytes the
uncached reader returns, follows its policy (hit / resumed / fresh / uncached, least recently touched evicted) to the count, drops
the cursor of a member whose decode fails, and is the reader it was once the cache is switched off."""
import pytest

import _cachecases as cc
import _data
import _rangecases as rc
from _rangecases import EINVAL


@pytest.fixture(scope="module")
def lib(emu):  # (the emu fixture builds build/libemu.so: the same compile line in _cachecases.emu_lib)
    return cc.emu_lib()


@pytest.fixture(scope="module")
def container(oracle):
    parts = rc.parts()
    return [p for p, _ in parts], [oracle.encode(p, lv) for p, lv in parts]


@pytest.fixture(scope="module")
def text(oracle):
    return rc.damaged_text_member(oracle)


def _open(lib, blob, budget=None):
    rd = cc.CachedEmuReader(lib, blob)
    assert rd.h, rd.err
    if budget is not None:
        rd.set_cache(budget)
    return rd


def _stats(rd, **want):
    got = rd.cache_stats()
    assert {k: got[k] for k in want} == want, got
    return got


def test_a_sequential_walk_decodes_every_byte_once(lib, container, text):
    plain, blobs = container
    data, good, _ = text
    rd = _open(lib, blobs[0] + good + b"".join(blobs[1:]), budget=1 << 30)
    try:
        base, step, produced = len(plain[0]), 100_000, 0
        for k, lo in enumerate(range(0, len(data), step)):
            stop = min(lo + step, len(data))
            r = rd.read([(base + lo, stop - lo)])
            assert r.rc == 0, r.err
            assert r.out == data[lo:stop] and r.rest_ok and r.canary_ok
            assert r.decoded_bytes < (stop - produced) + rc.SLACK, (k, r.decoded_bytes, stop, produced)
            assert r.members_decoded == 1 and r.launches == 1 and r.host_waits <= 4
            _stats(rd, hits=0, resumed=1 if k else 0, fresh=0 if k else 1, uncached=0, evicted=0, cursors=2 if k else 1)
            produced += r.decoded_bytes
            assert produced >= stop
            # another member's decode between two windows: the LDS the walk's cursor comes back to is not the one it left
            o = rd.read([(base + len(data) + len(plain[1]) + 7000 * k, 500)])
            assert o.rc == 0 and o.out == plain[2][7000 * k:7000 * k + 500]
        assert produced == len(data)  # the member's final `produced`: its length
        assert rd.cache_stats()["bytes"] == cc.cost(len(data), rd.state_bytes) + cc.cost(len(plain[2]), rd.state_bytes)
    finally:
        rd.close()
    # the same walk without the cache: every window starts the member at byte 0
    rd = _open(lib, blobs[0] + good + b"".join(blobs[1:]))
    try:
        total = 0
        for lo in range(0, len(data), 400_000):  # (every fourth window: enough to show the difference)
            r = rd.read([(base + lo, step)])
            assert r.rc == 0 and r.out == data[lo:lo + step] and r.decoded_bytes >= lo + step and r.host_waits == 3
            total += r.decoded_bytes
        assert total > len(data)
    finally:
        rd.close()


def test_a_second_read_and_a_seek_backwards_are_hits(lib, container, text):
    plain, blobs = container
    data, good, _ = text
    rd = _open(lib, blobs[0] + good + blobs[3], budget=1 << 30)
    try:
        base = len(plain[0])
        first = rd.read([(base + 300_000, 100_000)])
        assert first.rc == 0 and first.out == data[300_000:400_000] and 400_000 <= first.decoded_bytes < 400_000 + rc.SLACK
        for off, ln in ((300_000, 100_000), (1234, 56_789), (0, 1), (399_999, 1)):
            r = rd.read([(base + off, ln)])
            assert r.rc == 0 and r.out == data[off:off + ln], (off, ln)
            assert r.decoded_bytes == 0 and r.launches == 0 and r.members_decoded == 0 and r.rest_ok and r.canary_ok
            _stats(rd, hits=1, resumed=0, fresh=0, uncached=0, evicted=0, cursors=1)
        r = rd.read([(base + 400_000 + rc.SLACK, 1)])  # one byte further than any item of the first read can have gone
        assert r.rc == 0 and r.out == data[400_000 + rc.SLACK:400_001 + rc.SLACK] and 0 < r.decoded_bytes <= 2 * rc.SLACK
        _stats(rd, hits=0, resumed=1)
    finally:
        rd.close()


def test_a_resume_across_a_window_slide(lib, oracle):
    data = _data.zeros_noise(17_000_000)
    assert len(data) > 1 << 24
    rd = _open(lib, oracle.encode(data, 0) + oracle.encode(b"tail", 0), budget=1 << 30)
    try:
        slide, total = 1 << 24, 0
        for k, (off, ln) in enumerate([(slide - 5000, 4000), (slide - 300, 900), (len(data) - 3, 3)]):
            r = rd.read([(off, ln)])
            assert r.rc == 0, r.err
            assert r.out == data[off:off + ln] and r.canary_ok and r.rest_ok
            assert r.decoded_bytes < off + ln - total + rc.SLACK
            _stats(rd, hits=0, resumed=1 if k else 0, fresh=0 if k else 1, cursors=1)
            total += r.decoded_bytes
        assert total == len(data)
        r = rd.read([(slide - 8, 16), (len(data) - 2, 6)])  # a hit across the slide, and the neighbour member fresh
        assert r.rc == 0 and r.out == data[slide - 8:slide + 8] + data[-2:] + b"tail" and r.decoded_bytes == 4
        _stats(rd, hits=1, fresh=1, cursors=2)
    finally:
        rd.close()


def test_a_resume_inside_a_chunk_and_at_a_chunk_boundary(lib, oracle):
    data = _data.random_bytes(1_100_000) + _data.text(300_000, seed=3)  # more than 2^20 items: two chunks
    stream = oracle.encode(data, 1)
    ends = cc.chunk_ends(stream)
    assert len(ends) == 2 and 0 < ends[0] < ends[1] == len(data)
    cut = ends[0]
    walks = {"the boundary itself": [cut], "a chunk's first item": [cut + 1], "a chunk's last item": [cut - 1],
             "the middle of both chunks": [cut // 2, (cut + len(data)) // 2],
             "all of them in one reader": [cut // 2, cut - 1, cut, cut + 1, (cut + len(data)) // 2]}
    for name, stops in walks.items():
        rd = _open(lib, stream, budget=1 << 30)
        try:
            produced = 0
            for stop in stops + [len(data)]:
                r = rd.read([(max(stop - 1000, 0), min(stop, 1000))])
                assert r.rc == 0, (name, stop, r.err)
                assert r.out == data[max(stop - 1000, 0):stop], (name, stop)
                assert stop - produced <= r.decoded_bytes < stop - produced + rc.SLACK, (name, stop)
                produced += r.decoded_bytes
            assert produced == len(data), name
            r = rd.read([(0, len(data))])  # everything the cursor holds, stored whole across every suspension
            assert r.rc == 0 and r.out == data and r.decoded_bytes == 0, name
        finally:
            rd.close()


def test_the_batch_equals_the_uncached_reader_under_three_budgets(lib, container):
    plain, blobs = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    ranges = rc.batch(len(data))
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    plain_rd = _open(lib, b"".join(blobs))
    try:
        ref = plain_rd.read(ranges)
        assert ref.rc == 0 and ref.out == want and ref.host_waits == 3
        sb = plain_rd.state_bytes
    finally:
        plain_rd.close()
    touched = sorted(rc.touched(ranges, lengths))
    assert touched == [0, 2, 3, 4, 5, 6]
    everything = sum(cc.cost(lengths[m], sb) for m in touched)
    two = cc.cost(lengths[0], sb) + cc.cost(lengths[2], sb)
    for name, budget, held in (("all members", everything, 6), ("two members", two, 2), ("none fits", cc.cost(1, sb) - 1, 0)):
        rd = _open(lib, b"".join(blobs), budget=budget)
        try:
            r = rd.read(ranges)
            assert r.rc == 0, (name, r.err)
            assert r.out == ref.out and r.dst_len == ref.dst_len and r.rest_ok and r.canary_ok, name
            assert r.members_decoded == 6 and r.launches == 1 and r.host_waits <= 4 and r.decoded_bytes == ref.decoded_bytes, name
            st = _stats(rd, hits=0, resumed=0, fresh=held, uncached=6 - held, evicted=0, cursors=held, budget=budget)
            assert st["bytes"] == sum(cc.cost(lengths[m], sb) for m in touched[:held]) <= budget, name
            for slots, launches in ((1, 6 - held), (2, (6 - held + 1) // 2), (0, 1 if held < 6 else 0)):  # again: the held members are hits
                r = rd.read(ranges, slots=slots)
                assert r.rc == 0 and r.out == ref.out and r.rest_ok and r.canary_ok, (name, slots)
                assert r.members_decoded == 6 - held and r.launches == launches, (name, slots)
                _stats(rd, hits=held, resumed=0, fresh=0, uncached=6 - held, evicted=0, cursors=held)
                far = {m: f for m, f in rc.touched(ranges, lengths).items() if m not in touched[:held]}
                early = sum(1 for m, f in far.items() if f < lengths[m])
                assert sum(far.values()) <= r.decoded_bytes <= sum(far.values()) + early * (rc.SLACK - 1), (name, slots)
        finally:
            rd.close()


def test_the_least_recently_touched_cursor_is_evicted(lib, oracle):
    plain = [_data.mixed(50_000, seed=k) for k in (21, 22, 23)]
    rd = _open(lib, b"".join(oracle.encode(p, 1) for p in plain))
    try:
        one = cc.cost(50_000, rd.state_bytes)
        rd.set_cache(2 * one)
        A, B, C = 0, 50_000, 100_000

        def touch(off, **want):
            r = rd.read([(off + 100, 2000)])
            assert r.rc == 0 and r.out == b"".join(plain)[off + 100:off + 2100]
            _stats(rd, **want)

        touch(A, fresh=1, evicted=0, cursors=1)
        touch(B, fresh=1, evicted=0, cursors=2)
        touch(C, fresh=1, evicted=1, cursors=2, bytes=2 * one)  # A goes
        touch(B, hits=1, fresh=0, evicted=0)
        touch(C, hits=1, fresh=0, evicted=0)
        touch(A, fresh=1, evicted=1, cursors=2)                 # B goes: C was touched after it
        touch(C, hits=1, evicted=0)
        touch(A, hits=1, evicted=0)
        touch(B, fresh=1, evicted=1, hits=0)                    # C goes
        # one call that touches all three: the two held are hits and may not be evicted for the third
        r = rd.read([(C + 5, 10), (A + 5, 10), (B + 5, 10)])
        assert r.rc == 0 and r.out == plain[2][5:15] + plain[0][5:15] + plain[1][5:15]
        _stats(rd, hits=2, fresh=0, uncached=1, evicted=0, cursors=2)
        # a smaller budget evicts the least recently touched; 0 frees everything
        touch(A, hits=1)
        rd.set_cache(one)
        _stats(rd, cursors=1, bytes=one, budget=one)
        touch(A, hits=1, cursors=1)
        rd.set_cache(one - 1)
        _stats(rd, cursors=0, bytes=0)
        touch(A, uncached=1, fresh=0, cursors=0)
        rd.set_cache(0)
        _stats(rd, cursors=0, bytes=0, budget=0)
    finally:
        rd.close()


def test_a_cursor_that_cannot_be_allocated_is_no_error(lib, container):
    plain, blobs = container
    rd = _open(lib, b"".join(blobs), budget=1 << 30)
    try:
        rd.fail_alloc_in(0)  # the read's first allocation: the cursor
        r = rd.read([(10, 5000)])
        assert r.rc == 0 and r.out == plain[0][10:5010]
        _stats(rd, fresh=0, uncached=1, cursors=0, bytes=0)
        r = rd.read([(10, 5000)])
        assert r.rc == 0 and r.out == plain[0][10:5010]
        _stats(rd, fresh=1, uncached=0, cursors=1)
    finally:
        rd.close()


def test_a_member_whose_decode_fails_loses_its_cursor(lib, container, text):
    plain, blobs = container
    data, good, bad = text
    rd = _open(lib, blobs[0] + bad + blobs[3], budget=1 << 30)
    try:
        base, half = len(plain[0]), len(data) // 2
        sb = rd.state_bytes
        r = rd.read([(base, half), (5, 10)])
        assert r.rc == 0, r.err
        assert r.out == data[:half] + plain[0][5:15] and r.rest_ok and r.canary_ok
        _stats(rd, fresh=2, cursors=2, bytes=cc.cost(len(plain[0]), sb) + cc.cost(len(data), sb))
        r = rd.read([(base + len(data) - 1, 1), (0, 10)])
        assert r.rc == EINVAL and "(member 1," in r.err, (r.rc, r.err)
        assert r.canary_ok and r.buf[11:] == b"\xa5" * (len(r.buf) - 11)
        _stats(rd, hits=1, resumed=1, cursors=1, bytes=cc.cost(len(plain[0]), sb))  # the cursor is gone
        r = rd.read([(base, half)])
        assert r.rc == 0 and r.out == data[:half] and half <= r.decoded_bytes < half + rc.SLACK and r.rest_ok and r.canary_ok
        _stats(rd, hits=0, resumed=0, fresh=1, cursors=2)
        r = rd.read([(base + 100, 5000), (base + len(data), 1), (3, 9)])  # and the reader serves on
        assert r.rc == 0 and r.out == data[100:5100] + b"x" + plain[0][3:12] and r.canary_ok
    finally:
        rd.close()


def test_switched_off_the_reader_is_what_it_was(lib, container):
    plain, blobs = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    rd = _open(lib, b"".join(blobs))
    try:
        _stats(rd, cursors=0, bytes=0, budget=0)
        rd.set_cache(1 << 30)
        r = rd.read([(0, len(data))])
        assert r.rc == 0 and r.out == data and r.host_waits == 2  # the upload, and the members' verdicts
        assert _stats(rd, fresh=6, cursors=6)["bytes"] > 0
        rd.set_cache(0)
        _stats(rd, cursors=0, bytes=0, budget=0)
        for name, (off, ln) in rc.named_ranges(lengths).items():
            r = rd.read([(off, ln)])
            assert r.rc == 0 and r.out == data[off:off + ln] and r.rest_ok and r.canary_ok, name
            assert r.host_waits == (3 if ln else 0) and r.launches == (1 if ln else 0), name
            assert r.members_decoded == len(rc.touched([(off, ln)], lengths)), name
            rc.check_decoded_bytes(r.decoded_bytes, [(off, ln)], lengths)
            _stats(rd, hits=0, resumed=0, fresh=0, uncached=0, evicted=0, cursors=0)
    finally:
        rd.close()
