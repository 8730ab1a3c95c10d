"""Byte ranges of a members container (orz_amd/csrc/orz_decode_range.h) on the emulation backend: a reader indexes a container
once and serves reads; every read equals the Python slice of the known input, decodes only the members it touches and each
only as far as the furthest byte asked of it, waits for the host three times, and writes inside [dst, dst + dst_len) only."""
import ctypes
import math
import os

import pytest

import _data
import _rangecases as rc
from _rangecases import EINVAL, ENOMEM, EmuReader


@pytest.fixture(scope="module")
def lib(emu):  # (the emu fixture builds build/libemu.so: the same compile line in _rangecases.emu_lib)
    return rc.emu_lib()


@pytest.fixture(scope="module")
def container(oracle):
    parts = rc.parts()
    return [p for p, _ in parts], [oracle.encode(p, lv) for p, lv in parts]


@pytest.fixture(scope="module", params=["concatenation", "table"])
def reader(request, lib, container):
    plain, blobs = container
    if request.param == "table":
        buf, table = rc.table_layout(blobs)
        r = EmuReader(lib, buf, table)
    else:
        r = EmuReader(lib, b"".join(blobs))
    assert r.h, r.err
    yield r
    r.close()


def test_info(reader, container):
    plain, _ = container
    lengths = [len(p) for p in plain]
    assert reader.members == 7 and reader.total == sum(lengths)
    assert reader.member_offsets == rc.starts(lengths)


def test_named_ranges_equal_the_slices(reader, container):
    plain, _ = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    for name, (off, ln) in rc.named_ranges(lengths).items():
        r = reader.read([(off, ln)])
        assert r.rc == 0, (name, r.err)
        assert r.dst_len == ln and r.out == data[off:off + ln], name
        assert r.rest_ok and r.canary_ok, name
        assert r.host_waits == (3 if ln else 0) and r.launches == (1 if ln else 0), name
        assert r.members_decoded == len(rc.touched([(off, ln)], lengths)), name
        rc.check_decoded_bytes(r.decoded_bytes, [(off, ln)], lengths)


def test_a_batch_of_500_ranges_in_one_call(reader, container):
    plain, _ = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    ranges = rc.batch(len(data))
    assert len(ranges) == 500 and len(set(ranges)) < 500 and any(ln == 0 for _, ln in ranges)
    assert any(a[0] > b[0] for a, b in zip(ranges, ranges[1:]))
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    need = len(rc.touched(ranges, lengths))
    assert need == 6  # every member but the empty one
    for slots, launches in ((1, need), (2, math.ceil(need / 2)), (0, 1)):
        r = reader.read(ranges, slots=slots)
        assert r.rc == 0, r.err
        assert r.out == want and r.dst_len == len(want) and r.out_bytes == len(want) and r.ranges == 500
        assert r.members_decoded == need and r.host_waits == 3 and r.launches == launches
        assert r.rest_ok and r.canary_ok
        rc.check_decoded_bytes(r.decoded_bytes, ranges, lengths)


def test_the_decode_stops_early(reader, container):
    plain, _ = container
    lengths = [len(p) for p in plain]
    r = reader.read([(0, 1000)])
    assert r.rc == 0 and r.out == plain[0][:1000]
    assert 1000 <= r.decoded_bytes < 1000 + rc.SLACK and r.members_decoded == 1
    # a read that ends inside member 2: members 0 and 1 are not touched, member 2 stops at the range's end
    s = rc.starts(lengths)
    e = 33_333
    r = reader.read([(s[2] + 10, e - 10), (s[2] + 5, 20)])
    assert r.rc == 0 and r.out == plain[2][10:e] + plain[2][5:25]
    assert e <= r.decoded_bytes < e + rc.SLACK and r.members_decoded == 1 and r.launches == 1


def test_damage_behind_the_stop_is_not_seen(lib, oracle, container):
    plain, blobs = container
    data, good, bad = rc.damaged_text_member(oracle)
    assert len(data) >= 1_000_000 and len(bad) == len(good) and bad != good
    blob = blobs[0] + bad + blobs[3]
    # the precondition, by the existing driver: the whole decode of this container fails
    import test_decode_to_device_emu as whole

    wlib = rc.whole_lib()
    full = whole.decode(wlib, blob, cap=len(plain[0]) + len(data) + 1 + 64)
    assert full.rc == EINVAL and "(member 1" in full.err, (full.rc, full.err)
    assert whole.decode(wlib, blobs[0] + good + blobs[3]).rc == 0
    rd = EmuReader(lib, blob)
    assert rd.h, rd.err  # (the framing is intact: the index accepts the container)
    try:
        base = len(plain[0])
        half = len(data) // 2
        r = rd.read([(base, half)])
        assert r.rc == 0, r.err
        assert r.out == data[:half] and half <= r.decoded_bytes < half + rc.SLACK
        r = rd.read([(base + len(data) - 1, 1), (0, 10)])
        assert r.rc == EINVAL and "(member 1," in r.err, (r.rc, r.err)
        assert r.canary_ok and r.buf[11:] == b"\xa5" * (len(r.buf) - 11)
        r = rd.read([(base + 100, 5000), (base + len(data), 1), (3, 9)])  # the same reader serves a good read
        assert r.rc == 0 and r.out == data[100:5100] + b"x" + plain[0][3:12]
    finally:
        rd.close()


def test_a_member_of_more_than_one_block(lib, oracle):
    data = _data.zeros_noise(17_000_000)
    assert len(data) > 1 << 24
    rd = EmuReader(lib, oracle.encode(data, 0) + oracle.encode(b"tail", 0))
    assert rd.h and rd.total == len(data) + 4
    try:
        slide = 1 << 24
        ranges = [(slide - 5000, 4000), (slide - 300, 900), (slide + 10, 70_000), (len(data) - 3, 7)]
        r = rd.read(ranges)
        assert r.rc == 0, r.err
        assert r.out == b"".join((data + b"tail")[o:o + ln] for o, ln in ranges)
        assert r.members_decoded == 2 and r.decoded_bytes == len(data) + 4
        r = rd.read([(slide - 5000, 4000)])
        assert r.rc == 0 and r.out == data[slide - 5000:slide - 1000] and r.decoded_bytes < slide - 1000 + rc.SLACK
        r = rd.read([(slide - 300, 900)])
        assert r.rc == 0 and r.out == data[slide - 300:slide + 600] and slide + 600 <= r.decoded_bytes < slide + 600 + rc.SLACK
    finally:
        rd.close()


def test_nothing_outside_the_output_is_written(reader, container):
    plain, _ = container
    data = b"".join(plain)
    ranges = [(100_000, 50_000), (5, 3), (len(data) - 77, 77)]
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    a = reader.read(ranges, cap=len(want) + 1000, fill=0xA5)
    b = reader.read(ranges, cap=len(want) + 1000, fill=0x00)
    assert a.rc == 0 and b.rc == 0 and a.out == want and b.out == want
    assert a.buf[len(want):] == b"\xa5" * 1000 and b.buf[len(want):] == b"\x00" * 1000 and a.canary_ok and b.canary_ok
    exact = reader.read(ranges, cap=len(want))
    assert exact.rc == 0 and exact.out == want and exact.canary_ok


def test_refusals_come_before_any_launch(reader, container):
    plain, _ = container
    data = b"".join(plain)
    total = len(data)
    r = reader.read([(0, 1000), (50, 24)], cap=1023)
    assert r.rc == ENOMEM and r.dst_len == 1024 and r.launches == 0 and r.host_waits == 0
    assert r.buf == b"\xa5" * 1023 and r.canary_ok
    for why, ranges in {"past the end": [(0, 10), (total - 5, 6)], "offset past the end": [(total + 1, 0)],
                        "overflow": [(1 << 63, 1 << 63)], "overflow by one": [(2, (1 << 64) - 1)]}.items():
        r = reader.read(ranges, cap=4096)
        assert r.rc == EINVAL and r.launches == 0 and r.host_waits == 0, why
        assert "invalid argument" in r.err and r.buf == b"\xa5" * 4096 and r.canary_ok, why
    r = reader.read([(0, 10)], cap=64, null_arrays=True)
    assert r.rc == EINVAL and r.launches == 0 and r.buf == b"\xa5" * 64
    # a borrowed container that overlaps the output
    n = len(reader.src.raw)
    inside = (ctypes.c_uint8 * 16).from_buffer(reader.src, max(n - 17, 0))
    dl, st, err = ctypes.c_uint64(), (ctypes.c_uint64 * 6)(), ctypes.create_string_buffer(256)
    before = reader.src.raw
    got = reader.lib.emu_reader_read(ctypes.c_void_p(reader.h), rc._u64([0]), rc._u64([8]), ctypes.c_size_t(1), inside, ctypes.c_size_t(16), 0,
                                     ctypes.byref(dl), st, err, ctypes.c_size_t(256))
    assert got == EINVAL and "overlap" in err.value.decode() and st[4] == 0 and reader.src.raw == before
    # nothing to read: no launch
    for ranges in ([], [(0, 0), (total, 0), (17, 0)]):
        r = reader.read(ranges, cap=8)
        assert r.rc == 0 and r.dst_len == 0 and r.launches == 0 and r.buf == b"\xa5" * 8
    r = reader.read([(7, 5)])  # the reader is as good as before
    assert r.rc == 0 and r.out == data[7:12]


def test_a_host_container_is_copied(lib, container):
    plain, blobs = container
    data = b"".join(plain)
    rd = EmuReader(lib, b"".join(blobs), on_device=False)
    assert rd.h, rd.err
    try:
        ctypes.memset(rd.src, 0, len(rd.src.raw))  # the caller's copy may go
        r = rd.read([(119_990, 30)])
        assert r.rc == 0 and r.out == data[119_990:120_020] and r.host_waits == 3
    finally:
        rd.close()


def test_a_framing_defect_fails_the_open(lib, container):
    import test_decode_to_device_emu as whole

    plain, blobs = container
    wlib = rc.whole_lib()
    good = b"".join(blobs)
    for blob in (good[:-1], blobs[0] + blobs[2][:200], blobs[0] + b"\x85"):
        h = whole.host_index(wlib, blob)
        assert h[0] == "err"
        rd = EmuReader(lib, blob)
        assert not rd.h and rd.err.startswith(h[1] + " (member "), (h, rd.err)
    buf, table = rc.table_layout(blobs)
    table[2] = (table[2][0], table[2][1] - 1)
    rd = EmuReader(lib, buf, table)
    assert not rd.h and rd.err.startswith("invalid orz data") and rd.err.endswith("(member 2)")

