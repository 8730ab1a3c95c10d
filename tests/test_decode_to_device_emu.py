"""Members decoded from and into device memory (orz_amd/csrc/orz_decode_index.h) on the emulation backend.  The framing index
built by the device kernels must agree with index_members -- verdict and arrays -- on good and malformed containers, in both
layouts (one concatenation; a member table in any order with gaps), and the driver must write what the device decoder's
existing driver writes, inside the caller's buffer and nowhere else."""
import ctypes
import os
import random
import subprocess

import pytest

import _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPRE = ((1 << 25) - 1) // 2
KBLOCK = (1 << 25) - 1
ENOMEM, EINVAL = -12, -22


@pytest.fixture(scope="module")
def lib(emu):  # (the emu fixture builds build/libemu.so: the same compile line here)
    so = os.path.join(ROOT, "build", "libemu_decode_to_device.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_decode_to_device.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    return ctypes.CDLL(so)


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def _index(lib, blob, table=None):
    """output arrays for host_index / device_index, which return ("ok", begin, end, out_off, out_len, total) or ("err", message)"""
    blob = bytes(blob)
    cap = len(table) if table is not None else len(blob) + 1
    b, e, o = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)()
    ln = (ctypes.c_uint32 * cap)()
    m, tot = ctypes.c_uint64(), ctypes.c_uint64()
    err = ctypes.create_string_buffer(256)
    return b, e, o, ln, cap, m, tot, err, blob


def host_index(lib, blob):
    b, e, o, ln, cap, m, tot, err, blob = _index(lib, blob)
    rc = lib.emu_index_members(blob, ctypes.c_size_t(len(blob)), b, e, o, ln, ctypes.c_size_t(cap), ctypes.byref(m), ctypes.byref(tot),
                               err, ctypes.c_size_t(256))
    if rc:
        return ("err", err.value.decode())
    k = m.value
    return ("ok", list(b[:k]), list(e[:k]), list(o[:k]), list(ln[:k]), tot.value)


def device_index(lib, blob, table=None):
    b, e, o, ln, cap, m, tot, err, blob = _index(lib, blob, table)
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    rc = lib.emu_device_index(blob, ctypes.c_size_t(len(blob)), offs, lens, ctypes.c_size_t(len(table) if table is not None else 0), b, e, o,
                              ln, ctypes.c_size_t(cap), ctypes.byref(m), ctypes.byref(tot), err, ctypes.c_size_t(256))
    if rc:
        return ("err", err.value.decode())
    k = m.value
    return ("ok", list(b[:k]), list(e[:k]), list(o[:k]), list(ln[:k]), tot.value)


def same_verdict(h, d):
    """the device index says what index_members says: the same arrays, or a rejection with index_members' message (the device's
    names the member besides)"""
    if h[0] == "ok":
        assert d == h
    else:
        assert d[0] == "err" and d[1].startswith(h[1] + " (member "), (h, d)


class Decoded:
    pass


def decode(lib, blob, table=None, cap=None, slots=0, on_device=True, sizing=False, offsets=False, fill=0xA5):
    """decode_members_to_device into a buffer of `cap` bytes prefilled with `fill`, 64 canary bytes (0x5A) behind it"""
    blob = bytes(blob)
    src = ctypes.create_string_buffer(blob, max(len(blob), 1))
    r = Decoded()
    if sizing:
        cap = 0
    elif cap is None:
        cap = decode(lib, blob, table, sizing=True).dst_len
    buf = (ctypes.c_uint8 * (cap + 64))(*([fill] * cap + [0x5A] * 64))
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    dl, m = ctypes.c_uint64(), ctypes.c_uint64()
    oo = (ctypes.c_uint64 * (len(blob) + 1 + (len(table) if table else 0)))() if offsets else None
    st = (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r.rc = lib.emu_decode_to_device(src, ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                    ctypes.c_size_t(len(table) if table is not None else 0), None if sizing else buf,
                                    ctypes.c_size_t(0 if sizing else cap), slots, ctypes.byref(dl), ctypes.byref(m), oo, st, err,
                                    ctypes.c_size_t(256))
    r.dst_len, r.members, r.err = dl.value, m.value, err.value.decode()
    r.launches, r.host_waits = st[0], st[1]
    r.out = bytes(buf[: r.dst_len]) if r.rc == 0 and not sizing else None
    r.buf = bytes(buf[:cap])
    r.canary_ok = bytes(buf[cap:]) == b"\x5a" * 64
    r.offsets = list(oo[: r.members]) if offsets else None
    return r


@pytest.fixture(scope="module")
def emu_decode_members(emu):
    lib = ctypes.CDLL(os.path.join(ROOT, "build", "libemu.so"))

    def run(blob, slots=4):
        dst = ctypes.POINTER(ctypes.c_uint8)()
        n, m = ctypes.c_size_t(), ctypes.c_size_t()
        err = ctypes.create_string_buffer(256)
        rc = lib.emu_decode_members(bytes(blob), ctypes.c_size_t(len(blob)), slots, ctypes.byref(dst), ctypes.byref(n), ctypes.byref(m), err,
                                    ctypes.c_size_t(256))
        if rc:
            return None
        out = ctypes.string_at(dst, n.value)
        lib.emu_free(dst)
        return out, m.value

    return run


def _parts():  # (the shapes of tests/test_device_decoder.py's _parts(), smaller)
    return [(_data.mixed(60_000, seed=1), 1), (b"", 1), (_data.zeros_noise(50_000), 2), (b"x", 1), (_data.random_bytes(20_000), 0),
            (_data.periodic(30_000, 3), 1), (b"", 0)]


@pytest.fixture(scope="module")
def members(oracle):
    parts = _parts()
    return [p for p, _ in parts], [oracle.encode(p, lv) for p, lv in parts]


@pytest.fixture(scope="module")
def multi_chunk(oracle):
    data = _data.random_bytes(1_300_000)  # incompressible at -l0: one item per byte, more than 2^20 items -> two chunks
    return data, oracle.encode(data, 0)


def _chunks(member):
    """[(start of the chunk's LEB128 length, start of its payload, payload length)] of one member, EOF excluded"""
    out, at = [], 0
    while True:
        t, sh, s = 0, 0, at
        while True:
            b = member[at]
            at += 1
            t |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        if t == 0:
            return out
        out.append((s, at, t))
        at += t


def _varint_bits(v):
    """the end field's coding (src/coder.rs:101-113): two bits per payload bit, LSB first, (more, bit)"""
    nb = max(v.bit_length(), 1)
    bits = []
    for i in range(nb):
        bits += [1 if i + 1 < nb else 0, (v >> i) & 1]
    return bits


def _pack(bits):
    bits = bits + [0] * (-len(bits) % 32)
    return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def _leb(t):
    out = bytearray()
    while True:
        b = t & 0x7F
        t >>= 7
        out.append(b | (0x80 if t else 0))
        if not t:
            return bytes(out)


def _member(end_fields):
    """a member of framing only: one chunk per end field (the first with an empty census), then EOF"""
    out = bytearray()
    for i, ef in enumerate(end_fields):
        payload = _pack(([0, 0] if i == 0 else []) + _varint_bits(ef))
        out += _leb(len(payload)) + payload
    return bytes(out + b"\x00")


# ------------------------------------------------------------------------------------------------ the index
def test_device_index_equals_index_members_on_oracle_containers(lib, oracle, members, multi_chunk):
    _, blobs = members
    zeros = bytes(17_000_000)  # crosses the slide at kBlock
    cases = [b"".join(blobs), blobs[1], blobs[3], multi_chunk[1], oracle.encode(zeros, 0), multi_chunk[1] + b"".join(blobs), b""]
    for blob in cases:
        h = host_index(lib, blob)
        assert h[0] == "ok"
        assert device_index(lib, blob) == h
    h = host_index(lib, multi_chunk[1])
    assert len(_chunks(multi_chunk[1])) >= 2 and h[4] == [len(multi_chunk[0])]
    assert host_index(lib, oracle.encode(zeros, 0))[4] == [len(zeros)]


def test_device_index_agrees_on_truncated_containers(lib, members):
    _, blobs = members
    blob = b"".join(blobs)
    bounds = set()
    at = 0
    for b in blobs:
        at += len(b)
        bounds.update({at - 1, at, at + 1})
    cuts = sorted(set(range(0, len(blob), 173)) | {c for c in bounds if 0 <= c < len(blob)})
    rejected = 0
    for c in cuts:
        h = host_index(lib, blob[:c])
        same_verdict(h, device_index(lib, blob[:c]))
        rejected += h[0] == "err"
    assert rejected > len(cuts) // 2


def test_device_index_agrees_on_malformed_framing(lib, members, multi_chunk):
    _, blobs = members
    good = blobs[0] + multi_chunk[1] + blobs[2]
    head = len(blobs[0])
    (s0, p0, t0), (s1, p1, t1) = _chunks(multi_chunk[1])[:2]
    bad = []
    # a flipped LEB128 continuation bit: the length's last byte continues into the payload
    flipped = bytearray(good)
    flipped[head + p0 - 1] |= 0x80
    bad.append(bytes(flipped))
    # a chunk length past the end
    bad.append(blobs[0] + _leb(len(good)) + multi_chunk[1][p0:])
    # end fields that go backwards: the second chunk's below the first's, and one below the window's start
    for ef in (KPRE + 5, 0):
        m = bytearray(multi_chunk[1])
        patch = _pack(_varint_bits(ef))[:8]
        m[p1:p1 + len(patch)] = patch
        bad.append(blobs[0] + bytes(m))
    # an end field past the block
    bad.append(blobs[2] + _member([KBLOCK + 1]))
    # a member that announces more than its bits can code
    bad.append(blobs[0] + _member([KBLOCK - 1]))
    # a census of more than 389 symbols
    census = _pack(_varint_bits(390))
    bad.append(_leb(len(census)) + census + b"\x00")
    # a member of 4 GiB or more (255 slides)
    bad.append(_member([KBLOCK] * 256))
    seen = set()
    for blob in bad:
        h = host_index(lib, blob)
        assert h[0] == "err", h
        seen.add(h[1])
        same_verdict(h, device_index(lib, blob))
    assert len(seen) == 5, seen  # (the truncated length: the test above)


def test_member_table_index_equals_the_concatenation(lib, members):
    _, blobs = members
    rng = random.Random(5)
    order = list(range(len(blobs)))
    rng.shuffle(order)
    buf, table = bytearray(), [None] * len(blobs)
    for k in order:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40)))  # gaps of garbage
        table[k] = (len(buf), len(blobs[k]))
        buf += blobs[k]
    buf += b"\x07" * 9
    h = host_index(lib, b"".join(blobs))
    d = device_index(lib, bytes(buf), table)
    assert d[0] == "ok"
    assert d[1] == [o for o, _ in table] and d[2] == [o + ln for o, ln in table]
    assert d[3:] == h[3:]  # out_off, out_len, total


def test_member_table_errors_are_rejected(lib, members):
    _, blobs = members
    buf = b"".join(blobs) + b"\x00\x00"
    table, at = [], 0
    for b in blobs:
        table.append((at, len(b)))
        at += len(b)
    assert device_index(lib, buf, table)[0] == "ok"
    k = 2
    o, ln = table[k]
    cases = {
        "out of range": (len(buf), 1),
        "past the end": (o, len(buf) - o + 1),
        "ends before its EOF byte": (o, ln - 1),
        "ends after its EOF byte": (o, ln + 1),
        "zero length": (o, 0),
    }
    for why, entry in cases.items():
        t = list(table)
        t[k] = entry
        d = device_index(lib, buf, t)
        assert d[0] == "err" and d[1].endswith("(member %d)" % k), (why, d)
        assert d[1].startswith("invalid orz data"), (why, d)
        r = decode(lib, buf, t, cap=sum(len(p) for p in members[0]) + 16)
        assert r.rc == EINVAL and "(member %d)" % k in r.err and r.launches == 0, why
        assert r.buf == b"\xa5" * len(r.buf) and r.canary_ok, why
    t = list(table)
    t[1], t[4] = (len(buf), 0), (o, ln + 1)
    assert device_index(lib, buf, t)[1].endswith("(member 1)")  # the FIRST bad member is named


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_writes_what_the_device_decoder_writes(lib, members, emu_decode_members):
    parts, blobs = members
    blob = b"".join(blobs)
    want, m = emu_decode_members(blob)
    assert want == b"".join(parts) and m == len(parts)
    for on_device in (True, False):
        r = decode(lib, blob, on_device=on_device, offsets=True)
        assert r.rc == 0, r.err
        assert r.out == want and r.members == m and r.dst_len == len(want) and r.canary_ok
        assert r.offsets == [sum(len(p) for p in parts[:k]) for k in range(len(parts))]
        assert r.host_waits == (2 if on_device else 3)  # (the upload of a host container, the index record, the statuses)
    # a poisoned destination of another colour gives the same bytes: nothing is read before it is written
    assert decode(lib, blob, fill=0x00).out == want


def test_driver_member_table_decodes_to_member_order(lib, members):
    parts, blobs = members
    rng = random.Random(11)
    order = list(range(len(blobs)))
    rng.shuffle(order)
    buf, table = bytearray(b"\xff" * 3), [None] * len(blobs)
    for k in order:
        table[k] = (len(buf), len(blobs[k]))
        buf += blobs[k] + bytes(rng.randrange(256) for _ in range(rng.randrange(1, 30)))
    r = decode(lib, bytes(buf), table, offsets=True)
    assert r.rc == 0, r.err
    assert r.out == b"".join(parts) and r.members == len(parts) and r.canary_ok
    assert r.host_waits == 3  # (the table's upload, the index record, the statuses)


def test_driver_multi_chunk_and_slide(lib, oracle, multi_chunk):
    data, blob = multi_chunk
    two = oracle.encode(b"ab" * 40_000, 2)
    r = decode(lib, blob + two)
    assert r.rc == 0 and r.out == data + b"ab" * 40_000 and r.canary_ok


def test_driver_slots_bound_the_members_in_flight(lib, members):
    parts, blobs = members
    r = decode(lib, b"".join(blobs), slots=3)
    assert r.rc == 0 and r.out == b"".join(parts)
    assert r.launches == 3  # 7 members, 3 at a time


def test_sizing_call_decodes_nothing(lib, members):
    parts, blobs = members
    blob = b"".join(blobs)
    r = decode(lib, blob, sizing=True, offsets=True)
    assert r.rc == 0 and r.dst_len == sum(len(p) for p in parts) and r.members == len(parts)
    assert r.launches == 0 and r.offsets == [sum(len(p) for p in parts[:k]) for k in range(len(parts))]
    r = decode(lib, blob, sizing=True)
    assert r.rc == 0 and r.launches == 0 and r.dst_len == sum(len(p) for p in parts) and r.host_waits == 1
    e = decode(lib, b"", sizing=True)
    assert e.rc == 0 and e.members == 0 and e.dst_len == 0
    e = decode(lib, b"")
    assert e.rc == 0 and e.members == 0 and e.out == b""


def test_capacity_one_byte_short(lib, members):
    parts, blobs = members
    total = sum(len(p) for p in parts)
    r = decode(lib, b"".join(blobs), cap=total - 1)
    assert r.rc == ENOMEM and r.launches == 0
    assert r.dst_len == total and r.members == len(parts)
    assert r.buf == b"\xa5" * (total - 1) and r.canary_ok
    assert decode(lib, b"".join(blobs), cap=total + 5).out == b"".join(parts)


def test_corrupted_payloads_agree_with_the_device_decoder(lib, oracle, emu_decode_members):
    good = oracle.encode(_data.mixed(50_000, seed=3), 1) + oracle.encode(_data.text(20_000, seed=2), 0)
    rejected = 0
    for start, step, x in ((200, 997, 0x5A), (31, 1499, 0x01), (500, 211, 0x80), (90, 4001, 0xFF)):
        bad = bytearray(good)
        for i in range(start, len(bad), step):
            bad[i] ^= x
        want = emu_decode_members(bytes(bad))
        r = decode(lib, bytes(bad), cap=200_000)
        if want is None:
            assert r.rc == EINVAL, r.err
            rejected += 1
        else:
            assert r.rc == 0 and r.out == want[0] and r.members == want[1]
        assert r.canary_ok
    assert rejected >= 1
