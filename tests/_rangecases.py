"""Shared by the two tiers of the range reader's tests (test_decode_range_emu.py, test_gpu_decode_range.py): the container, the
ranges, the damaged member, and the emulation twin (tests/emu/emu_decode_range.cpp) behind a small Python face."""
import ctypes
import os
import random
import subprocess

import _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENOMEM, EINVAL = -12, -22
SLACK = 240 + 127  # kMaxLen + 127: the longest item the decoder admits (orz_decode_device.h)


def parts():  # (tests/test_gpu_decode_to_device.py::_parts)
    return [(_data.mixed(120_000, seed=1), 1), (b"", 1), (_data.zeros_noise(90_000), 2), (b"x", 1), (_data.random_bytes(30_000), 0),
            (_data.periodic(40_000, 3), 1), (_data.mixed(50_000, seed=9), 0)]


def table_layout(blobs, seed=5):
    """the members shuffled into one buffer with gaps of garbage: (buffer, [(offset, length)] in member order)"""
    rng = random.Random(seed)
    order = list(range(len(blobs)))
    rng.shuffle(order)
    buf, table = bytearray(b"\xff" * 3), [None] * len(blobs)
    for k in order:
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40)))
        table[k] = (len(buf), len(blobs[k]))
        buf += blobs[k]
    buf += b"\x07" * 9
    return bytes(buf), table


def starts(lengths):
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += n
    return out


def named_ranges(lengths):
    """{name: (offset, length)} over a container whose members decode to `lengths` bytes (the shape of parts())"""
    s, total = starts(lengths), sum(lengths)
    r = {"everything": (0, total), "first byte": (0, 1), "last byte": (total - 1, 1), "nothing at 0": (0, 0), "nothing at the end": (total, 0),
         "inside member 0": (1234, 40_001), "inside member 2, unaligned": (s[2] + 7, 333),
         "across one boundary": (s[5] - 100, 300), "across the empty member": (s[1] - 50, 120),
         "across several boundaries": (s[2] + 80_000, lengths[2] - 80_000 + lengths[3] + lengths[4] + 500),
         "the one-byte member and its neighbours": (s[3] - 1, 3)}
    for k, n in enumerate(lengths):
        r["member %d exactly" % k] = (s[k], n)
    return r


def batch(total, n=500, seed=77):
    """n seeded ranges: short and long, duplicates, overlaps, a descending stretch, empty ones"""
    rng = random.Random(seed)
    out = []
    for _ in range(n - 60):
        ln = rng.choice([0, 1, 2, 15, 16, 17, 100, 1000, rng.randrange(0, 5000)])
        off = rng.randrange(0, total - ln + 1)
        out.append((off, ln))
    out += [out[3], out[3], out[10], (out[10][0] + 1, out[10][1]), (0, 0), (total, 0), (total - 1, 1)]
    desc = sorted(((rng.randrange(0, total - 64), rng.randrange(1, 64)) for _ in range(60 - 7)), reverse=True)
    return out + desc


def touched(ranges, lengths):
    """{member: furthest member offset asked of it} over the non-empty ranges"""
    s, far = starts(lengths), {}
    for off, ln in ranges:
        if not ln:
            continue
        for m, n in enumerate(lengths):
            lo, hi = max(off, s[m]), min(off + ln, s[m] + n)
            if lo < hi:
                far[m] = max(far.get(m, 0), hi - s[m])
    return far


def check_decoded_bytes(decoded_bytes, ranges, lengths):
    """the early stop: every decoded member went as far as the furthest byte asked of it, and less than one item further"""
    far = touched(ranges, lengths)
    least = sum(far.values())
    early = sum(1 for m, f in far.items() if f < lengths[m])
    assert least <= decoded_bytes <= least + early * (SLACK - 1), (decoded_bytes, least, early)


def chunks(member):
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


DAMAGE_SEED = 4  # (chosen so that the whole decode of the damaged member fails: the tests assert that it does)


def damaged_text_member(oracle, seed=DAMAGE_SEED):
    """(data, good stream, stream with payload bits flipped in the last tenth of its last chunk): the framing -- chunk lengths,
    census, end fields, which open a chunk -- is untouched, and so is every item before the flip (the bits are read in order)"""
    data = _data.text(1_200_000, seed=6)
    good = oracle.encode(data, 1)
    _, p, t = chunks(good)[-1]
    rng = random.Random(seed)
    bad = bytearray(good)
    for _ in range(40):
        bad[p + t - 1 - rng.randrange(0, t // 10)] ^= 1 << rng.randrange(8)
    return data, good, bytes(bad)


# ------------------------------------------------------------------------------------------------ the emulation twin
def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_decode_range.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_decode_range.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_reader_open.restype = ctypes.c_void_p
    return lib


def whole_lib():
    """build/libemu_decode_to_device.so (the existing whole-container driver on the emulation), built as the fixture of
    tests/test_decode_to_device_emu.py builds it"""
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


class Read:
    pass


class EmuReader:
    """the reader on the emulation backend; "device memory" is host memory"""

    def __init__(self, lib, blob, table=None, on_device=True):
        self.lib = lib
        blob = bytes(blob)
        self.src = ctypes.create_string_buffer(blob, max(len(blob), 1))  # (borrowed by the reader when on_device)
        err = ctypes.create_string_buffer(256)
        offs = _u64([t[0] for t in table]) if table is not None else None
        lens = _u64([t[1] for t in table]) if table is not None else None
        self.h = lib.emu_reader_open(self.src, ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                     ctypes.c_size_t(len(table) if table is not None else 0), err, ctypes.c_size_t(256))
        self.err = err.value.decode()
        if self.h:
            m, tot = ctypes.c_uint64(), ctypes.c_uint64()
            oo = (ctypes.c_uint64 * (len(blob) + 1))()
            lib.emu_reader_info(ctypes.c_void_p(self.h), ctypes.byref(m), ctypes.byref(tot), oo, ctypes.c_size_t(len(blob) + 1))
            self.members, self.total, self.member_offsets = m.value, tot.value, list(oo[: m.value])

    def read(self, ranges, cap=None, slots=0, fill=0xA5, null_arrays=False):
        """the ranges into a buffer of `cap` bytes (default: the sum of the lengths plus 32) prefilled with `fill`, 64 canary
        bytes (0x5A) behind it"""
        r = Read()
        if cap is None:
            cap = sum(ln for _, ln in ranges) + 32
        buf = (ctypes.c_uint8 * (cap + 64)).from_buffer(bytearray(bytes([fill]) * cap + b"\x5a" * 64))
        off, ln = _u64([o for o, _ in ranges]), _u64([n for _, n in ranges])
        dl = ctypes.c_uint64()
        st = (ctypes.c_uint64 * 6)()
        err = ctypes.create_string_buffer(256)
        r.rc = self.lib.emu_reader_read(ctypes.c_void_p(self.h), None if null_arrays else off, None if null_arrays else ln,
                                        ctypes.c_size_t(len(ranges)), buf, ctypes.c_size_t(cap), slots, ctypes.byref(dl), st, err,
                                        ctypes.c_size_t(256))
        r.err, r.dst_len = err.value.decode(), dl.value
        r.ranges, r.members_decoded, r.decoded_bytes, r.out_bytes, r.launches, r.host_waits = list(st)
        raw = bytes(buf)
        r.out = raw[: r.dst_len] if r.rc == 0 else None
        r.rest_ok = raw[min(r.dst_len, cap) if r.rc == 0 else 0:cap] == bytes([fill]) * (cap - (min(r.dst_len, cap) if r.rc == 0 else 0))
        r.buf = raw[:cap]
        r.canary_ok = raw[cap:] == b"\x5a" * 64
        return r

    def close(self):
        if self.h:
            self.lib.emu_reader_close(ctypes.c_void_p(self.h))
            self.h = None
