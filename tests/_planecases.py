"""Shared by the two tiers of the byte-plane tests (test_planes_emu.py, test_gpu_planes.py): the cases, split and merge restated
in numpy, the emulation twin (tests/emu/emu_planes.cpp) behind a small Python face, and poisoned arenas with guard gaps."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENOMEM, EINVAL = -12, -22
GUARD, POISON = 64, 0xA5
MASK = (1 << 64) - 1
ELEMS = (1, 2, 4, 8)
# the partial unit only, a full unit exactly, full plus partial, more than one wavefront of units (a unit is 16 elements)
COUNTS = (0, 1, 15, 16, 17, 1029, 4097)


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_planes.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_planes.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_plane_move.restype = ctypes.c_uint64
    lib.emu_plane_pitch.restype = ctypes.c_uint64
    return lib


# ------------------------------------------------------------------------------------------------ the restatement
def np_split(data, e):
    """the e byte planes of `data` (bytes, a multiple of e long): plane p = the bytes at offsets p, p + e, p + 2 e, ..."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    assert a.size % e == 0
    return [a[p::e].tobytes() for p in range(e)]


def np_merge(planes):
    """the inverse: planes of equal length interleaved"""
    e = len(planes)
    out = np.empty(e * len(planes[0]), dtype=np.uint8)
    for p, pl in enumerate(planes):
        out[p::e] = np.frombuffer(bytes(pl), dtype=np.uint8)
    return out.tobytes()


def pitch(count):
    return (count + 15) // 16 * 16


def tensor_bytes(e, count, seed):
    """count elements of e bytes: every byte random, so that a byte routed to the wrong place shows"""
    return np.random.default_rng(1000 * seed + 10 * count + e).integers(0, 256, size=e * count, dtype=np.uint8).tobytes()


def mixed_tensors(elems=ELEMS, counts=COUNTS):
    """[(bytes, element size)]: every element size at every count in ONE list, sizes alternating, empty tensors between them"""
    out = []
    for ci, c in enumerate(counts):
        for ei in range(len(elems)):
            e = elems[(ei + ci) % len(elems)]
            out.append((tensor_bytes(e, c, len(out)), e))
        out.append((b"", elems[ci % len(elems)]))
    return out


def planes_of(tensors):
    """the members of a list of tensors: the planes of each, plane 0 first"""
    return [pl for data, e in tensors for pl in np_split(data, e)]


# ------------------------------------------------------------------------------------------------ arenas
class Arena:
    """`length` bytes of `fill` whose first byte lies at a multiple of `align`"""

    def __init__(self, length, align=256, fill=POISON):
        self._raw = (ctypes.c_uint8 * (length + align)).from_buffer(bytearray(bytes([fill]) * (length + align)))
        self.skip = (-ctypes.addressof(self._raw)) % align
        self.base = ctypes.addressof(self._raw) + self.skip
        self.length, self.fill = length, fill

    def write(self, off, data):
        ctypes.memmove(self.base + off, bytes(data), len(data))

    def bytes(self):
        return bytes(self._raw)[self.skip:self.skip + self.length]


def layout(sizes, rem, align=16, guard=GUARD, reverse=False):
    """places of `sizes` bytes in one arena, each at an address that is `rem[k]` modulo `align`, a guard gap in front of, between
    and behind them: ([offset], arena length)"""
    at, offs = guard, [0] * len(sizes)
    order = reversed(range(len(sizes))) if reverse else range(len(sizes))
    for k in order:
        at += (rem[k] - at) % align
        offs[k] = at
        at += sizes[k] + guard
    return offs, at


def expect_arena(length, pieces, fill=POISON):
    """an arena of `fill` with (offset, bytes) pieces in it"""
    want = bytearray(bytes([fill]) * length)
    for o, b in pieces:
        want[o:o + len(b)] = b
    return bytes(want)


def same(got, want, what):
    if got != want:
        k = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
        raise AssertionError("%s differs from what was expected from byte %d on" % (what, k))


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def _u32(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


# ------------------------------------------------------------------------------------------------ the kernels
def staging_layout(tensors):
    """as the encode driver stages: the planes of every tensor with an element size above 1 at a multiple of 256, pitch apart:
    ([offset of plane 0, or None], staging length)"""
    at, offs = 256, []
    for data, e in tensors:
        if e == 1:
            offs.append(None)
            continue
        offs.append(at)
        at = (at + e * pitch(len(data) // e) + 255) // 256 * 256
    return offs, at + 256


def move(lib, merge, tensors, inter, inter_offs, stage, stage_offs):
    """ONE PlaneSplit (merge = False) or PlaneMerge launch over the tensors with an element size above 1; returns its units"""
    rows = [(inter.base + io, stage.base + so, len(data) // e, e) for (data, e), io, so in zip(tensors, inter_offs, stage_offs) if e > 1]
    return lib.emu_plane_move(1 if merge else 0, ctypes.c_size_t(len(rows)), _u64([r[0] for r in rows]), _u64([r[1] for r in rows]),
                              _u64([r[2] for r in rows]), _u32([r[3] for r in rows]))


# ------------------------------------------------------------------------------------------------ the decode driver
class Decoded:
    pass


def decode_planes(lib, blob, table, places, elems, arena_len, on_device=True, sizing=False, slots=0, src_at=None, fill=POISON):
    """decode_members_planes on the emulation.  `places`: (offset in the arena or None for a null pointer, capacity) per
    destination; the arena is `arena_len` bytes of `fill` at a multiple of 16.  src_at: the container lies INSIDE the arena at that
    offset.  Returns rc / err / members / out_lens / launches / host_waits / arena."""
    blob = bytes(blob)
    arena = Arena(max(arena_len, 1), align=16, fill=fill)
    if src_at is not None:
        arena.write(src_at, blob)
        src = ctypes.c_void_p(arena.base + src_at)
    else:
        keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
        src = ctypes.cast(keep, ctypes.c_void_p)
    nd = len(places)
    dsts = (ctypes.c_void_p * max(nd, 1))(*[(arena.base + o if o is not None else None) for o, _ in places])
    caps = _u64([c for _, c in places])
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    out_lens = (ctypes.c_uint64 * max(nd, 1))(*([MASK] * max(nd, 1)))
    m = ctypes.c_uint64()
    st = (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r = Decoded()
    r.rc = lib.emu_decode_planes(src, ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                 ctypes.c_size_t(len(table) if table is not None else 0), None if sizing else dsts, caps, _u32(elems),
                                 ctypes.c_size_t(nd), slots, out_lens, ctypes.byref(m), st, err, ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens = list(out_lens[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.arena = arena.bytes()[:arena_len]
    return r


def table_of(blobs, order=None, gap=7):
    """the members in one buffer in `order` with gaps of garbage: (buffer, [(offset, length)] in member order)"""
    order = list(range(len(blobs))) if order is None else order
    buf, table = bytearray(b"\xff" * 3), [None] * len(blobs)
    for k in order:
        table[k] = (len(buf), len(blobs[k]))
        buf += blobs[k] + b"\x07" * gap
    return bytes(buf), table
