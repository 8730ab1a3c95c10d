"""Shared by the two tiers of the element-range tests (test_read_elements_emu.py, test_gpu_read_elements.py): the tensors, the
containers made of their numpy planes, the restatement in numpy, and the emulation twin (tests/emu/emu_elements.cpp: the reader
with the new calls, and ElementGather alone) behind the Python face of _cachecases."""
import ctypes
import os
import random
import subprocess

import _cachecases as cc
import _planecases as pc
import _rangecases as rc

ROOT = rc.ROOT
ENOMEM, EINVAL = rc.ENOMEM, rc.EINVAL
GUARD, POISON = pc.GUARD, pc.POISON
LONG = 1029  # elements of the long tensors: 64 full units and a tail of 5


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_elements.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_elements.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_reader_open.restype = ctypes.c_void_p
    lib.emu_reader_cursor_state_bytes.restype = ctypes.c_uint64
    lib.emu_element_gather.restype = ctypes.c_uint64
    return lib


# ------------------------------------------------------------------------------------------------ the cases
def long_tensors():
    """one tensor each of element size 2, 4 and 8 with LONG elements"""
    return [(pc.tensor_bytes(e, LONG, 900 + e), e) for e in (2, 4, 8)]


def tensors():
    """[(bytes, element size)]: pc.mixed_tensors() -- every element size at counts around 16 and beyond, empty tensors between --
    and the long tensors behind them"""
    return pc.mixed_tensors() + long_tensors()


def index_of(ts, e, count):
    """the first tensor of `ts` with that element size and element count"""
    return next(j for j, (d, te) in enumerate(ts) if te == e and len(d) // te == count)


def np_elements(ts, ranges):
    """the restatement: the bytes of [(tensor, first, count)] back to back"""
    return b"".join(ts[j][0][f * ts[j][1]:(f + c) * ts[j][1]] for j, f, c in ranges)


def first_members(ts):
    out, m = [], 0
    for _, e in ts:
        out.append(m)
        m += e
    return out


def expand(ts, ranges, member_offsets):
    """the byte ranges an element range becomes: one per plane of its tensor"""
    fm = first_members(ts)
    return [(member_offsets[fm[j] + p] + f, c) for j, f, c in ranges for p in range(ts[j][1])]


def container(stream, ts, how="concatenation"):
    """the streams of the planes of `ts` (stream: bytes -> an orz stream) as (blob, member table or None, the streams)"""
    blobs = [stream(pl) for pl in pc.planes_of(ts)]
    if how == "concatenation":
        return b"".join(blobs), None, blobs
    order = list(range(len(blobs)))
    random.Random(len(blobs)).shuffle(order)
    blob, table = pc.table_of(blobs, order=order)
    return blob, table, blobs


def mixed_batch(ts):
    """ranges that mix tensors and element sizes: out of order, repeated, overlapping, empty, a single-byte tensor in the middle"""
    j2, j4, j8 = (index_of(ts, e, LONG) for e in (2, 4, 8))
    b17, b15 = index_of(ts, 1, 17), index_of(ts, 1, 15)
    s16, q17 = index_of(ts, 2, 16), index_of(ts, 8, 17)
    empty = next(j for j, (d, _) in enumerate(ts) if not d)
    return [(j8, 1000, 29), (j2, 3, 40), (s16, 0, 16), (j4, 0, 0), (j2, 3, 40), (b17, 1, 16), (j4, 15, 34), (j4, 31, 3), (empty, 0, 0),
            (q17, 16, 1), (b15, 0, 15), (j2, 17, 1), (j8, 0, 17), (j4, LONG, 0), (j4, 1, 1)]


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def _u32(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


# ------------------------------------------------------------------------------------------------ the gather alone
def gather(lib, ts, ranges, rem, plane_rem=0, bad_plane=None):
    """ONE ElementGather launch: the planes of `ts` at multiples of 16 plus plane_rem in one arena, the output at an address that
    is `rem` modulo 16 in a poisoned arena with guard gaps.  bad_plane: that plane's status is a failed decode.
    Returns (units, the output arena, where the output starts in it, the arena of planes before, after)."""
    planes = pc.planes_of(ts)
    offs, plen = pc.layout([len(p) for p in planes], [plane_rem] * len(planes))
    src = pc.Arena(plen, align=16)
    for o, p in zip(offs, planes):
        src.write(o, p)
    before = src.bytes()
    total = len(np_elements(ts, ranges))
    (at,), alen = pc.layout([total], [rem])
    dst = pc.Arena(alen, align=16)
    assert (dst.base + at) % 16 == rem
    status = [0] * len(planes)
    if bad_plane is not None:
        status[bad_plane] = 1
    units = lib.emu_element_gather(ctypes.c_size_t(len(ranges)), _u64([r[0] for r in ranges]), _u64([r[1] for r in ranges]),
                                   _u64([r[2] for r in ranges]), ctypes.c_size_t(len(ts)), _u32([e for _, e in ts]),
                                   _u64([src.base + o for o in offs]), _u32(status), ctypes.c_void_p(dst.base + at))
    return units, dst.bytes(), at, before, src.bytes()


def units_of(first, count):
    return (first + count + 15) // 16 - first // 16 if count else 0


# ------------------------------------------------------------------------------------------------ the reader
class ElemRead:
    pass


class ElemReader(cc.CachedEmuReader):
    """cc.CachedEmuReader on the twin that has the element calls"""

    def set_planes(self, elems, null=False):
        """(rc, message)"""
        err = ctypes.create_string_buffer(256)
        got = self.lib.emu_reader_set_planes(ctypes.c_void_p(self.h), None if null else _u32(elems), ctypes.c_size_t(len(elems)), err,
                                             ctypes.c_size_t(256))
        return got, err.value.decode()

    def tensor_info(self):
        """[(element count, element size)]"""
        n = ctypes.c_uint64()
        cap = self.members + 1
        counts, elems = (ctypes.c_uint64 * cap)(), (ctypes.c_uint32 * cap)()
        self.lib.emu_reader_tensor_info(ctypes.c_void_p(self.h), ctypes.byref(n), counts, elems, ctypes.c_size_t(cap))
        return [(counts[j], elems[j]) for j in range(n.value)]

    def read_elements(self, ranges, want_bytes=0, cap=None, rem=0, slots=0, null_arrays=False, raw=None):
        """the ranges into `cap` bytes (default: want_bytes, what they ask for) at an address that is `rem` modulo 16 inside a
        poisoned arena with guard gaps; raw = (address, capacity) instead: a buffer of the caller's"""
        r = ElemRead()
        cap = want_bytes if cap is None else cap
        (at,), alen = pc.layout([cap], [rem])
        arena = pc.Arena(alen, align=16)
        dst, dcap = (arena.base + at, cap) if raw is None else raw
        dl = ctypes.c_uint64()
        st = (ctypes.c_uint64 * 6)()
        err = ctypes.create_string_buffer(256)
        cols = [None] * 3 if null_arrays else [_u64([q[i] for q in ranges]) for i in range(3)]
        r.rc = self.lib.emu_reader_read_elements(ctypes.c_void_p(self.h), cols[0], cols[1], cols[2], ctypes.c_size_t(len(ranges)),
                                                 ctypes.c_void_p(dst), ctypes.c_size_t(dcap), slots, ctypes.byref(dl), st, err,
                                                 ctypes.c_size_t(256))
        r.err, r.dst_len = err.value.decode(), dl.value
        r.ranges, r.members_decoded, r.decoded_bytes, r.out_bytes, r.launches, r.host_waits = list(st)
        r.arena, r.at, r.arena_len = arena.bytes(), at, alen
        r.out = r.arena[at:at + r.dst_len] if r.rc == 0 else None
        r.untouched = r.arena == bytes([POISON]) * alen
        return r

    def close(self):
        if self.h:
            self.lib.emu_elements_close(ctypes.c_void_p(self.h))
            self.h = None
