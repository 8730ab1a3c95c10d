"""Shared by the two tiers of the tests of base-aware reads (test_reader_bases_emu.py, test_gpu_reader_bases.py): the emulation
twin (tests/emu/emu_reader_bases.cpp: the reader with set_bases, and ElementGatherDelta / ElementGatherDeltaPieces alone) behind the
Python faces of _elemcases, _piececases and _deltacases, and arenas that hold a launch's output and its base slices together."""
import ctypes
import os
import subprocess

import _deltacases as dc
import _elemcases as ec
import _piececases as pp
import _planecases as pc

ROOT = pc.ROOT
ENOMEM, EINVAL = pc.ENOMEM, pc.EINVAL
GUARD, POISON = pc.GUARD, pc.POISON
LONG = ec.LONG
PIECE = 32

_u64, _u32 = pc._u64, pc._u32


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_reader_bases.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_reader_bases.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_delta.cpp", "emu_crc.cpp", "emu_plane_pieces.cpp", "emu_elements.cpp",
                                                                     "emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_reader_open.restype = ctypes.c_void_p
    lib.emu_reader_cursor_state_bytes.restype = ctypes.c_uint64
    lib.emu_element_gather_delta.restype = ctypes.c_uint64
    return lib


def rem_of(how, e):
    """an address remainder modulo 16 by its name in a test's parameters; "e": the element size"""
    return e % 16 if how == "e" else int(how)


def slice_of(ts, r):
    """the bytes of range r = (tensor, first, count) of [(bytes, element size)]"""
    return ec.np_elements(ts, [r])


# ------------------------------------------------------------------------------------------------ the gather alone
class Gathered:
    pass


def gather(lib, ts, bases, ranges, rem=0, base_rem=0, plane_rem=0, S=0, bad_member=None, in_place=()):
    """ONE ElementGatherDelta launch (S == 0) or ElementGatherDeltaPieces launch (pieces of S elements): the members of the DELTAS
    of `ts` against `bases`, each at a multiple of 16 plus plane_rem in an arena of their own; the ranges' bytes back to back at an
    address that is `rem` modulo 16 in a poisoned arena with guard gaps, and in the SAME arena, behind guard gaps, the base slice
    of every range whose tensor has a base -- only the slice, so a byte read outside it is poison and shows -- at base_rem modulo
    16.  in_place: the ranges (by index) whose base slice lies where the range's bytes go instead.  bad_member: that member's status
    is a failed decode.  Returns .units, .arena (after), .before, .at (the output's offset), .offs (each range's offset in the
    output), .slices ([(offset, bytes)] of the base slices, those in place included), .members_before / .members_after."""
    members, qs = pp.members_of(dc.deltas(ts, bases), S)
    moffs, plen = pc.layout([len(m) for m in members], [plane_rem] * len(members))
    src = pc.Arena(plen, align=16)
    for o, m in zip(moffs, members):
        src.write(o, m)
    g = Gathered()
    g.members_before = src.bytes()
    g.offs, total = [], 0
    for j, f, c in ranges:
        g.offs.append(total)
        total += c * ts[j][1]
    apart = [k for k, (j, f, c) in enumerate(ranges) if bases[j] is not None and c and k not in in_place]
    places, alen = pc.layout([total] + [ranges[k][2] * ts[ranges[k][0]][1] for k in apart], [rem] + [base_rem] * len(apart))
    g.at = places[0]
    arena = pc.Arena(alen, align=16)
    assert (arena.base + g.at) % 16 == rem
    where = dict(zip(apart, places[1:]))
    where.update({k: g.at + g.offs[k] for k in in_place})
    g.slices = [(o, slice_of([(bases[ranges[k][0]], ts[ranges[k][0]][1])], (0,) + tuple(ranges[k][1:]))) for k, o in sorted(where.items())]
    for o, b in g.slices:
        arena.write(o, b)
    g.before = arena.bytes()
    status = [0] * len(members)
    if bad_member is not None:
        status[bad_member] = 1
    psize = [S if q > 1 else max(len(d) // e, 1) for (d, e), q in zip(ts, qs)]
    g.units = lib.emu_element_gather_delta(ctypes.c_size_t(len(ranges)), _u64([r[0] for r in ranges]), _u64([r[1] for r in ranges]),
                                           _u64([r[2] for r in ranges]), _u64(g.offs), _u64([arena.base + where[k] if k in where else 0 for k in range(len(ranges))]),
                                           ctypes.c_size_t(len(ts)), _u32([e for _, e in ts]), _u64(qs) if S else None, _u64(psize) if S else None,
                                           _u64([src.base + o for o in moffs]), _u32(status), ctypes.c_void_p(arena.base + g.at))
    g.arena, g.members_after = arena.bytes(), src.bytes()
    return g


def expect(g, ts, ranges, skip=()):
    """the arena after a launch: as before it, with the ranges' RESTORED bytes -- those of `ts` -- where they go; skip: the ranges (by
    index) that write nothing"""
    return pc.expect_arena(len(g.before), [(0, g.before)] + [(g.at + o, slice_of(ts, r)) for k, (o, r) in enumerate(zip(g.offs, ranges)) if k not in skip])


# ------------------------------------------------------------------------------------------------ the reader
class BaseReader(pp.PieceReader):
    """pp.PieceReader on the twin that has set_bases.  The bases lie in buffers the caller keeps alive."""

    def set_bases(self, addrs, null=False):
        """(rc, message); addrs: an address per tensor, 0 for none"""
        err = ctypes.create_string_buffer(256)
        got = self.lib.emu_reader_set_bases(ctypes.c_void_p(self.h), None if null else _u64(addrs), ctypes.c_size_t(len(addrs)), err, ctypes.c_size_t(256))
        return got, err.value.decode()

    def bases(self):
        """the addresses the reader holds ([] when no bases are set)"""
        n = ctypes.c_uint64()
        out = (ctypes.c_uint64 * (self.members + 1))()
        self.lib.emu_reader_bases(ctypes.c_void_p(self.h), ctypes.byref(n), out, ctypes.c_size_t(self.members + 1))
        return list(out[:n.value])


class Held:
    """the bases of [(bytes, element size)] in ONE arena, each at `rem` modulo 16 ("e": its element size): .addrs for set_bases"""

    def __init__(self, ts, bases, rem=0):
        sizes = [len(b) if b is not None else 0 for b in bases]
        self.offs, total = pc.layout(sizes, [rem_of(rem, e) for _, e in ts])
        self.arena = pc.Arena(total, align=16)
        for o, b in zip(self.offs, bases):
            if b is not None:
                self.arena.write(o, b)
        self.addrs = [self.arena.base + o if b is not None else 0 for o, b in zip(self.offs, bases)]
        self.before = self.arena.bytes()

    def untouched(self):
        return self.arena.bytes() == self.before
