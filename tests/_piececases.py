"""Shared by the two tiers of the plane-piece tests (test_plane_pieces_emu.py, test_gpu_plane_pieces.py): tensors cut into pieces
in numpy, the containers made of them, restatements of the plan kernel and of what a read touches, and the emulation twin
(tests/emu/emu_plane_pieces.cpp: the decode driver and the reader with pieces, the plan and the gather alone) behind the Python
faces of _planecases and _elemcases."""
import ctypes
import os
import random
import subprocess

import _elemcases as ec
import _planecases as pc
import _rangecases as rc

ROOT = rc.ROOT
ENOMEM, EINVAL = rc.ENOMEM, rc.EINVAL
GUARD, POISON, MASK = pc.GUARD, pc.POISON, pc.MASK
ELEMS = (1, 2, 4, 8)
SIZES = (16, 32, 4096)  # S, elements to a piece


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_plane_pieces.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_plane_pieces.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f)
                    for f in ("emu_elements.cpp", "emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_reader_open.restype = ctypes.c_void_p
    lib.emu_reader_cursor_state_bytes.restype = ctypes.c_uint64
    lib.emu_element_gather.restype = ctypes.c_uint64
    lib.emu_element_gather_pieces.restype = ctypes.c_uint64
    lib.emu_plane_stage_bound.restype = ctypes.c_uint64
    return lib


_u64, _u32 = pc._u64, pc._u32


# ------------------------------------------------------------------------------------------------ the cases
def counts_for(S):
    """the element counts of the issue at a piece size of S, without repeats"""
    return sorted({0, 1, 15, 16, 17, S - 1, S, S + 1, 2 * S, 2 * S + 5, 3 * S + 16})


def pieces_of(count, S):
    """Q: pieces to a plane of `count` elements at a piece size of S (0: never cut)"""
    return -(-count // S) if S and S < count else 1


def cut(data, e, S):
    """the members of one tensor, plane-major: plane 0's pieces, then plane 1's, ..."""
    count = len(data) // e
    Q = pieces_of(count, S)
    if Q == 1:
        return pc.np_split(data, e)
    return [pl[q * S:(q + 1) * S] for pl in pc.np_split(data, e) for q in range(Q)]


def members_of(ts, S):
    """the members of [(bytes, element size)] at a piece size of S, and [Q of each tensor]"""
    return [m for d, e in ts for m in cut(d, e, S)], [pieces_of(len(d) // e, S) for d, e in ts]


def first_members(ts, qs):
    out, m = [], 0
    for (_, e), q in zip(ts, qs):
        out.append(m)
        m += e * q
    return out


def tensors(S, elems=ELEMS, seed=0):
    """[(bytes, element size)]: every count of counts_for(S), element sizes alternating, so that tensors of one piece and of
    several interleave"""
    out = []
    for ci, c in enumerate(counts_for(S)):
        e = elems[(ci + seed) % len(elems)]
        out.append((pc.tensor_bytes(e, c, 50 * seed + len(out)), e))
    return out


def container(stream, ts, S, how="concatenation"):
    """the streams of the pieces of `ts` (stream: bytes -> an orz stream) as (blob, member table or None, the streams, [Q])"""
    members, qs = members_of(ts, S)
    blobs = [stream(m) for m in members]
    if how == "concatenation":
        return b"".join(blobs), None, blobs, qs
    order = list(range(len(blobs)))
    random.Random(len(blobs)).shuffle(order)
    blob, table = pc.table_of(blobs, order=order)
    return blob, table, blobs, qs


# ------------------------------------------------------------------------------------------------ the decode driver
def decode_pieces(lib, blob, table, places, elems, pieces, arena_len, on_device=True, sizing=False, slots=0, fill=POISON):
    """pc.decode_planes with pieces[j] pieces to a plane of destination j"""
    blob = bytes(blob)
    arena = pc.Arena(max(arena_len, 1), align=16, fill=fill)
    keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
    nd = len(places)
    dsts = (ctypes.c_void_p * max(nd, 1))(*[(arena.base + o if o is not None else None) for o, _ in places])
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    out_lens = (ctypes.c_uint64 * max(nd, 1))(*([MASK] * max(nd, 1)))
    m = ctypes.c_uint64()
    st = (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r = pc.Decoded()
    r.rc = lib.emu_decode_pieces(ctypes.cast(keep, ctypes.c_void_p), ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                 ctypes.c_size_t(len(table) if table is not None else 0), None if sizing else dsts, _u64([c for _, c in places]),
                                 _u32(elems), _u32(pieces), ctypes.c_size_t(nd), slots, out_lens, ctypes.byref(m), st, err, ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens = list(out_lens[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.arena = arena.bytes()[:arena_len]
    return r


# ------------------------------------------------------------------------------------------------ the plan kernel alone
def plan(lib, dsts, caps, elems, pieces, out_len, base, stage):
    """PlanePlan and PlaneScan over invented columns: a dict of what they wrote (verdict and status: True = a short destination)"""
    J, M = len(dsts), len(out_len)
    out_off = (ctypes.c_uint64 * max(M, 1))()
    verdict, t_elem = (ctypes.c_uint32 * max(J, 1))(), (ctypes.c_uint32 * max(J, 1))()
    cols = [(ctypes.c_uint64 * max(J, 1))() for _ in range(6)]  # units, first, inter, plane0, pitch, count
    rec = (ctypes.c_uint64 * 3)()
    lib.emu_piece_plan(ctypes.c_size_t(J), _u64(dsts), _u64(caps), _u32(elems), _u32(pieces), ctypes.c_size_t(M), _u32(out_len),
                       ctypes.c_uint64(base), ctypes.c_uint64(stage), out_off, verdict, cols[0], cols[1], cols[2], cols[3], cols[4], cols[5],
                       t_elem, rec)
    names = ("units", "first", "inter", "plane0", "pitch", "count")
    got = {n: list(c[:J]) for n, c in zip(names, cols)}
    got.update(out_off=list(out_off[:M]), verdict=[v != 0 for v in verdict[:J]], elem=list(t_elem[:J]), bad=rec[0], total_units=rec[1], status=rec[2] != 0)
    return got


def np_plan(dsts, caps, elems, pieces, out_len, base, stage):
    """the restatement, in Python's unbounded integers reduced modulo 2^64 where the kernel's are"""
    J = len(dsts)
    want = {n: [0] * J for n in ("units", "first", "inter", "plane0", "pitch", "count", "verdict", "elem")}
    want["out_off"] = []
    ix_off, at = [], 0
    for n in out_len:
        ix_off.append(at)
        at += n
    f, units, bad = 0, 0, J
    for j in range(J):
        e, Q = elems[j], pieces[j]
        S, last = out_len[f], out_len[f + Q - 1]
        count = (Q - 1) * S + last
        pitch = (count + 15) // 16 * 16
        place = stage + (ix_off[f] + 15) // 16 * 16 + 32 * f
        for p in range(e):
            for q in range(Q):
                want["out_off"].append(((dsts[j] if e == 1 else place + p * pitch) + q * S - base) & MASK)
        short = caps[j] < count * e
        want["verdict"][j] = short
        if short and bad == J:
            bad = j
        want["units"][j] = 0 if e == 1 else (count + 15) // 16
        want["first"][j] = units
        units += want["units"][j]
        want["inter"][j], want["plane0"][j], want["pitch"][j] = dsts[j], place, pitch
        want["count"][j], want["elem"][j] = (0 if e == 1 else count), e
        f += e * Q
    want.update(bad=bad, total_units=units, status=bad < J)
    return want


# ------------------------------------------------------------------------------------------------ the gather alone
def gather(lib, ts, S, ranges, rem, bad_member=None):
    """ONE ElementGatherPieces launch: the members of `ts` cut at S, each at a multiple of 16 of its own in one arena, the output at
    an address that is `rem` modulo 16 in a poisoned arena with guard gaps.  bad_member: that member's status is a failed decode.
    Returns (units, the output arena, where the output starts in it, the members' arena before, after)."""
    members, qs = members_of(ts, S)
    offs, plen = pc.layout([len(m) for m in members], [0] * len(members))
    src = pc.Arena(plen, align=16)
    for o, m in zip(offs, members):
        src.write(o, m)
    before = src.bytes()
    total = len(ec.np_elements(ts, ranges))
    (at,), alen = pc.layout([total], [rem])
    dst = pc.Arena(alen, align=16)
    status = [0] * len(members)
    if bad_member is not None:
        status[bad_member] = 1
    psize = [S if q > 1 else max(len(d) // e, 1) for (d, e), q in zip(ts, qs)]
    units = lib.emu_element_gather_pieces(ctypes.c_size_t(len(ranges)), _u64([r[0] for r in ranges]), _u64([r[1] for r in ranges]),
                                          _u64([r[2] for r in ranges]), ctypes.c_size_t(len(ts)), _u32([e for _, e in ts]), _u64(qs), _u64(psize),
                                          _u64([src.base + o for o in offs]), _u32(status), ctypes.c_void_p(dst.base + at))
    return units, dst.bytes(), at, before, src.bytes()


# ------------------------------------------------------------------------------------------------ the reader
def expand(ts, qs, S, ranges, member_offsets):
    """the byte ranges an element range becomes: one per plane and per piece it touches"""
    fm = first_members(ts, qs)
    out = []
    for j, f, c in ranges:
        if not c:
            continue
        e, Q = ts[j][1], qs[j]
        P = S if Q > 1 else max(len(ts[j][0]) // e, 1)
        for p in range(e):
            for q in range(f // P, (f + c - 1) // P + 1):
                lo, hi = max(f, q * P), min(f + c, (q + 1) * P)
                out.append((member_offsets[fm[j] + p * Q + q] + lo - q * P, hi - lo))
    return out


class PieceReader(ec.ElemReader):
    """ec.ElemReader on the twin that has the declaration with pieces"""

    def set_planes_pieces(self, elems, pieces, null=False):
        """(rc, message)"""
        err = ctypes.create_string_buffer(256)
        got = self.lib.emu_reader_set_planes_pieces(ctypes.c_void_p(self.h), _u32(elems), None if null else _u32(pieces),
                                                    ctypes.c_size_t(len(elems)), err, ctypes.c_size_t(256))
        return got, err.value.decode()
