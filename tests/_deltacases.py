"""Shared by the two tiers of the delta tests (test_delta_emu.py, test_gpu_delta.py): tensors with bases, XOR restated in numpy, the
emulation twin (tests/emu/emu_delta.cpp: PlaneSplitDelta / PlaneMergeDelta alone, and decode_members_planes with bases) behind the
Python faces of _planecases and _crccases, and the issue's bf16 weights with their successor."""
import ctypes
import os
import subprocess

import numpy as np

import _crccases as cc
import _piececases as pp
import _planecases as pc

ROOT = pc.ROOT
ENOMEM, EINVAL, EBADMSG = cc.ENOMEM, cc.EINVAL, cc.EBADMSG
GUARD, POISON, MASK = pc.GUARD, pc.POISON, pc.MASK
ELEMS, COUNTS = pc.ELEMS, pc.COUNTS
REMS = (0, 1, "e", 8)  # address remainders modulo 16; "e": the tensor's element size
PIECE = 32

_u64, _u32 = pc._u64, pc._u32


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_delta.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_delta.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_crc.cpp", "emu_plane_pieces.cpp", "emu_elements.cpp", "emu_reader_cache.cpp",
                                                                     "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_delta_move.restype = ctypes.c_uint64
    return lib


# ------------------------------------------------------------------------------------------------ the cases
def xor(a, b):
    """a XOR b, byte by byte; b None: a"""
    if b is None:
        return bytes(a)
    assert len(a) == len(b)
    return (np.frombuffer(bytes(a), dtype=np.uint8) ^ np.frombuffer(bytes(b), dtype=np.uint8)).tobytes()


def with_bases(ts, seed=77):
    """[base or None] for [(bytes, element size)]: random bytes of the tensor's size; about half of the tensors -- and every empty
    one -- have none, in a pattern that drifts against mixed_tensors' groups of five, so that rows with and without a base of
    every element size stand side by side"""
    return [None if (k % 5 + 3 * (k // 5)) % 4 < 2 or not d else pc.tensor_bytes(e, len(d) // e, seed + k) for k, (d, e) in enumerate(ts)]


def mixed():
    """(tensors, bases): every element size at every count of the issue in ONE list, with and without a base"""
    ts = pc.mixed_tensors()
    bases = with_bases(ts)
    # every element size with and without a base, among the tensors with full units and a partial one
    assert {(e, b is not None) for (d, e), b in zip(ts, bases) if len(d) // e > 1000} == {(e, h) for e in ELEMS for h in (False, True)}
    return ts, bases


def deltas(ts, bases):
    """[(tensor XOR base, element size)]: what the members of a delta container hold"""
    return [(xor(d, b), e) for (d, e), b in zip(ts, bases)]


def rems_for(ts, rem):
    return [(e if rem == "e" else rem) % 16 for _, e in ts]


def staged(ts, bases):
    """whether tensor k is a row of the delta kernels, as the drivers make them: more than one byte an element, or a base"""
    return [e > 1 or b is not None for (_, e), b in zip(ts, bases)]


def staging_layout(ts, rows):
    """the planes of every row at a multiple of 256, pitch apart: ([offset of plane 0, or None], staging length)"""
    at, offs = 256, []
    for (data, e), row in zip(ts, rows):
        if not row:
            offs.append(None)
            continue
        offs.append(at)
        at = (at + e * pc.pitch(len(data) // e) + 255) // 256 * 256
    return offs, at + 256


def plane_pieces(ts, rows, stage_offs):
    """[(offset, bytes)]: the planes of the rows of `ts` where staging_layout put them"""
    out = []
    for (d, e), row, so in zip(ts, rows, stage_offs):
        if row:
            out += [(so + p * pc.pitch(len(d) // e), pl) for p, pl in enumerate(pc.np_split(d, e))]
    return out


def move(lib, merge, ts, rows, inter, inter_offs, base, base_offs, stage, stage_offs):
    """ONE PlaneSplitDelta (merge = False) or PlaneMergeDelta launch over the rows; base_offs[k] None: no base.  Returns its units."""
    r = [(inter.base + io, (base.base + bo if bo is not None else 0), stage.base + so, len(d) // e, e)
         for (d, e), row, io, bo, so in zip(ts, rows, inter_offs, base_offs, stage_offs) if row]
    return lib.emu_delta_move(1 if merge else 0, ctypes.c_size_t(len(r)), _u64([x[0] for x in r]), _u64([x[1] for x in r]), _u64([x[2] for x in r]),
                              _u64([x[3] for x in r]), _u32([x[4] for x in r]))


# ------------------------------------------------------------------------------------------------ the decode driver
def decode_delta(lib, blob, table, spots, bases, elems, pieces, crcs, arena_len, prefill=(), verify=True, on_device=True, slots=0):
    """decode_members_planes with bases on the emulation.  spots: (offset in the arena or None, capacity) per destination; bases:
    per destination None, an offset in the arena, or ("abs", address); bases=None: the call without the column.  prefill: (offset,
    bytes) written into the poisoned arena first.  crcs None: no digest check.  Returns cc.decode_verified's answers."""
    blob = bytes(blob)
    arena = pc.Arena(max(arena_len, 1), align=16)
    for o, b in prefill:
        arena.write(o, b)
    keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
    nd = len(spots)
    dsts = (ctypes.c_void_p * max(nd, 1))(*[(arena.base + o if o is not None else None) for o, _ in spots])
    bs = None if bases is None else _u64([0 if b is None else (b[1] if isinstance(b, tuple) else arena.base + b) for b in bases])
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    out_lens = (ctypes.c_uint64 * max(nd, 1))(*([MASK] * max(nd, 1)))
    out_crcs = (ctypes.c_uint32 * max(nd, 1))(*([0xDEADBEEF] * max(nd, 1)))
    m = ctypes.c_uint64()
    st, bad = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r = pc.Decoded()
    r.before = arena.bytes()[:arena_len]
    r.rc = lib.emu_decode_delta(ctypes.cast(keep, ctypes.c_void_p), ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                ctypes.c_size_t(len(table) if table is not None else 0), dsts, _u64([c for _, c in spots]), bs,
                                None if elems is None else _u32(elems), None if pieces is None else _u32(pieces), ctypes.c_size_t(nd),
                                _u32(crcs if crcs is not None else [0] * nd), 1 if verify and crcs is not None else 0, slots, out_lens, out_crcs,
                                ctypes.byref(m), st, bad, err, ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens, r.out_crcs = list(out_lens[:nd]), list(out_crcs[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.bad = tuple(bad)
    r.arena = arena.bytes()[:arena_len]
    r.base = arena.base
    return r


def places(ts, bases, room=9, rem=None):
    """destinations in reverse order and, behind them, the bases given out of place, in one arena: ([destination offset],
    [capacity], [base offset or None], arena length, [(offset, base bytes)] to write first).  rem None: destinations at their
    element size modulo 16, bases at remainders of their own; else everything at `rem` ("e": the element size)"""
    caps = [len(d) + room for d, _ in ts]
    sizes = caps + [len(b) for b in bases if b is not None]
    if rem is None:
        rems = [e % 16 for _, e in ts] + [(3 * k) % 16 for k, b in enumerate(bases) if b is not None]
    else:
        rems = rems_for(ts, rem) + [r for r, b in zip(rems_for(ts, rem), bases) if b is not None]
    offs, total = pc.layout(sizes, rems, reverse=True)
    it = iter(offs[len(ts):])
    base_offs = [next(it) if b is not None else None for b in bases]
    return offs[:len(ts)], caps, base_offs, total, [(o, b) for o, b in zip(base_offs, bases) if b is not None]


# ------------------------------------------------------------------------------------------------ the issue's weights
def bf16_step(count=1 << 19, lr=1e-4):
    """(w, tuned) as bytes: w = randn(count, seed 1) * 0.02 and tuned = w + randn(count, seed 5) * lr, both cast to bf16"""
    import torch

    w = torch.randn(count, generator=torch.Generator().manual_seed(1)) * 0.02
    d = torch.randn(count, generator=torch.Generator().manual_seed(5))
    as_bytes = lambda t: t.to(torch.bfloat16).view(torch.int16).numpy().tobytes()  # noqa: E731
    return as_bytes(w), as_bytes(w + d * lr)


def planes_size(stream, data, e, S=0):
    """the size of the container of `data`'s planes (pieces of S elements) at `stream`: bytes -> an orz stream"""
    return sum(len(stream(m)) for m in pp.cut(data, e, S))
