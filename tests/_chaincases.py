"""Shared by the two tiers of the chain tests (test_chain_emu.py, test_gpu_chain.py): the steps of a run and the links between them
restated in numpy, the emulation twin (tests/emu/emu_chain.cpp: PlaneMergeChain and ChainPlan alone, and decode_members_chain)
behind the Python faces of _planecases and _deltacases."""
import ctypes
import os
import subprocess
from functools import reduce

import numpy as np

import _crccases as cc
import _deltacases as dc
import _piececases as pp
import _planecases as pc

ROOT = pc.ROOT
ENOMEM, EINVAL, EBADMSG = cc.ENOMEM, cc.EINVAL, cc.EBADMSG
POISON, MASK = pc.POISON, pc.MASK
ELEMS = pc.ELEMS
COUNTS = (0, 1, 15, 16, 17, 31, 33, 4097)
LINKS = (1, 2, 3, 5)

_u64, _u32 = pc._u64, pc._u32


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_chain.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_chain.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_delta.cpp", "emu_crc.cpp", "emu_plane_pieces.cpp", "emu_elements.cpp",
                                                                     "emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_delta_move.restype = ctypes.c_uint64
    lib.emu_chain_move.restype = ctypes.c_uint64
    lib.emu_plane_stage_bound.restype = ctypes.c_uint64
    return lib


def xor_all(datas):
    """the XOR of byte strings of one length"""
    return reduce(dc.xor, datas)


# ------------------------------------------------------------------------------------------------ the kernel alone
def link_tensors(ts, K, seed=300):
    """[[(bytes, element size)] per link]: what each of K links holds of every tensor of `ts` -- random bytes of the tensor's size"""
    return [[(pc.tensor_bytes(e, len(d) // e, seed + 40 * k + j), e) for j, (d, e) in enumerate(ts)] for k in range(K)]


def merged(links, bases):
    """[bytes]: what the merge must write -- the XOR of the links' tensors and the base, if any"""
    return [xor_all([link[j][0] for link in links] + ([b] if b is not None else [])) for j, b in enumerate(bases)]


def chain_move(lib, ts, dst, dst_offs, base, base_offs, stage, link_offs):
    """ONE PlaneMergeChain launch over all of `ts`: link_offs[k][j] = where link k keeps plane 0 of tensor j in `stage`; base_offs[j]
    None: no base.  Returns its units."""
    n, K = len(ts), len(link_offs)
    return lib.emu_chain_move(ctypes.c_size_t(n), _u64([dst.base + o for o in dst_offs]), _u64([0 if o is None else base.base + o for o in base_offs]),
                              _u64([stage.base + link_offs[k][j] for k in range(K) for j in range(n)]), _u64([len(d) // e for d, e in ts]),
                              _u32([e for _, e in ts]), ctypes.c_uint32(K))


def stage_links(ts, links, shift=None):
    """a staging arena with the planes of every link in it, each tensor's at a multiple of 256 (shift: {(k, j): bytes to move that
    tensor's planes of that link off it}): (arena, link_offs)"""
    rows = [True] * len(ts)
    offs, slen = dc.staging_layout(ts, rows)
    slen += 256
    arena = pc.Arena(slen * len(links))
    link_offs = [[o + k * slen + (shift or {}).get((k, j), 0) for j, o in enumerate(offs)] for k in range(len(links))]
    for k, link in enumerate(links):
        for o, pl in dc.plane_pieces(link, rows, link_offs[k]):
            arena.write(o, pl)
    return arena, link_offs


# ------------------------------------------------------------------------------------------------ the steps of a run
SHAPES = ((2, 4097, 0), (4, 4101, 1024), (1, 100, 0))  # (element size, elements, piece size): bf16-shaped whole, float32 in pieces, bytes


def steps(K=3, shapes=SHAPES, seed=3):
    """[[(bytes, element size)] per step], K + 1 steps: step 0 random weights, each further step the one before plus small noise, cast"""
    import torch

    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    cur = []
    for e, c, _ in shapes:
        if e == 1:
            cur.append(rng.integers(0, 256, size=c, dtype=np.uint8))
        else:
            cur.append(torch.randn(c, generator=g) * 0.02)
    out = []
    for _ in range(K + 1):
        step = []
        for (e, c, _), t in zip(shapes, cur):
            if e == 1:
                step.append((t.tobytes(), 1))
            elif e == 2:
                step.append((t.to(torch.bfloat16).view(torch.int16).numpy().tobytes(), 2))
            else:
                step.append((t.to(torch.float32).numpy().tobytes(), 4))
        out.append(step)
        cur = [(t + (rng.integers(0, 8, size=t.size, dtype=np.uint8) == 0)).astype(np.uint8) if isinstance(t, np.ndarray)
               else t + torch.randn(t.numel(), generator=g) * 1e-4 for t in cur]
    return out


def deltas_of(sts):
    """[[(step i + 1 XOR step i, element size)]]: the links between consecutive steps"""
    return [[(dc.xor(b, a), e) for (a, e), (b, _) in zip(prev, nxt)] for prev, nxt in zip(sts, sts[1:])]


def link_members(ts, shapes=SHAPES):
    """the members of one link, each tensor cut at its own piece size, and [Q of each tensor]"""
    return [m for (d, e), (_, _, S) in zip(ts, shapes) for m in pp.cut(d, e, S)], [pp.pieces_of(len(d) // e, S) for (d, e), (_, _, S) in zip(ts, shapes)]


def chain_container(stream, links, shapes=SHAPES, table=False, order=None):
    """(blob, member table or None, [Q], [[stream] per link]): the links' members (stream: bytes -> an orz stream) one link behind the
    other; with a table in one buffer with gaps, the links in `order`"""
    per_link = [[stream(m) for m in link_members(ts, shapes)[0]] for ts in links]
    qs = link_members(links[0], shapes)[1]
    flat = [s for blobs in per_link for s in blobs]
    if not table:
        return b"".join(flat), None, qs, per_link
    blob, tab = pc.table_of(flat, order=list(reversed(range(len(flat)))))
    if order is not None:
        M1 = len(per_link[0])
        tab = [tab[k * M1 + m] for k in order for m in range(M1)]
    return blob, tab, qs, per_link


def decode_chain(lib, blob, table, spots, bases, elems, pieces, crcs, arena_len, links, prefill=(), on_device=True, slots=0):
    """decode_members_chain on the emulation: dc.decode_delta's arguments and answers, and `links`"""
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
    r.rc = lib.emu_decode_chain(ctypes.cast(keep, ctypes.c_void_p), ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                ctypes.c_size_t(len(table) if table is not None else 0), dsts, _u64([c for _, c in spots]), bs,
                                None if elems is None else _u32(elems), None if pieces is None else _u32(pieces), ctypes.c_size_t(nd),
                                _u32(crcs if crcs is not None else [0] * nd), 1 if crcs is not None else 0, slots, ctypes.c_uint32(links), out_lens,
                                out_crcs, ctypes.byref(m), st, bad, err, ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens, r.out_crcs = list(out_lens[:nd]), list(out_crcs[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.bad = tuple(bad)
    r.arena = arena.bytes()[:arena_len]
    r.base = arena.base
    return r


# ------------------------------------------------------------------------------------------------ the plan kernel alone
def plan(lib, dsts, caps, elems, pieces, links, out_len, base, stage):
    """ChainPlan and PlaneScan over invented columns: a dict of what they wrote (verdict and status: True = a short destination)"""
    J, M = len(dsts), len(out_len)
    out_off = (ctypes.c_uint64 * max(M, 1))()
    verdict, t_elem = (ctypes.c_uint32 * max(J, 1))(), (ctypes.c_uint32 * max(J, 1))()
    cols = [(ctypes.c_uint64 * max(J, 1))() for _ in range(5)]  # units, first, inter, pitch, count
    plane0 = (ctypes.c_uint64 * max(J * links, 1))()
    rec = (ctypes.c_uint64 * 3)()
    lib.emu_chain_plan(ctypes.c_size_t(J), _u64(dsts), _u64(caps), _u32(elems), _u32(pieces), ctypes.c_uint32(links), ctypes.c_size_t(M), _u32(out_len),
                       ctypes.c_uint64(base), ctypes.c_uint64(stage), out_off, verdict, cols[0], cols[1], cols[2], plane0, cols[3], cols[4], t_elem, rec)
    got = {n: list(c[:J]) for n, c in zip(("units", "first", "inter", "pitch", "count"), cols)}
    got.update(out_off=list(out_off[:M]), plane0=list(plane0[:J * links]), verdict=[v != 0 for v in verdict[:J]], elem=list(t_elem[:J]), bad=rec[0],
               total_units=rec[1], status=rec[2] != 0)
    return got


def np_plan(dsts, caps, elems, pieces, links, out_len, base, stage):
    """the restatement, in Python's unbounded integers reduced modulo 2^64 where the kernel's are"""
    J = len(dsts)
    M1 = sum(e * q for e, q in zip(elems, pieces))
    assert len(out_len) == links * M1
    want = {n: [0] * J for n in ("units", "first", "inter", "pitch", "count", "verdict", "elem")}
    want["out_off"], want["plane0"] = [], []
    ix_off, at = [], 0
    for n in out_len:
        ix_off.append(at)
        at += n
    units, bad = 0, J
    for k in range(links):
        f = k * M1
        for j in range(J):
            e, Q = elems[j], pieces[j]
            S, last = out_len[f], out_len[f + Q - 1]
            count = (Q - 1) * S + last
            pitch = (count + 15) // 16 * 16
            place = stage + (ix_off[f] + 15) // 16 * 16 + 32 * f
            want["plane0"].append(place)
            want["out_off"] += [(place + p * pitch + q * S - base) & MASK for p in range(e) for q in range(Q)]
            f += e * Q
            if k:
                continue
            short = caps[j] < count * e
            want["verdict"][j] = short
            if short and bad == J:
                bad = j
            want["units"][j], want["first"][j] = (count + 15) // 16, units
            units += want["units"][j]
            want["inter"][j], want["pitch"][j], want["count"][j], want["elem"][j] = dsts[j], pitch, count, e
    want.update(bad=bad, total_units=units, status=bad < J)
    return want
