"""Shared by the two tiers of the CRC-32 tests (test_crc_emu.py, test_digests_emu.py, test_gpu_crc.py, test_gpu_digests.py): the
buffers every digest launch is held to zlib over, a GF(2) restatement of x^n mod P, the emulation twin (tests/emu/emu_crc.cpp)
behind a small Python face, and the containers of the verified decode."""
import ctypes
import os
import subprocess
import zlib

import numpy as np

import _piececases as pp
import _planecases as pc

ROOT = pc.ROOT
ENOMEM, EINVAL, EBADMSG = -12, -22, -74
POISON, MASK = pc.POISON, pc.MASK
TILE = 64 * 1024  # kCrcTileBytes (the twin says so: test_crc_emu.py)
POLY = 0xEDB88320
REMS = (0, 1, 7, 15)


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_crc.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_crc.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f)
                    for f in ("emu_plane_pieces.cpp", "emu_elements.cpp", "emu_reader_cache.cpp", "emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    for name in ("emu_crc_tile_bytes", "emu_crc_lds_bytes", "emu_crc_xpow_bytes", "emu_crc_combine", "emu_crc_host"):
        getattr(lib, name).restype = ctypes.c_uint32
    lib.emu_crc_tiles.restype = ctypes.c_uint64
    lib.emu_crc_xpow_bytes.argtypes = [ctypes.c_uint64]
    lib.emu_crc_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    lib.emu_crc_tiles.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return lib


_u64, _u32 = pc._u64, pc._u32


# ------------------------------------------------------------------------------------------------ GF(2), restated
def times_x(s):
    """the register one zero bit further: s x mod P (bit 31 is the coefficient of x^0)"""
    return (s >> 1) ^ (POLY if s & 1 else 0)


def mul(a, b):
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = times_x(b)
    return p


def xpow(bits):
    """x^bits mod P by square-and-multiply over Python's unbounded exponent"""
    r, sq = 0x80000000, 0x40000000
    while bits:
        if bits & 1:
            r = mul(r, sq)
        sq = mul(sq, sq)
        bits >>= 1
    return r


def np_combine(a, b, len_b):
    return mul(a, xpow(8 * len_b)) ^ b


# ------------------------------------------------------------------------------------------------ the buffers
LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 37, 4 * TILE + 1024 + 16 * 5 + 3)


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def buffers():
    """[(bytes, address remainder modulo 16)]: every length of LENGTHS at every remainder of REMS, random bytes; all zero and all
    0xFF at lengths on both sides of a word, a row and a tile; pairs that differ in their first byte only and in their last only;
    empty buffers between the others"""
    out = []
    for li, n in enumerate(LENGTHS):
        for rem in REMS:
            out.append((_random(n, 100 * li + rem), rem))
        out.append((b"", li % 16))
    for n in (1, 17, 1025, TILE + 1, 2 * TILE + 37):
        for fill in (0, 0xFF):
            out.append((bytes([fill]) * n, (n + fill) % 16))
    for n, rem in ((1, 3), (16, 0), (1040, 9), (TILE + 40, 15), (2 * TILE + 37, 0)):
        base = bytearray(_random(n, 7000 + n))
        first, last = bytearray(base), bytearray(base)
        first[0] ^= 0x80
        last[-1] ^= 0x01
        out += [(bytes(base), rem), (bytes(first), rem), (b"", 5), (bytes(last), rem)]
    # leading zeros in front of the same bytes: a raw residue cannot tell them apart, the digest must
    tail = _random(50, 9)
    out += [(tail, 2), (b"\0" * 16 + tail, 2), (b"\0" * 1024 + tail, 2), (b"\0" * TILE + tail, 2)]
    return out


def zlib_crcs(bufs):
    return [zlib.crc32(d) & 0xFFFFFFFF for d, _ in bufs]


def crc_arena(bufs):
    """the buffers in one poisoned arena with guard gaps, each at its remainder: (arena, [offset])"""
    offs, total = pc.layout([len(d) for d, _ in bufs], [r for _, r in bufs])
    arena = pc.Arena(total, align=16)
    for o, (d, _) in zip(offs, bufs):
        arena.write(o, d)
    return arena, offs


def emu_crcs(lib, bufs):
    """ONE call over all buffers: (digests, launches, host waits, the arena before, the arena after)"""
    arena, offs = crc_arena(bufs)
    before = arena.bytes()
    n = len(bufs)
    crcs = (ctypes.c_uint32 * max(n, 1))(*([0xDEADBEEF] * max(n, 1)))
    st = (ctypes.c_uint64 * 2)()
    err = ctypes.create_string_buffer(256)
    rc = lib.emu_crc_buffers(_u64([arena.base + o if d else 0 for o, (d, _) in zip(offs, bufs)]), _u64([len(d) for d, _ in bufs]), ctypes.c_size_t(n),
                             crcs, st, err, ctypes.c_size_t(256))
    assert rc == 0, err.value.decode()
    return list(crcs[:n]), st[0], st[1], before, arena.bytes()


# ------------------------------------------------------------------------------------------------ the verified decode
COUNTS = (0, 1, 17, 4097)
PIECE = 32


def crcs_of(ts):
    return [zlib.crc32(d) & 0xFFFFFFFF for d, _ in ts]


def places(ts, room=9):
    """destinations in REVERSE order in the arena, at addresses that are the element size modulo 16, `room` bytes of capacity
    behind each size: ([offset], [capacity], arena length)"""
    caps = [len(d) + room for d, _ in ts]
    offs, total = pc.layout(caps, [e % 16 for _, e in ts], reverse=True)
    return offs, caps, total


def decode_verified(lib, blob, table, spots, elems, pieces, crcs, arena_len, verify=True, on_device=True, sizing=False, slots=0, null_crcs=False):
    """decode_members_planes with a digest check on the emulation (verify=False: the same call without one, with ALL its launches
    counted too).  elems / pieces None: NULL.  Returns rc / err / members / out_lens / out_crcs / launches / host_waits / arena /
    bad (destination, expected, computed)."""
    blob = bytes(blob)
    arena = pc.Arena(max(arena_len, 1), align=16)
    keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
    nd = len(spots)
    dsts = (ctypes.c_void_p * max(nd, 1))(*[(arena.base + o if o is not None else None) for o, _ in spots])
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    out_lens = (ctypes.c_uint64 * max(nd, 1))(*([MASK] * max(nd, 1)))
    out_crcs = (ctypes.c_uint32 * max(nd, 1))(*([0xDEADBEEF] * max(nd, 1)))
    m = ctypes.c_uint64()
    st, bad = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r = pc.Decoded()
    r.rc = lib.emu_decode_verified(ctypes.cast(keep, ctypes.c_void_p), ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                   ctypes.c_size_t(len(table) if table is not None else 0), None if sizing else dsts, _u64([c for _, c in spots]),
                                   None if elems is None else _u32(elems), None if pieces is None else _u32(pieces), ctypes.c_size_t(nd),
                                   None if null_crcs else _u32(crcs), 1 if verify else 0, slots, out_lens, out_crcs, ctypes.byref(m), st, bad, err,
                                   ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens, r.out_crcs = list(out_lens[:nd]), list(out_crcs[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.bad = tuple(bad)
    r.arena = arena.bytes()[:arena_len]
    return r


def flip(blob, bit):
    out = bytearray(blob)
    out[bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def bf16_weights(count=4096, seed=1):
    """`count` bf16 values of randn * 0.02 as bytes: the weights of the issue's silent-flip measurement"""
    import torch

    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(count, generator=g) * 0.02).to(torch.bfloat16)
    return t.view(torch.int16).numpy().tobytes()
