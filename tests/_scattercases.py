"""Shared by the two tiers of the scatter decode's tests (test_decode_scatter_emu.py, test_gpu_segments.py): the emulation twin
(tests/emu/emu_decode_scatter.cpp) behind a small Python face, the arena layout with guard gaps, and ScatterPlan restated."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENOMEM, EINVAL = -12, -22
OK, SHORT = 0, 9  # kIxOk, kIxShortDestination (orz_decode_index.h)
GUARD, POISON = 64, 0xA5
MASK = (1 << 64) - 1


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_decode_scatter.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_decode_scatter.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_scatter_plan.restype = None
    return lib


def _u64(values):
    return (ctypes.c_uint64 * max(len(values), 1))(*values)


def plan_reference(dsts, caps, out_len, base):
    """ScatterPlan and ScatterVerdict in plain Python: (out_off, verdict, (members, first bad member, its verdict))"""
    off = [(d - base) & MASK for d in dsts]
    verdict = [SHORT if c < n else OK for c, n in zip(caps, out_len)]
    bad = next((k for k, v in enumerate(verdict) if v != OK), len(dsts))
    return off, verdict, (len(dsts), bad, verdict[bad] if bad < len(dsts) else OK)


def plan_emulated(lib, dsts, caps, out_len, base):
    m = len(dsts)
    off, verdict, sizes = (ctypes.c_uint64 * max(m, 1))(), (ctypes.c_uint32 * max(m, 1))(), (ctypes.c_uint32 * max(m, 1))()
    rec = (ctypes.c_uint64 * 3)()
    lib.emu_scatter_plan(_u64(dsts), _u64(caps), (ctypes.c_uint32 * max(m, 1))(*out_len), ctypes.c_uint64(m), ctypes.c_uint64(base), off,
                         verdict, sizes, rec)
    assert list(sizes[:m]) == list(out_len)
    return list(off[:m]), list(verdict[:m]), tuple(rec)


def reverse_layout(caps, guard=GUARD):
    """destinations of `caps` bytes laid out in REVERSE order in one arena, a guard gap in front of, between and behind them:
    ([offset of destination k], arena length)"""
    at, offs = guard, [0] * len(caps)
    for k in reversed(range(len(caps))):
        offs[k] = at
        at += caps[k] + guard
    return offs, at


class Scattered:
    pass


def scatter(lib, blob, table, places, arena_len, on_device=True, sizing=False, slots=0, n_dsts=None, src_at=None, fill=POISON):
    """decode_members_scatter on the emulation.  `places`: (offset in the arena or None for a null pointer, capacity) per
    destination; the arena is `arena_len` bytes of `fill`.  src_at: the container lies INSIDE the arena at that offset (a
    device-resident container next to the destinations).  Returns rc / err / members / out_lens / launches / host_waits / arena."""
    blob = bytes(blob)
    arena = (ctypes.c_uint8 * max(arena_len, 1)).from_buffer(bytearray(bytes([fill]) * max(arena_len, 1)))
    base = ctypes.addressof(arena)
    if src_at is not None:
        ctypes.memmove(base + src_at, blob, len(blob))
        src = ctypes.c_void_p(base + src_at)
    else:
        keep = ctypes.create_string_buffer(blob, max(len(blob), 1))
        src = ctypes.cast(keep, ctypes.c_void_p)
    nd = len(places) if n_dsts is None else n_dsts
    dsts = (ctypes.c_void_p * max(len(places), 1))(*[(base + o if o is not None else None) for o, _ in places])
    caps = _u64([c for _, c in places])
    offs = _u64([t[0] for t in table]) if table is not None else None
    lens = _u64([t[1] for t in table]) if table is not None else None
    out_lens = (ctypes.c_uint64 * max(nd, 1))(*([MASK] * max(nd, 1)))
    m = ctypes.c_uint64()
    st = (ctypes.c_uint64 * 3)()
    err = ctypes.create_string_buffer(256)
    r = Scattered()
    r.rc = lib.emu_decode_scatter(src, ctypes.c_size_t(len(blob)), 1 if on_device else 0, offs, lens,
                                  ctypes.c_size_t(len(table) if table is not None else 0), None if sizing else dsts, caps, ctypes.c_size_t(nd),
                                  slots, out_lens, ctypes.byref(m), st, err, ctypes.c_size_t(256))
    r.err, r.members = err.value.decode(), m.value
    r.out_lens = list(out_lens[:nd])
    r.launches, r.host_waits = st[0], st[1]
    r.arena = bytes(arena)[:arena_len]
    return r


def check_arena(arena, offs, caps, want, fill=POISON):
    """destination k holds want[k] and every other byte of the arena -- guards, and what lies behind a member in its destination --
    is still poison"""
    expect = bytearray(bytes([fill]) * len(arena))
    for o, c, w in zip(offs, caps, want):
        assert len(w) <= c
        expect[o:o + len(w)] = w
    if arena != bytes(expect):
        k = next(i for i in range(len(arena)) if arena[i] != expect[i])
        raise AssertionError("the arena differs from what was expected from byte %d on" % k)
