"""Shared by the two tiers of the reader cache's tests (test_reader_cache_emu.py, test_gpu_reader_cache.py): the emulation twin
with the cache calls (tests/emu/emu_reader_cache.cpp) behind the Python face of _rangecases, the cost formula, and where the
chunks of a stream end in its decoded bytes."""
import ctypes
import os
import subprocess

import _rangecases as rc

ROOT = rc.ROOT
PRE = ((1 << 25) - 1) // 2  # SBVEC_PREMATCH_LEN: a chunk's end field counts from here (orz_common.h)
STAT_NAMES = ("hits", "resumed", "fresh", "uncached", "evicted", "cursors", "bytes", "budget")


def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_reader_cache.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_reader_cache.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_decode_range.cpp", "emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.emu_reader_open.restype = ctypes.c_void_p
    lib.emu_reader_cursor_state_bytes.restype = ctypes.c_uint64
    return lib


def cost(member_bytes, state_bytes):
    """what a cursor of a member that decodes to member_bytes costs of the budget"""
    return (member_bytes + 255) // 256 * 256 + state_bytes


class CachedEmuReader(rc.EmuReader):
    """rc.EmuReader on the twin that has the cache calls"""

    @property
    def state_bytes(self):
        return self.lib.emu_reader_cursor_state_bytes()

    def set_cache(self, nbytes):
        err = ctypes.create_string_buffer(256)
        got = self.lib.emu_reader_set_cache(ctypes.c_void_p(self.h), ctypes.c_uint64(nbytes), err, ctypes.c_size_t(256))
        assert got == 0, err.value

    def cache_stats(self):
        st = (ctypes.c_uint64 * 8)()
        self.lib.emu_reader_cache_stats(ctypes.c_void_p(self.h), st)
        return dict(zip(STAT_NAMES, list(st)))

    def fail_alloc_in(self, calls):
        self.lib.emu_reader_fail_alloc_in(ctypes.c_void_p(self.h), ctypes.c_long(calls))


class _Bits:  # MSB-first, as the decoder reads a chunk
    def __init__(self, data):
        self.data, self.at = data, 0

    def bits(self, k):
        v = 0
        for _ in range(k):
            byte = self.data[self.at >> 3] if self.at >> 3 < len(self.data) else 0
            v = (v << 1) | ((byte >> (7 - (self.at & 7))) & 1)
            self.at += 1
        return v

    def varint(self):
        v, sh = 0, 0
        while True:
            b = self.bits(2)
            v |= (b & 1) << sh
            sh += 1
            if b < 2:
                return v


def chunk_ends(member):
    """the decoded offset at which each chunk of a member of ONE block ends, from the chunks' end fields"""
    out = []
    for k, (_, p, t) in enumerate(rc.chunks(member)):
        br = _Bits(member[p:p + t])
        if k == 0:  # the census
            for _ in range(br.varint()):
                br.bits(9)
        out.append(br.varint() - PRE)
    return out
