"""The CRC-32 kernels (orz_amd/csrc/orz_crc.h) on the emulation backend: ONE call -- three launches -- over every buffer of
_crccases.buffers() in a poisoned arena against zlib.crc32, the power function of the fold kernel where the bit count passes
2^32, the combine and the host restatement."""
import ctypes
import zlib

import pytest

import _crccases as cc
from _crccases import TILE


@pytest.fixture(scope="module")
def lib():
    return cc.emu_lib()


@pytest.fixture(scope="module")
def digests(lib):
    """every buffer of the cases in one call, once: (buffers, digests, launches, host waits, arena before, arena after)"""
    bufs = cc.buffers()
    return (bufs,) + cc.emu_crcs(lib, bufs)


def test_the_cases_cover_what_they_claim(lib):
    assert lib.emu_crc_tile_bytes() == TILE and TILE % 1024 == 0
    assert lib.emu_crc_lds_bytes() == 16 * 1024
    bufs = cc.buffers()
    assert len(bufs) > 64
    lengths = {len(d) for d, _ in bufs}
    assert {0, 1, 15, 16, 17, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 37} <= lengths and max(lengths) > 4 * TILE
    for n in cc.LENGTHS:
        assert {r for d, r in bufs if len(d) == n} >= set(cc.REMS), n
    assert any(not a and b and c for (a, _), (b, _), (c, _) in zip(bufs, bufs[1:], bufs[2:]))  # empty buffers between the others
    assert any(d and not any(d) for d, _ in bufs) and any(d and all(b == 0xFF for b in d) for d, _ in bufs)
    # a buffer of fewer bytes than its head has one tile; one that ends inside a word, a row and a tile each appear
    assert lib.emu_crc_tiles(1, 3) == 1 and lib.emu_crc_tiles(16, 0) == 0 and lib.emu_crc_tiles(1, 15 + TILE) == 1 and lib.emu_crc_tiles(1, 16 + TILE) == 2


def test_every_buffer_has_zlibs_digest(digests):
    bufs, got, launches, waits, before, after = digests
    want = cc.zlib_crcs(bufs)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "buffer %d (%d bytes at %d mod 16): 0x%08x, zlib says 0x%08x" % (k, len(bufs[k][0]), bufs[k][1], g, w)
    assert (launches, waits) == (3, 2)
    assert after == before


def test_buffers_that_differ_in_one_byte_or_in_leading_zeros_differ_in_digest(digests):
    bufs, got = digests[0], digests[1]
    by_len = {}
    for (d, _), g in zip(bufs, got):
        by_len.setdefault(len(d), {})[d] = g
    for n in (1, 16, 1040, TILE + 40, 2 * TILE + 37):
        assert len(set(by_len[n].values())) == len(by_len[n]) >= 3, n
    tail = [g for (d, r), g in zip(bufs, got) if r == 2 and d.endswith(bufs[-1][0][-50:])]
    assert len(tail) == len(set(tail)) == 4


def test_no_buffers_and_only_empty_ones(lib):
    assert cc.emu_crcs(lib, [])[:3] == ([], 0, 0)
    got, launches, waits, _, _ = cc.emu_crcs(lib, [(b"", 0), (b"", 5)])
    assert got == [0, 0] and (launches, waits) == (1, 2)  # (no tiles: only the sums are launched)


BIG = ((1 << 29) - 1, 1 << 29, (1 << 32) + 5, 1 << 40)


@pytest.mark.parametrize("len_b", BIG)
def test_the_power_function_beyond_32_bits(lib, len_b):
    want = cc.xpow(8 * len_b)
    assert lib.emu_crc_xpow_bytes(len_b) == want
    a, b = 0x12345678, 0x9ABCDEF0
    assert lib.emu_crc_combine(a, b, len_b) == cc.np_combine(a, b, len_b)


def test_the_restatement_knows_small_powers():
    assert cc.xpow(0) == 0x80000000 and cc.xpow(1) == 0x40000000 and cc.xpow(31) == 1 and cc.xpow(32) == cc.POLY
    # x^(8 n) carries a digest over n zero bytes: crc(A + B) from crc(A), crc(B)
    a, b = b"hello, ", b"world" * 40
    assert cc.np_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)


def test_combine_equals_zlib_over_the_concatenation(lib):
    data = cc._random(3000, 5)
    for cut in (0, 1, 1500, len(data)):
        a, b = data[:cut], data[cut:]
        assert lib.emu_crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)


def test_the_host_restatement(lib):
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 4099):
        d = cc._random(n, n)
        buf = ctypes.create_string_buffer(d, max(n, 1))
        assert lib.emu_crc_host(buf, ctypes.c_size_t(n)) == zlib.crc32(d), n
