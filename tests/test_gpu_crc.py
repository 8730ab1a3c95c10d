"""GPU tier: the CRC-32 kernels (orz_crc32_buffers through orz_amd.crc32_buffers) against zlib.crc32 -- ONE call over every
buffer of _crccases.buffers() laid out in a poisoned arena with guard gaps, exactly what tests/test_crc_emu.py runs on the
emulation -- and one buffer of more than 4 GiB, where the fold's bit count and the tile offsets pass 2^32."""
import zlib

import pytest

import _crccases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def digests():
    """(buffers, digests from ONE call, the arena before, the arena after)"""
    import orz_amd
    import torch

    torch.cuda.init()
    bufs = cc.buffers()
    host, offs = cc.crc_arena(bufs)
    before = host.bytes()
    arena = torch.frombuffer(bytearray(before), dtype=torch.uint8).to("cuda:0")
    assert arena.data_ptr() % 16 == 0
    views = [arena[o:o + len(d)] for o, (d, _) in zip(offs, bufs)]
    assert all(v.data_ptr() % 16 == r for v, (d, r) in zip(views, bufs) if d)
    got = orz_amd.crc32_buffers(views, device=0)
    torch.cuda.synchronize()
    return bufs, got, before, bytes(arena.cpu().numpy())


def test_every_buffer_has_zlibs_digest(digests):
    bufs, got, before, after = digests
    want = cc.zlib_crcs(bufs)
    assert len(got) == len(want) > 64
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "buffer %d (%d bytes at %d mod 16): 0x%08x, zlib says 0x%08x" % (k, len(bufs[k][0]), bufs[k][1], g, w)
    assert after == before


def test_the_emulation_agrees(digests):
    bufs, got = digests[0], digests[1]
    assert cc.emu_crcs(cc.emu_lib(), bufs)[0] == got


def test_no_tensors_and_empty_ones():
    import orz_amd
    import torch

    assert orz_amd.crc32_buffers([], device=0) == []
    e = torch.empty(0, dtype=torch.float32, device="cuda:0")
    assert orz_amd.crc32_buffers([e, e], device=0) == [0, 0]
    with pytest.raises(ValueError):
        orz_amd.crc32_buffers([e, torch.empty(0)], device=0)


def _crc_zeros(n):
    """zlib's digest of n zero bytes, by doubling with the GF(2) restatement"""
    crc, have, chunk = 0, 0, (zlib.crc32(b"\0"), 1)
    while n:
        if n & 1:
            crc, have = cc.np_combine(crc, chunk[0], chunk[1]), have + chunk[1]
        chunk = (cc.np_combine(chunk[0], chunk[0], chunk[1]), 2 * chunk[1])
        n >>= 1
    return crc


def test_a_buffer_of_more_than_4_gib():
    """zeros between two short random runs, starting 7 bytes off a multiple of 16: 65,537 tiles, bytes behind a tile beyond 2^32"""
    import orz_amd
    import torch

    n = (1 << 32) + 5
    a, b = cc._random(40, 1), cc._random(1029, 2)
    assert _crc_zeros(5000) == zlib.crc32(b"\0" * 5000)
    big = torch.zeros(7 + len(a) + n + len(b), dtype=torch.uint8, device="cuda:0")
    buf = big[7:]
    buf[:len(a)] = torch.frombuffer(bytearray(a), dtype=torch.uint8).to("cuda:0")
    buf[len(a) + n:] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")
    want = cc.np_combine(cc.np_combine(zlib.crc32(a), _crc_zeros(n), n), zlib.crc32(b), len(b))
    small = buf[:len(a) + 100]
    got = orz_amd.crc32_buffers([small, buf, buf[len(a) + n:]], device=0)
    assert got == [zlib.crc32(a + b"\0" * 100), want, zlib.crc32(b)]
    assert orz_amd.crc32_combine(orz_amd.crc32_combine(zlib.crc32(a), _crc_zeros(n), n), zlib.crc32(b), len(b)) == want
