"""GPU tier of tests/test_freeparse_decoders.py: the legal streams of the free-parse writer (tests/_freeparse.py; the same named
cases, which the CPU tier holds to the oracle) through the device decoder itself -- decode_members_device, decode_members_into
with every member in a buffer of its own between guard bands, and MemberReader.read_ranges at the chunk-edge ranges with and
without the cursor cache.  Bars: the known data, byte for byte, and what the emulation twin returned for the same container.
Everything decodes in one launch per call; the members are 6 KB at most."""
import ctypes

import pytest

import _cachecases as cc
import _freeparse as fp
import _scattercases as sc

pytestmark = pytest.mark.gpu


def _dev(data, device=0):
    import torch

    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)[: len(data)].to("cuda:%d" % device)


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def legal(oracle):
    import torch

    torch.zeros(1, device="cuda:0")  # (torch opens the device before the library does: the order every GPU test here keeps)
    suites = fp.load_cases()
    for cases in suites.values():
        for c in cases:
            oracle.assert_decodes_to(c.stream, c.data, "free-parse stream " + c.name)
    assert sum(c.counters["overruns_past_end_followed"] for c in suites["end-overrun"]) >= 12
    parts, streams = fp.container(suites, oracle)
    assert len(parts) >= 24 and max(len(p) for p in parts) <= 6000
    return suites, parts, streams


def test_decode_members_device(legal, emu):
    import orz_amd

    _, parts, streams = legal
    blob = b"".join(streams)
    out, m = orz_amd.decode_members_device(blob)
    assert m == len(parts) and out == b"".join(parts)
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, em = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    assert emu.lib.emu_decode_members(blob, ctypes.c_size_t(len(blob)), 5, ctypes.byref(dst), ctypes.byref(n), ctypes.byref(em), err,
                                      ctypes.c_size_t(256)) == 0, err.value
    twin = ctypes.string_at(dst, n.value)
    emu.lib.emu_free(dst)
    assert out == twin and em.value == m


def test_members_into_buffers_of_their_own(legal):
    import torch

    import orz_amd

    _, parts, streams = legal
    caps = [len(p) for p in parts]
    offs, total = sc.reverse_layout(caps)
    arena = torch.full((total,), sc.POISON, dtype=torch.uint8, device="cuda:0")
    sizes = orz_amd.decode_members_into(_dev(b"".join(streams)), [arena[o:o + c] for o, c in zip(offs, caps)])
    assert sizes == caps
    got = _host(arena)
    sc.check_arena(got, offs, caps, parts)  # (the guard bands are whole: no overrun stored a byte outside its member)
    twin = sc.scatter(sc.emu_lib(), b"".join(streams), None, list(zip(offs, caps)), total)
    assert twin.rc == 0 and twin.arena == got


@pytest.mark.parametrize("cache", ["no cache", "cursor cache"])
def test_read_ranges_at_the_chunk_edges(legal, cache):
    import orz_amd

    suites, parts, streams = legal
    whole, blob = b"".join(parts), b"".join(streams)
    budget = len(parts) * cc.cost(6400, orz_amd.MemberReader.cursor_state_bytes()) if cache == "cursor cache" else 0
    rd = orz_amd.MemberReader(_dev(blob), cache_bytes=budget)
    twin = cc.CachedEmuReader(cc.emu_lib(), blob)
    assert twin.h, twin.err
    try:
        assert orz_amd.MemberReader.cursor_state_bytes() == twin.state_bytes
        if budget:
            twin.set_cache(budget)
        assert rd.total == len(whole)
        for k, batch in enumerate(fp.read_rounds(parts, suites)):
            ranges = [(o, ln) for o, ln, _ in batch]
            out = _host(rd.read_ranges(ranges))
            e = twin.read(ranges)
            assert e.rc == 0, e.err
            at = 0
            for o, ln, what in batch:
                assert out[at:at + ln] == whole[o:o + ln], (k, what, o, ln)
                at += ln
            assert out == e.out and len(out) == at
            if budget:
                assert rd.cache_stats() == twin.cache_stats()
    finally:
        rd.close()
        twin.close()


def test_a_member_across_the_window_slide(oracle):
    """one member a little longer than 2^24 bytes, the smallest at which a slide exists: a chunk that ends exactly at the block's
    end, and behind the slide a match from the ring node of member offset 2 -- window offset 1 by then, the last one alive"""
    import torch

    import orz_amd

    torch.zeros(1, device="cuda:0")
    data, stream, c = fp.write_slide()
    oracle.assert_decodes_to(stream, data, "free-parse stream across the slide")
    assert c["slides"] == 1 and fp.NEW in c["map"]["chunk_ends"] and c["slide_match"] == [fp.NEW + 1000]
    out, m = orz_amd.decode_members_device(stream)
    assert m == 1 and out == data
    again = fp.NEW + 1000
    ranges = [(0, 50), (fp.NEW - 100, 200), (again - 10, 60), (len(data) - 9, 9)]
    rd = orz_amd.MemberReader(_dev(stream), cache_bytes=cc.cost(len(data), orz_amd.MemberReader.cursor_state_bytes()))
    try:
        for o, ln in ranges:  # (the cursor stops in front of the slide, then goes on across it)
            assert _host(rd.read(o, ln)) == data[o:o + ln], (o, ln)
    finally:
        rd.close()
