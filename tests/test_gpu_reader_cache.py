"""GPU tier: the range reader's cursor cache through orz_amd.MemberReader (orz_reader_set_cache / orz_reader_cache_stats).  Bars:
every read equals the Python slice of the known input; a walk through a member decodes every byte once; a second read and a
seek backwards decode nothing and launch nothing; the batch equals the uncached reader under three budgets; a member whose
decode fails loses its cursor and the reader serves on; the statistics of every read equal those of the emulation twin for the
same reads.  Members are a few MB at most: a member decodes on one lane."""
import pytest

import _cachecases as cc
import _rangecases as rc

pytestmark = pytest.mark.gpu

KEYS = ("members_decoded", "decoded_bytes", "out_bytes", "launches", "host_waits")


def _dev(data, device=0):
    import torch

    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)[: len(data)].to("cuda:%d" % device)


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def container(oracle):
    parts = rc.parts()
    return [p for p, _ in parts], [oracle.encode(p, lv) for p, lv in parts]


@pytest.fixture(scope="module")
def text(oracle):
    return rc.damaged_text_member(oracle)


class Pair:
    """a MemberReader on the device and the emulation twin of the same container under the same budget: every read goes to both"""

    def __init__(self, blob, budget, members=None, src=None):
        import orz_amd

        self.src = _dev(blob) if src is None else src
        self.rd = orz_amd.MemberReader(self.src, members=members, cache_bytes=budget)
        self.twin = cc.CachedEmuReader(cc.emu_lib(), blob, members)
        assert self.twin.h, self.twin.err
        self.twin.set_cache(budget)
        assert orz_amd.MemberReader.cursor_state_bytes() == self.twin.state_bytes

    def read(self, ranges, want):
        out, st = self.rd.read_ranges(ranges, stats=True)
        e = self.twin.read(ranges)
        assert e.rc == 0, e.err
        assert _host(out) == e.out == want
        assert {k: st[k] for k in KEYS} == {k: getattr(e, k) for k in KEYS}, (st, {k: getattr(e, k) for k in KEYS})
        cs = self.rd.cache_stats()
        assert cs == self.twin.cache_stats()
        return st, cs

    def close(self):
        self.rd.close()
        self.twin.close()


def test_a_walk_decodes_once_and_a_second_read_decodes_nothing(emu, container, text):
    plain, blobs = container
    data, good, _ = text
    p = Pair(blobs[0] + good + b"".join(blobs[1:]), 1 << 30)
    try:
        base, step, produced = len(plain[0]), 100_000, 0
        for k, lo in enumerate(range(0, len(data), step)):
            stop = min(lo + step, len(data))
            st, cs = p.read([(base + lo, stop - lo)], data[lo:stop])
            assert st["decoded_bytes"] < (stop - produced) + rc.SLACK and st["launches"] == 1 and st["host_waits"] <= 4
            assert st["kernel_ms"] > 0
            assert (cs["hits"], cs["resumed"], cs["fresh"], cs["uncached"]) == (0, 1 if k else 0, 0 if k else 1, 0)
            produced += st["decoded_bytes"]
            # another member's decode between two windows: the LDS the walk's cursor comes back to is not the one it left
            p.read([(base + len(data) + 7000 * k, 500)], plain[2][7000 * k:7000 * k + 500])
        assert produced == len(data)
        for off, ln in ((300_000, 100_000), (0, len(data)), (len(data) - 1, 1)):  # again, backwards, everything
            st, cs = p.read([(base + off, ln)], data[off:off + ln])
            assert st["decoded_bytes"] == 0 and st["launches"] == 0 and st["members_decoded"] == 0 and cs["hits"] == 1
            assert st["kernel_ms"] == 0
    finally:
        p.close()


def test_the_batch_equals_the_uncached_reader_under_three_budgets(emu, container):
    import orz_amd

    plain, blobs = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    ranges = rc.batch(len(data))
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    sb = orz_amd.MemberReader.cursor_state_bytes()
    src = _dev(b"".join(blobs))
    rd = orz_amd.MemberReader(src)
    try:
        ref, ref_st = rd.read_ranges(ranges, stats=True)
        assert _host(ref) == want and ref_st["host_waits"] == 3
    finally:
        rd.close()
    touched = sorted(rc.touched(ranges, lengths))
    everything = sum(cc.cost(lengths[m], sb) for m in touched)
    two = cc.cost(lengths[0], sb) + cc.cost(lengths[2], sb)
    for name, budget, held in (("all members", everything, 6), ("two members", two, 2), ("none fits", cc.cost(1, sb) - 1, 0)):
        p = Pair(b"".join(blobs), budget, src=src)
        try:
            st, cs = p.read(ranges, want)
            assert st["decoded_bytes"] == ref_st["decoded_bytes"] and st["members_decoded"] == 6 and st["host_waits"] <= 4, name
            assert (cs["hits"], cs["fresh"], cs["uncached"], cs["evicted"], cs["cursors"]) == (0, held, 6 - held, 0, held), name
            assert cs["bytes"] == sum(cc.cost(lengths[m], sb) for m in touched[:held]) and cs["budget"] == budget, name
            st, cs = p.read(ranges, want)
            assert (cs["hits"], cs["fresh"], cs["uncached"], cs["evicted"]) == (held, 0, 6 - held, 0), name
            assert st["members_decoded"] == 6 - held and st["launches"] == (1 if held < 6 else 0), name
        finally:
            p.close()


def test_a_member_whose_decode_fails_loses_its_cursor(emu, container, text):
    import torch

    import orz_amd

    plain, blobs = container
    data, good, bad = text
    blob = blobs[0] + bad + blobs[3]
    src = _dev(blob)
    sb = orz_amd.MemberReader.cursor_state_bytes()
    rd = orz_amd.MemberReader(src, cache_bytes=1 << 30)
    twin = cc.CachedEmuReader(cc.emu_lib(), blob)
    twin.set_cache(1 << 30)
    try:
        base, half = len(plain[0]), len(data) // 2
        whole = torch.full((64 + half + 10 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        out, st = rd.read_ranges([(base, half), (5, 10)], out=whole[64:64 + half + 10], stats=True)
        back = _host(whole)
        assert back[64:64 + half + 10] == data[:half] + plain[0][5:15] and back[:64] == back[-64:] == b"\x5a" * 64
        e = twin.read([(base, half), (5, 10)])
        assert e.rc == 0 and {k: st[k] for k in KEYS} == {k: getattr(e, k) for k in KEYS}
        assert rd.cache_stats() == twin.cache_stats()
        assert rd.cache_stats()["bytes"] == cc.cost(len(plain[0]), sb) + cc.cost(len(data), sb)
        guard = torch.full((64 + 11 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(orz_amd.OrzError, match=r"\(member 1,"):
            rd.read_ranges([(base + len(data) - 1, 1), (0, 10)], out=guard[64:75])
        back = _host(guard)
        assert back[:64] == back[-64:] == b"\x5a" * 64
        e = twin.read([(base + len(data) - 1, 1), (0, 10)])
        assert e.rc == rc.EINVAL and "(member 1," in e.err
        cs = rd.cache_stats()
        assert cs == twin.cache_stats() and cs["cursors"] == 1 and cs["bytes"] == cc.cost(len(plain[0]), sb) and cs["resumed"] == 1
        out, st = rd.read(base, half, stats=True)  # a fresh decode
        assert _host(out) == data[:half] and half <= st["decoded_bytes"] < half + rc.SLACK
        cs = rd.cache_stats()
        assert cs["fresh"] == 1 and cs["cursors"] == 2
        assert _host(rd.read_ranges([(base + 100, 5000), (base + len(data), 1), (3, 9)])) == data[100:5100] + b"x" + plain[0][3:12]
        # switched off, the reader is what it was
        rd.set_cache(0)
        assert rd.cache_stats() == dict.fromkeys(cc.STAT_NAMES, 0)
        out, st = rd.read(0, 1000, stats=True)
        assert _host(out) == plain[0][:1000] and 1000 <= st["decoded_bytes"] < 1000 + rc.SLACK and st["host_waits"] == 3
    finally:
        rd.close()
        twin.close()


def test_members_left_in_hbm_by_the_encoder():
    """offs / lens straight from MemberEncoder.encode_to_device: four members of 1 MB, a budget for two"""
    import corpus
    import torch

    import orz_amd

    data = corpus.enwik_like(4_000_000)
    src = _dev(data)
    mb = 1_000_000
    cap = 4 * orz_amd.stream_bound(mb)
    streams = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=2)
    try:
        members = enc.encode_to_device(src.data_ptr(), len(data), streams.data_ptr(), cap, member_bytes=mb)
    finally:
        enc.close()
    assert len(members) == 4
    one = cc.cost(mb, orz_amd.MemberReader.cursor_state_bytes())
    rd = orz_amd.MemberReader(streams, members=members, cache_bytes=2 * one)
    try:
        assert rd.member_offsets == [0, mb, 2 * mb, 3 * mb]
        total = 0
        for lo in range(mb + 100_000, 2 * mb + 300_000, 200_000):  # a walk across the boundary of members 1 and 2
            out, st = rd.read(lo, 200_000, stats=True)
            assert torch.equal(out, src[lo:lo + 200_000]) and st["host_waits"] == 2
            total += st["decoded_bytes"]
        assert mb + 300_000 <= total < mb + 300_000 + rc.SLACK  # member 1 once, member 2 as far as the walk came
        assert rd.cache_stats()["cursors"] == 2 and rd.cache_stats()["bytes"] == 2 * one
        out, st = rd.read_ranges([(mb, 10), (3 * mb - 400_000, 64), (5, 5)], stats=True)  # member 0 does not fit beside the two touched
        assert torch.equal(out, torch.cat([src[mb:mb + 10], src[3 * mb - 400_000:3 * mb - 400_000 + 64], src[5:10]]))
        cs = rd.cache_stats()
        assert (cs["hits"], cs["resumed"], cs["uncached"], cs["evicted"]) == (1, 1, 1, 0) and st["members_decoded"] == 2
        out, st = rd.read(3 * mb + 17, 4096, stats=True)  # member 3 takes the place of the least recently touched: member 1
        assert torch.equal(out, src[3 * mb + 17:3 * mb + 17 + 4096])
        cs = rd.cache_stats()
        assert (cs["fresh"], cs["evicted"], cs["cursors"]) == (1, 1, 2)
        out, st = rd.read(2 * mb + 10, 100, stats=True)
        assert torch.equal(out, src[2 * mb + 10:2 * mb + 110]) and st["decoded_bytes"] == 0 and rd.cache_stats()["hits"] == 1
    finally:
        rd.close()
