"""GPU tier: byte ranges of a members container through orz_amd.MemberReader (orz_reader_*).  Bars: every read equals the Python
slice of the known input and what the emulation of the same kernels writes, from HBM and from host memory; a member is decoded
only as far as the furthest byte asked of it, so damage behind that point is not seen; three host waits a read; refusals leave
the reader usable; nothing outside the output is written."""
import pytest

import _data
import _rangecases as rc

pytestmark = pytest.mark.gpu


def _dev(data, device=0):
    import torch

    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8)[: len(data)].to("cuda:%d" % device)


def _host(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def container(oracle):
    parts = rc.parts()
    return [p for p, _ in parts], [oracle.encode(p, lv) for p, lv in parts]


def test_the_batch_from_hbm_and_from_host_memory(container, emu):
    import orz_amd

    plain, blobs = container
    data, lengths = b"".join(plain), [len(p) for p in plain]
    ranges = rc.batch(len(data))
    want = b"".join(data[o:o + ln] for o, ln in ranges)
    twin = rc.EmuReader(rc.emu_lib(), b"".join(blobs))
    try:
        e = twin.read(ranges)
        assert e.rc == 0 and e.out == want
    finally:
        twin.close()
    buf, table = rc.table_layout(blobs)
    for src, members in ((_dev(b"".join(blobs)), None), (b"".join(blobs), None), (_dev(buf), table), (bytearray(buf), table)):
        rd = orz_amd.MemberReader(src, members=members)
        try:
            assert rd.members == 7 and rd.total == len(data) and rd.member_offsets == rc.starts(lengths)
            out, st = rd.read_ranges(ranges, stats=True)
            assert _host(out) == e.out == want
            assert st["host_waits"] == 3 and st["members_decoded"] == 6 and st["launches"] == 1 and st["ranges"] == 500
            assert st["out_bytes"] == len(want) and st["kernel_ms"] > 0
            rc.check_decoded_bytes(st["decoded_bytes"], ranges, lengths)
            for name, (off, ln) in rc.named_ranges(lengths).items():
                assert _host(rd.read(off, ln)) == data[off:off + ln], name
            out, st = rd.read(0, 1000, stats=True)
            assert _host(out) == data[:1000] and 1000 <= st["decoded_bytes"] < 1000 + rc.SLACK and st["host_waits"] == 3
        finally:
            rd.close()


def test_members_left_in_hbm_by_the_encoder():
    """offs / lens straight from MemberEncoder.encode_to_device; the first member is more than one block"""
    import corpus
    import torch

    import orz_amd

    data = corpus.enwik_like(17_600_000)
    src = _dev(data)
    mb = (1 << 24) + 400_000
    cap = 2 * orz_amd.stream_bound(mb)
    streams = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    enc = orz_amd.MemberEncoder(device=0, level=1, jobs=2)
    try:
        members = enc.encode_to_device(src.data_ptr(), len(data), streams.data_ptr(), cap, member_bytes=mb)
    finally:
        enc.close()
    assert len(members) == 2
    rd = orz_amd.MemberReader(streams, members=members)
    try:
        assert rd.members == 2 and rd.total == len(data) and rd.member_offsets == [0, mb]
        # (one call: the range across the boundary makes the first member decode whole, 17 MB, once)
        ranges = [(2_999_000, 1000), (17, 70_001), (mb + 50_000, 4096), (mb, 1), (mb - 1500, 3000), (1_000_000, 16), (mb + 200_000, 333)]
        out, st = rd.read_ranges(ranges, stats=True)
        assert torch.equal(out, torch.cat([src[o:o + ln] for o, ln in ranges]))
        assert st["members_decoded"] == 2 and st["host_waits"] == 3 and st["launches"] == 1
        rc.check_decoded_bytes(st["decoded_bytes"], ranges, [mb, len(data) - mb])
        out, st = rd.read(mb + 123, 4567, stats=True)  # the second member alone: the first is not decoded
        assert torch.equal(out, src[mb + 123:mb + 123 + 4567]) and st["members_decoded"] == 1
        assert st["decoded_bytes"] < 123 + 4567 + rc.SLACK
    finally:
        rd.close()


def test_damage_behind_the_stop_and_refusals_leave_the_reader_usable(oracle, container):
    import torch

    import orz_amd

    plain, blobs = container
    data, good, bad = rc.damaged_text_member(oracle)
    blob = blobs[0] + bad + blobs[3]
    with pytest.raises(orz_amd.OrzError, match=r"member 1"):  # the precondition: the whole decode fails
        orz_amd.decode_members_to_device(_dev(blob))
    src = _dev(blob)
    rd = orz_amd.MemberReader(src)
    try:
        base, half = len(plain[0]), len(data) // 2
        out, st = rd.read(base, half, stats=True)
        assert _host(out) == data[:half] and half <= st["decoded_bytes"] < half + rc.SLACK
        with pytest.raises(orz_amd.OrzError, match=r"\(member 1,"):
            rd.read(base + len(data) - 1, 1)
        assert _host(rd.read_ranges([(base + 100, 5000), (base + len(data), 1), (3, 9)])) == data[100:5100] + b"x" + plain[0][3:12]
        total = rd.total
        for ranges in ([(total - 5, 6)], [(total + 1, 0)], [(1 << 63, 1 << 63)]):
            with pytest.raises(orz_amd.OrzError, match="invalid argument"):
                rd.read_ranges(ranges, out=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
            assert _host(rd.read(5, 7)) == plain[0][5:12]
        small = torch.full((99,), 0xA5, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(orz_amd.OrzError, match="too small"):
            rd.read(0, 100, out=small)
        assert _host(small) == b"\xa5" * 99
        with pytest.raises(orz_amd.OrzError, match="overlap"):
            rd.read(0, 16, out=src[100:200])
        assert _host(src) == blob
        out, st = rd.read_ranges([(0, 0), (total, 0)], stats=True)
        assert out.numel() == 0 and st["launches"] == 0
        assert _host(rd.read(base - 10, 20)) == plain[0][-10:] + data[:10]
    finally:
        rd.close()
    with pytest.raises(orz_amd.OrzError, match=r"\(member "):  # a framing defect fails the open
        orz_amd.MemberReader(_dev(blob[:-1]))


def test_out_with_guards_on_both_sides(container):
    import torch

    import orz_amd

    plain, blobs = container
    data = b"".join(plain)
    rd = orz_amd.MemberReader(_dev(b"".join(blobs)))
    try:
        ranges = [(100_000, 50_000), (5, 3), (len(data) - 77, 77)]
        want = b"".join(data[o:o + ln] for o, ln in ranges)
        for lead, fill in ((64, 0x5A), (61, 0x00)):  # (an output that starts at a multiple of 16, and one that does not)
            whole = torch.full((lead + len(want) + 200,), fill, dtype=torch.uint8, device="cuda:0")
            out = rd.read_ranges(ranges, out=whole[lead:lead + len(want) + 100])
            assert out.data_ptr() == whole.data_ptr() + lead and _host(out) == want
            back = _host(whole)
            assert back[:lead] == bytes([fill]) * lead and back[lead + len(want):] == bytes([fill]) * 200
    finally:
        rd.close()
