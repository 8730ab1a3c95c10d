"""GPU tier: digests through the Python face.  MemberEncoder's digests=True against zlib, the verified decode
(orz_decode_tensors_verified) of the three layouts inside a poisoned arena -- its host waits against the unverified call's --, the
two kinds of damage no decoder reports (a member table whose entries are mixed up, a payload bit that flips in the library's own
stream), damage the decoder does report, refusals with nothing written, and MemberReader.read_tensor(digest=...)."""
import zlib

import pytest

import _crccases as cc
import _piececases as pp
import _planecases as pc

pytestmark = pytest.mark.gpu

POISON = pc.POISON


@pytest.fixture(scope="module")
def enc():
    import orz_amd
    import torch

    torch.cuda.init()  # (torch opens the device before the library does, as in the other GPU tests)
    e = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    yield e
    e.close()


def _typed(torch, data, e):
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e]
    if not data:
        return torch.empty(0, dtype=dt, device="cuda:0")
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0").view(dt)


def _host(t):
    import torch

    return bytes(t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy())


def _fresh(torch, ts, room=0):
    """(a poisoned arena, the destinations in it at multiples of their element size in reverse order, their offsets)"""
    caps = [len(d) + room * e for d, e in ts]
    offs, total = pc.layout(caps, [e % 16 for _, e in ts], reverse=True)
    arena = torch.full((total,), POISON, dtype=torch.uint8, device="cuda:0")
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    return arena, [arena[o:o + c].view(dt[e]) for o, c, (_, e) in zip(offs, caps, ts)], offs


def _expect(ts, offs, total, swap=None):
    return pc.expect_arena(total, [(o, (swap or {}).get(j, d)) for j, ((d, _), o) in enumerate(zip(ts, offs))])


def _encode(enc, torch, ts, which):
    """(container, members, the keyword arguments of the decode, the decode function, the digests) of a layout"""
    import orz_amd

    tensors = [_typed(torch, d, e) for d, e in ts]
    if which == "whole":
        container, members, crcs = enc.encode_tensors(tensors, digests=True)
        return container, members, {}, orz_amd.decode_members_into, crcs
    if which == "planes":
        container, members, elems, crcs = enc.encode_tensor_planes(tensors, digests=True)
        return container, members, {"elems": elems}, orz_amd.decode_planes_into, crcs
    container, members, elems, pieces, crcs = enc.encode_tensor_pieces(tensors, cc.PIECE, digests=True)
    return container, members, {"elems": elems, "pieces": pieces}, orz_amd.decode_planes_into, crcs


def _tensors(which):
    return pc.mixed_tensors(counts=cc.COUNTS) if which != "pieces" else pp.tensors(cc.PIECE, seed=1) + pc.mixed_tensors(counts=(17,))


# ------------------------------------------------------------------------------------------------ round trips
@pytest.mark.parametrize("which", ["whole", "planes", "pieces"])
def test_digests_round_trip(enc, which):
    import torch

    ts = _tensors(which)
    container, members, kw, decode, crcs = _encode(enc, torch, ts, which)
    assert crcs == cc.crcs_of(ts)  # the digests of the INPUT, zlib's
    assert [len(enc.encode_tensors([], digests=g)) for g in (False, True)] == [2, 3]
    assert [len(enc.encode_tensor_planes([], digests=g)) for g in (False, True)] == [3, 4]
    assert [len(enc.encode_tensor_pieces([], 32, digests=g)) for g in (False, True)] == [4, 5]
    arena, outs, offs = _fresh(torch, ts)
    sizes, st = decode(container, outs, device=0, members=members, stats=True, digests=crcs, **kw)
    assert sizes == [len(d) for d, _ in ts]
    pc.same(bytes(arena.cpu().numpy()), _expect(ts, offs, arena.numel()), "the arena of destinations")
    arena2, outs2, _ = _fresh(torch, ts)
    sizes2, plain = decode(container, outs2, device=0, members=members, stats=True, **kw)
    assert sizes2 == sizes and bytes(arena2.cpu().numpy()) == bytes(arena.cpu().numpy())
    assert st["host_waits"] == plain["host_waits"] + 1 == 6 and st["launches"] == plain["launches"] == 1
    # the digests of CPU tensors are the same digests
    assert enc.encode_tensors([t.cpu() for t in outs[:4]], digests=True)[2] == crcs[:4]


def test_a_wrong_digest_for_the_last_of_many_names_it(enc):
    import orz_amd
    import torch

    ts = _tensors("planes")
    container, members, kw, decode, crcs = _encode(enc, torch, ts, "planes")
    last = max(j for j, (d, _) in enumerate(ts) if d)
    for j in (last, len(ts) - 1):
        given = list(crcs)
        given[j] ^= 0x80000000
        arena, outs, offs = _fresh(torch, ts)
        with pytest.raises(orz_amd.OrzDigestError) as info:
            decode(container, outs, device=0, members=members, digests=given, **kw)
        e = info.value
        assert (e.tensor, e.expected, e.computed) == (j, given[j], crcs[j])
        assert "(-74)" in str(e) and "destination %d " % j in str(e) and "0x%08x" % crcs[j] in str(e)
        pc.same(bytes(arena.cpu().numpy()), _expect(ts, offs, arena.numel()), "the arena: the tensors keep what was decoded")


# ------------------------------------------------------------------------------------------------ silent damage
def test_a_mixed_up_table_is_silent_without_digests(enc):
    import orz_amd
    import torch

    ts = pc.mixed_tensors(counts=(1, 17))
    container, members, kw, decode, crcs = _encode(enc, torch, ts, "planes")
    planes = pc.planes_of(ts)
    first = pp.first_members(ts, [1] * len(ts))
    a = next(j for j, (d, e) in enumerate(ts) if e == 2 and len(d) == 34)
    b = next(j for j, (d, e) in enumerate(ts) if e == 4 and len(d) == 68)
    ma, mb = first[a], first[b] + 1
    mixed = list(members)
    mixed[ma], mixed[mb] = members[mb], members[ma]
    wrong = list(planes)
    wrong[ma], wrong[mb] = planes[mb], planes[ma]
    got = {j: pc.np_merge(wrong[first[j]:first[j] + ts[j][1]]) for j in (a, b)}
    arena, outs, offs = _fresh(torch, ts)
    decode(container, outs, device=0, members=mixed, **kw)  # the gap: no error, two wrong tensors
    pc.same(bytes(arena.cpu().numpy()), _expect(ts, offs, arena.numel(), swap=got), "the arena of the mixed-up decode")
    arena, outs, offs = _fresh(torch, ts)
    with pytest.raises(orz_amd.OrzDigestError) as info:
        decode(container, outs, device=0, members=mixed, digests=crcs, **kw)
    low = min(a, b)
    assert (info.value.tensor, info.value.expected, info.value.computed) == (low, crcs[low], zlib.crc32(got[low]))


def _flipped(torch, container, bit):
    host = bytearray(container.cpu().numpy().tobytes())
    host[bit // 8] ^= 1 << (bit % 8)
    return torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")


def test_a_silent_flip_in_the_librarys_own_stream_is_caught(enc):
    import orz_amd
    import torch

    head, weights = pc.tensor_bytes(1, 33, 4), cc.bf16_weights()
    ts = [(head, 1), (weights, 2)]
    container, members, kw, decode, crcs = _encode(enc, torch, ts, "planes")
    at, length = members[1]  # the low plane's stream
    for k in range(32):
        bad = _flipped(torch, container, 8 * at + 8 * length // 2 + 7 * k)
        arena, outs, offs = _fresh(torch, ts)
        try:
            decode(bad, outs, device=0, members=members, **kw)
        except orz_amd.OrzError:
            continue
        if _host(outs[1]) != weights:
            break
    else:
        raise AssertionError("no silent flip within 32 tries: the set-up broke")
    print("silent flip at try", k)
    silent = bytes(arena.cpu().numpy())
    arena, outs, offs = _fresh(torch, ts)
    with pytest.raises(orz_amd.OrzDigestError) as info:
        decode(bad, outs, device=0, members=members, digests=crcs, **kw)
    assert info.value.tensor == 1 and info.value.expected == crcs[1] == zlib.crc32(weights)
    assert info.value.computed == zlib.crc32(_host(outs[1])) != crcs[1]
    assert bytes(arena.cpu().numpy()) == silent


def test_damage_the_decoder_sees_is_reported_as_the_member(enc):
    import orz_amd
    import torch

    head, weights = pc.tensor_bytes(1, 33, 4), cc.bf16_weights()
    ts = [(head, 1), (weights, 2)]
    container, members, kw, decode, crcs = _encode(enc, torch, ts, "planes")
    at, length = members[2]  # the high plane's stream
    for k in range(64):
        bad = _flipped(torch, container, 8 * at + 8 * length // 2 + 7 * k)
        arena, outs, offs = _fresh(torch, ts)
        try:
            decode(bad, outs, device=0, members=members, digests=crcs, **kw)
        except orz_amd.OrzDigestError:
            continue
        except orz_amd.OrzError as e:
            if "status" in str(e):
                assert "(-22)" in str(e) and "member 2," in str(e)
                return
    raise AssertionError("no flip within 64 tries fails the decode: the set-up broke")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(enc):
    import orz_amd
    import torch

    ts = pc.mixed_tensors(counts=(17,))
    container, members, kw, decode, crcs = _encode(enc, torch, ts, "planes")

    def refused(outs, pattern, **more):
        with pytest.raises(orz_amd.OrzError, match=pattern) as info:
            decode(container, outs, device=0, members=members, digests=crcs, **dict(kw, **more))
        assert not isinstance(info.value, orz_amd.OrzDigestError)
        assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()

    arena, outs, offs = _fresh(torch, ts)
    short = list(outs)
    short[1] = outs[1][:-1]
    refused(short, r"\(-12\).*destination 1 ")
    over = list(outs)
    over[2] = arena[offs[1] + 2:offs[1] + 2 + len(ts[2][0])].view(outs[2].dtype)
    refused(over, r"\(-22\).*overlap")
    refused(outs, r"\(-22\).*planes for", elems=[1] * len(ts))
    with pytest.raises(ValueError):
        decode(container, outs, device=0, members=members, digests=crcs[:-1], **kw)
    with pytest.raises(ValueError):
        decode(container, outs, device=0, members=members, digests=[-1] + crcs[1:], **kw)
    assert bytes(arena.cpu().numpy()) == bytes([POISON]) * arena.numel()


# ------------------------------------------------------------------------------------------------ the reader
def test_read_tensor_holds_a_whole_tensor_to_its_digest(enc):
    import orz_amd
    import torch

    ts = pp.tensors(cc.PIECE, seed=2)
    container, members, kw, _, crcs = _encode(enc, torch, ts, "pieces")
    rd = orz_amd.MemberReader(container, device=0, members=members, **kw)
    try:
        for j, (d, e) in enumerate(ts):
            assert _host(rd.read_tensor(j, digest=crcs[j])) == d
            assert _host(rd.read_tensor(j, 0, len(d) // e, digest=crcs[j])) == d
        j = max(range(len(ts)), key=lambda k: len(ts[k][0]))
        d, e = ts[j]
        out = torch.zeros(len(d) // e, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e], device="cuda:0")
        assert _host(rd.read_tensor(j, out=out, digest=crcs[j])) == d
        with pytest.raises(orz_amd.OrzDigestError) as info:
            rd.read_tensor(j, digest=crcs[j] ^ 1)
        assert (info.value.tensor, info.value.expected, info.value.computed) == (j, crcs[j] ^ 1, crcs[j])
        for first, count in ((1, None), (0, len(d) // e - 1), (1, len(d) // e - 1)):
            with pytest.raises(ValueError, match="partial read"):
                rd.read_tensor(j, first, count, digest=crcs[j])
        assert _host(rd.read_tensor(j, 1, 5)) == d[e:6 * e]  # (unverified partial reads do what they did)
    finally:
        rd.close()
