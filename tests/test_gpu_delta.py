"""GPU tier: the delta layout (orz_members_encode_deltas_to_device, orz_decode_tensors_delta) through the Python face.  Bars: every
member of encode_tensor_deltas is byte for byte the member encode_tensor_pieces of the same kind of encoder writes for the tensors
XORed in torch; the decode restores the tensors out of place and in place inside a poisoned arena and equals the plain decode
followed by a torch XOR; digests vouch for the restored tensors, so a wrong base is a digest error; sizes, messages and host waits
agree with the emulation twin (tests/emu/emu_delta.cpp); and the bf16 step of the issue comes to less than half its plain planes.
A few dozen members of a few KB at most, but for the size bar."""
import pytest

import _crccases as cc
import _deltacases as dc
import _planecases as pc

pytestmark = pytest.mark.gpu

POISON = pc.POISON
PIECE = 512  # 16 x 32: the tensors of 1029 elements are three pieces a plane
# (element size, elements, with a base): every element size with a base, single bytes and int64 without one too, an empty tensor; 44 members at PIECE
SHAPES = ((2, 1029, True), (1, 1029, True), (4, 17, True), (8, 33, False), (1, 16, False), (2, 0, False), (4, 1029, True), (8, 15, True))
DT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _members(P):
    return sum(e * (-(-c // P) if P and P < c else 1) for e, c, _ in SHAPES)


def _case():
    ts = [(pc.tensor_bytes(e, c, 11 + k), e) for k, (e, c, _) in enumerate(SHAPES)]
    bases = [pc.tensor_bytes(e, c, 90 + k) if has else None for k, (e, c, has) in enumerate(SHAPES)]
    return ts, bases


def _typed(torch, data, e, device="cuda:0"):
    dt = getattr(torch, DT[e])
    if not data:
        return torch.empty(0, dtype=dt, device=device)
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device).view(dt)


def _host(t):
    import torch

    return bytes(t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy())


def _streams(container, members):
    host = _host(container)
    return [host[o:o + ln] for o, ln in members]


@pytest.fixture(scope="module")
def encoders():
    import orz_amd
    import torch

    torch.cuda.init()  # (torch opens the device before the library does, as in the other GPU tests)
    made = {jobs: orz_amd.MemberEncoder(device=0, level=1, jobs=jobs) for jobs in (1, 3)}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def enc(encoders):
    return encoders[3]


@pytest.fixture(scope="module")
def packed(enc):
    """(tensors as bytes, bases as bytes, tensors and bases on the device, container, members, elems, pieces, digests) at PIECE"""
    import torch

    ts, bases = _case()
    tensors = [_typed(torch, d, e) for d, e in ts]
    d_bases = [_typed(torch, b, e) if b is not None else None for b, (_, e) in zip(bases, ts)]
    container, members, elems, pieces, crcs = enc.encode_tensor_deltas(tensors, d_bases, PIECE, digests=True)
    assert len(members) == _members(PIECE) == 44 and crcs == cc.crcs_of(ts)  # the digests of the INPUT tensors, zlib's
    return ts, bases, tensors, d_bases, container, members, elems, pieces, crcs


# ------------------------------------------------------------------------------------------------ streams
@pytest.mark.parametrize("where", ["cuda:0", "cpu"])
@pytest.mark.parametrize("P", [0, PIECE])
@pytest.mark.parametrize("jobs", [1, 3])
def test_every_member_is_the_pieces_member_of_the_xored_tensor(encoders, jobs, P, where):
    import torch

    e = encoders[jobs]
    ts, bases = _case()
    tensors = [_typed(torch, d, el, where) for d, el in ts]
    d_bases = [_typed(torch, b, el, where) if b is not None else None for b, (_, el) in zip(bases, ts)]
    before = [_host(t) for t in tensors], [_host(b) for b in d_bases if b is not None]
    container, members, elems, pieces = e.encode_tensor_deltas(tensors, d_bases, P)
    assert ([_host(t) for t in tensors], [_host(b) for b in d_bases if b is not None]) == before  # neither is written
    xored = [t ^ b if b is not None else t for t, b in zip(tensors, d_bases)]
    assert [_host(x) for x in xored] == [d for d, _ in dc.deltas(ts, bases)]
    c2, m2, e2, q2 = e.encode_tensor_pieces(xored, P)
    assert (elems, pieces) == (e2, q2) and len(members) == len(m2) == _members(P)
    for k, (a, b) in enumerate(zip(_streams(container, members), _streams(c2, m2))):
        assert a == b, "member %d differs from the member of the tensor XORed in torch" % k
    # with no base anywhere: the pieces call's whole result
    nobase = e.encode_tensor_deltas(tensors, [None] * len(tensors), P)
    plain = e.encode_tensor_pieces(tensors, P)
    assert nobase[2:] == plain[2:] and [ln for _, ln in nobase[1]] == [ln for _, ln in plain[1]]
    assert _streams(nobase[0], nobase[1]) == _streams(plain[0], plain[1])
    if jobs == 1:  # (one worker fills the container front to back: the same places too)
        assert nobase[1] == plain[1] and _host(nobase[0]) == _host(plain[0])


def test_no_tensors(enc):
    assert [len(enc.encode_tensor_deltas([], [], digests=g)) for g in (False, True)] == [4, 5]
    assert enc.encode_tensor_deltas([], [], 32)[1:] == ([], [], [])
    assert enc.encode_deltas_to_device([], [], [], [], 32, 0, 0) == ([], [])


# ------------------------------------------------------------------------------------------------ round trip
def _arena(torch, ts, bases, in_place=False, rem="e"):
    """(a poisoned arena, the destinations in it in reverse order, the bases in it behind them -- or the destinations themselves,
    holding their bases --, the offsets of both, what the arena holds before the call).  Everything lies at `rem` modulo 16: "e",
    the element size -- every unit goes byte by byte --, or 0 -- full units move as 16-byte accesses."""
    caps = [len(d) for d, _ in ts]
    if in_place:
        offs, total = pc.layout(caps, dc.rems_for(ts, rem), reverse=True)
        base_offs = [o if b is not None else None for o, b in zip(offs, bases)]
    else:
        offs, _, base_offs, total, _ = dc.places(ts, bases, room=0, rem=rem)
    before = pc.expect_arena(total, [(o, b) for o, b in zip(base_offs, bases) if b is not None])
    arena = torch.frombuffer(bytearray(before), dtype=torch.uint8).to("cuda:0")
    assert arena.data_ptr() % 16 == 0
    view = lambda o, n, e: arena[o:o + n].view(getattr(torch, DT[e]))  # noqa: E731
    outs = [view(o, c, e) for o, c, (_, e) in zip(offs, caps, ts)]
    d_bases = [None if b is None else (out if in_place else view(bo, len(b), e)) for b, bo, out, (_, e) in zip(bases, base_offs, outs, ts)]
    return arena, outs, d_bases, offs, base_offs, before


def _twin(packed_, spots, base_offs, total, before_pieces, crcs, on_device=True):
    """the same call on the emulation twin, over the library's own container"""
    ts, bases, _, _, container, members, elems, pieces, _ = packed_
    return dc.decode_delta(dc.emu_lib(), _host(container), members, spots, base_offs, elems, pieces, crcs, total, prefill=before_pieces)


@pytest.mark.parametrize("rem", [0, "e"])
@pytest.mark.parametrize("in_place", [False, True])
def test_round_trip(packed, in_place, rem):
    import orz_amd
    import torch

    ts, bases, tensors, _, container, members, elems, pieces, crcs = packed
    arena, outs, d_bases, offs, base_offs, before = _arena(torch, ts, bases, in_place, rem)
    sizes, st = orz_amd.decode_planes_into(container, outs, device=0, members=members, elems=elems, pieces=pieces, bases=d_bases, stats=True)
    assert sizes == [len(d) for d, _ in ts]
    kept = [] if in_place else [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    # the tensors in their places, bases given out of place as they were, poison everywhere else
    pc.same(_host(arena), pc.expect_arena(arena.numel(), kept + [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations and bases")
    # the pieces call on the same container: the deltas, in the same host waits; XORed in torch they are the tensors
    a2, outs2, b2, _, _, _ = _arena(torch, ts, bases, False, rem)
    sizes2, plain = orz_amd.decode_planes_into(container, outs2, device=0, members=members, elems=elems, pieces=pieces, stats=True)
    assert sizes2 == sizes and st["host_waits"] == plain["host_waits"] == 5 and st["launches"] == plain["launches"] == 1
    assert [_host(o ^ b if b is not None else o) for o, b in zip(outs2, b2)] == [_host(o) for o in outs] == [d for d, _ in ts]
    # the emulation twin: the same bytes, sizes and host waits
    prefill = [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    twin = _twin(packed, [(o, len(d)) for o, (d, _) in zip(offs, ts)], base_offs, arena.numel(), prefill, None)
    assert twin.rc == 0, twin.err
    assert twin.arena == _host(arena) and twin.out_lens == sizes and twin.host_waits == st["host_waits"]


def test_without_pieces_and_from_a_host_container(enc, packed):
    import orz_amd
    import torch

    ts, bases, tensors, d_bases, _, _, _, _, _ = packed
    container, members, elems, pieces = enc.encode_tensor_deltas(tensors, d_bases)
    assert pieces == [1] * len(ts)
    host = b"".join(_streams(container, members))
    arena, outs, bs, offs, base_offs, _ = _arena(torch, ts, bases)
    sizes, st = orz_amd.decode_planes_into(host, outs, device=0, elems=elems, bases=bs, stats=True)  # (no `pieces`, no table)
    assert sizes == [len(d) for d, _ in ts] and [_host(o) for o in outs] == [d for d, _ in ts] and st["host_waits"] == 5


# ------------------------------------------------------------------------------------------------ digests
@pytest.mark.parametrize("in_place", [False, True])
def test_digests_vouch_for_the_restored_tensors(packed, in_place):
    import orz_amd
    import torch

    ts, bases, _, _, container, members, elems, pieces, crcs = packed
    kw = dict(device=0, members=members, elems=elems, pieces=pieces)
    arena, outs, d_bases, offs, base_offs, _ = _arena(torch, ts, bases, in_place)
    sizes, st = orz_amd.decode_planes_into(container, outs, bases=d_bases, digests=crcs, stats=True, **kw)
    assert [_host(o) for o in outs] == [d for d, _ in ts] and st["host_waits"] == 6
    # ONE flipped bit in ONE base: the digest error names its tensor
    j = max(k for k, b in enumerate(bases) if b is not None and len(b) > 1000)
    arena, outs, d_bases, offs, base_offs, _ = _arena(torch, ts, bases, in_place)
    arena[base_offs[j] + len(bases[j]) // 2] ^= 0x10
    wrong = _host(arena)
    with pytest.raises(orz_amd.OrzDigestError) as info:
        orz_amd.decode_planes_into(container, outs, bases=d_bases, digests=crcs, **kw)
    e = info.value
    assert e.tensor == j and e.expected == crcs[j] and e.computed != crcs[j]
    assert "orz_decode_tensors_delta failed (-74)" in str(e) and "destination %d " % j in str(e)
    prefill = [(o, wrong[o:o + len(b)]) for o, b in zip(base_offs, bases) if b is not None]
    twin = _twin(packed, [(o, len(d)) for o, (d, _) in zip(offs, ts)], base_offs, arena.numel(), prefill, crcs)
    assert twin.rc == dc.EBADMSG and twin.err == str(e).split("): ", 1)[1] and twin.arena == _host(arena)
    if not in_place:  # a base given out of place is untouched
        assert all(_host(arena)[o:o + len(b)] == wrong[o:o + len(b)] for o, b in zip(base_offs, bases) if b is not None)


def test_a_flipped_payload_bit_is_reported_as_today(packed):
    """the same damaged container through the delta call and through the verified call that knows no bases (held to the digests of
    the DELTAS): the same kind of error for the same member or tensor"""
    import orz_amd
    import torch

    ts, bases, _, _, container, members, elems, pieces, crcs = packed
    kw = dict(device=0, members=members, elems=elems, pieces=pieces)
    delta_crcs = cc.crcs_of(dc.deltas(ts, bases))
    at, length = max(members, key=lambda m: m[1])
    kinds = set()
    for k in range(6):
        host = bytearray(_host(container))
        bit = 8 * at + 8 * length // 2 + 7 * k
        host[bit // 8] ^= 1 << (bit % 8)
        bad = torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")
        got = []
        for bs, digests in ((True, crcs), (False, delta_crcs)):
            arena, outs, d_bases, _, _, _ = _arena(torch, ts, bases)
            with pytest.raises(orz_amd.OrzError) as info:
                orz_amd.decode_planes_into(bad, outs, digests=digests, **dict(kw, **({"bases": d_bases} if bs else {})))
            err = info.value
            got.append(("digest", err.tensor) if isinstance(err, orz_amd.OrzDigestError) else ("member", str(err).split("): ", 1)[1]))
        assert got[0] == got[1], (k, got)
        kinds.add(got[0][0])
    print("kinds of error over six flips:", sorted(kinds))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing_and_read_like_the_twins(packed):
    import orz_amd
    import torch

    ts, bases, _, _, container, members, elems, pieces, crcs = packed
    kw = dict(device=0, members=members, elems=elems, pieces=pieces, digests=crcs)
    arena, outs, d_bases, offs, base_offs, before = _arena(torch, ts, bases)
    prefill = [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    u8 = lambda o, n, e: arena[o:o + n].view(getattr(torch, DT[e]))  # noqa: E731

    def refused(bs, twin_offs, pattern):
        with pytest.raises(orz_amd.OrzError) as info:
            orz_amd.decode_planes_into(container, outs, bases=bs, **kw)
        text = str(info.value)
        assert "orz_decode_tensors_delta failed (-22): " in text and pattern in text and not isinstance(info.value, orz_amd.OrzDigestError)
        assert _host(arena) == before
        twin = _twin(packed, [(o, len(d)) for o, (d, _) in zip(offs, ts)], twin_offs, arena.numel(), prefill, crcs)
        assert twin.rc == dc.EINVAL and twin.err == text.split("): ", 1)[1] and twin.arena == before

    n0 = len(ts[0][0])
    # a base that overlaps its own destination at another address (two bytes in: the same element size and count, another place)
    bs, bo = list(d_bases), list(base_offs)
    bs[0], bo[0] = u8(offs[0] + 2, n0, 2), offs[0] + 2
    refused(bs, bo, "the base of destination 0 overlaps destination 0 at another address")
    # one that overlaps another destination
    j = 6  # (int32, 1029 elements: larger than destination 0)
    bs, bo = list(d_bases), list(base_offs)
    at = offs[0] + 6 - 4 * 1029  # (destination 0 lies at 2 modulo 16: a multiple of 4, and the base's last 6 bytes are its first)
    bs[j], bo[j] = u8(at, 4 * 1029, 4), at
    refused(bs, bo, "the base of destination 6 overlaps destination 0")
    # what the Python face refuses itself, as ValueErrors
    with pytest.raises(ValueError, match="one base"):
        orz_amd.decode_planes_into(container, outs, bases=d_bases[:-1], **kw)
    with pytest.raises(ValueError, match="base 0 has"):
        orz_amd.decode_planes_into(container, outs, bases=[outs[0][:-1]] + d_bases[1:], **kw)
    with pytest.raises(ValueError, match="base 0 lies on cpu"):
        orz_amd.decode_planes_into(container, outs, bases=[d_bases[0].cpu()] + d_bases[1:], **kw)
    assert _host(arena) == before


# ------------------------------------------------------------------------------------------------ size
def test_the_bf16_step_is_below_half_its_plain_planes(enc):
    """the issue's bar: w and its lr 1e-4 successor, 2^19 bf16 elements -- the oracle gives 0.43, the fast parse stays within half a
    percent of the reference's sizes, 0.5 is a condition with room to spare"""
    import orz_amd
    import torch

    w, tuned = dc.bf16_step()
    t = torch.frombuffer(bytearray(tuned), dtype=torch.uint8).to("cuda:0").view(torch.bfloat16)
    b = torch.frombuffer(bytearray(w), dtype=torch.uint8).to("cuda:0").view(torch.bfloat16)
    plain, mp, _ = enc.encode_tensor_planes([t])
    delta, md, elems, pieces, crcs = enc.encode_tensor_deltas([t], [b], digests=True)
    size = lambda m: sum(ln for _, ln in m)  # noqa: E731
    print("plain planes %d, delta %d: %.3f" % (size(mp), size(md), size(md) / size(mp)))
    assert size(md) < 0.5 * size(mp)
    out = b.clone()  # restored in place
    orz_amd.decode_planes_into(delta, [out], device=0, members=md, elems=elems, pieces=pieces, bases=[out], digests=crcs)
    assert _host(out) == tuned
