"""GPU tier: chains of delta links (orz_decode_tensors_chain) through the Python face.  The links are what encode_tensor_deltas
writes on the GPU for the steps of a run, joined with join_links.  Bars: the chain call restores the last step out of place and in
place inside a poisoned arena, equals K sequential decode_planes_into(bases=) calls, works without pieces and from a host
container; digests vouch for the final tensors, so a wrong base and a mixed-up member table are digest errors; refusals write
nothing; bytes, sizes, host waits, members and messages agree with the emulation twin (tests/emu/emu_chain.cpp) on the same
containers; links=1 is the call without links; and PlaneMergeChain alone, through the measuring hook, against numpy.  A few dozen
members of a few KB at most."""
import ctypes

import numpy as np
import pytest

import _chaincases as ch
import _crccases as cc
import _deltacases as dc
import _planecases as pc

pytestmark = pytest.mark.gpu

K = 3
PIECE = 512
# (element size, elements, whether the reader holds step 0 of it: without, link 0 holds the tensor itself -- a keyframe)
SHAPES = ((2, 4101, True), (1, 1029, True), (4, 1029, True), (8, 33, False), (2, 0, False), (1, 16, False), (8, 1029, True))
DT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}
J = len(SHAPES)


def _pieces(P):
    return [(-(-c // P) if P and P < c else 1) for _, c, _ in SHAPES]


def _typed(torch, data, e, device="cuda:0"):
    dt = getattr(torch, DT[e])
    if not data:
        return torch.empty(0, dtype=dt, device=device)
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device).view(dt)


def _host(t):
    import torch

    return bytes(t.contiguous().view(torch.uint8).reshape(-1).cpu().numpy())


@pytest.fixture(scope="module")
def enc():
    import orz_amd
    import torch

    torch.cuda.init()  # (torch opens the device before the library does, as in the other GPU tests)
    e = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    yield e
    e.close()


def _steps():
    """[[(bytes, element size)] per step], K + 1 steps of random bytes: a byte routed to the wrong link or place shows"""
    return [[(pc.tensor_bytes(e, c, 11 + 20 * s + k), e) for k, (e, c, _) in enumerate(SHAPES)] for s in range(K + 1)]


def _encode(enc, P):
    """the K links at a piece size of P, each encoded on the GPU against the step before: (steps, bases as bytes or None, [(container,
    members)], elems, pieces, the digests of the last step)"""
    import torch

    sts = _steps()
    dev = [[_typed(torch, d, e) for d, e in st] for st in sts]
    links, crcs = [], None
    for k in range(K):
        bases = [b if has or k else None for b, (_, _, has) in zip(dev[k], SHAPES)]
        container, members, elems, pieces, crcs = enc.encode_tensor_deltas(dev[k + 1], bases, P, digests=True)
        assert pieces == _pieces(P) and len(members) == sum(e * q for (e, _, _), q in zip(SHAPES, pieces))
        links.append((container, members))
    assert crcs == cc.crcs_of(sts[K])
    bases = [d if has else None for (d, _), (_, _, has) in zip(sts[0], SHAPES)]
    return sts, bases, links, elems, pieces, crcs


@pytest.fixture(scope="module")
def packed(enc):
    import orz_amd

    sts, bases, links, elems, pieces, crcs = _encode(enc, PIECE)
    container, members = orz_amd.join_links(links)
    assert container.is_cuda and len(members) == K * len(links[0][1])
    return sts, bases, links, container, members, elems, pieces, crcs


def _arena(torch, ts, bases, in_place=False, rem="e"):
    """test_gpu_delta's arena: the destinations in reverse order, the bases behind them or in them, everything at `rem` modulo 16"""
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


def _twin(container, members, elems, pieces, ts, offs, base_offs, total, prefill, crcs, links=K):
    """the same call on the emulation twin, over the library's own container"""
    host = container if isinstance(container, bytes) else _host(container)
    return ch.decode_chain(ch.emu_lib(), host, members, [(o, len(d)) for o, (d, _) in zip(offs, ts)], base_offs, elems, pieces, crcs, total, links,
                           prefill=prefill)


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("rem", [0, "e"])
@pytest.mark.parametrize("in_place", [False, True])
def test_round_trip(packed, in_place, rem):
    import orz_amd
    import torch

    sts, bases, links, container, members, elems, pieces, crcs = packed
    ts = sts[K]
    arena, outs, d_bases, offs, base_offs, before = _arena(torch, ts, bases, in_place, rem)
    sizes, st = orz_amd.decode_planes_into(container, outs, device=0, members=members, elems=elems, pieces=pieces, bases=d_bases, links=K, stats=True)
    assert sizes == [len(d) for d, _ in ts] and st["members"] == len(members)
    kept = [] if in_place else [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    # the last step in its places, bases given out of place as they were, poison everywhere else
    pc.same(_host(arena), pc.expect_arena(arena.numel(), kept + [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations and bases")
    # K sequential calls, a link each, in place: the same bytes, K times the host waits
    a2, outs2, b2, _, _, _ = _arena(torch, ts, bases, True, rem)
    waits = 0
    for k, (c, m) in enumerate(links):
        bs = [o if b is not None or k else None for o, b in zip(outs2, bases)]
        sizes2, s2 = orz_amd.decode_planes_into(c, outs2, device=0, members=m, elems=elems, pieces=pieces, bases=bs, stats=True)
        assert sizes2 == sizes
        waits += s2["host_waits"]
    assert [_host(o) for o in outs2] == [_host(o) for o in outs] == [d for d, _ in ts]
    assert st["host_waits"] == 5 and waits == K * 5
    # the emulation twin: the same bytes, sizes, members and host waits
    prefill = [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    twin = _twin(container, members, elems, pieces, ts, offs, base_offs, arena.numel(), prefill, None)
    assert twin.rc == 0, twin.err
    assert twin.arena == _host(arena) and twin.out_lens == sizes and twin.host_waits == st["host_waits"] and twin.members == st["members"]


def test_without_pieces_and_from_a_host_container(enc):
    import orz_amd
    import torch

    sts, bases, links, elems, pieces, crcs = _encode(enc, 0)
    assert pieces == [1] * J
    host_links = [(_host(c), m) for c, m in links]
    container, members = orz_amd.join_links(host_links)
    assert isinstance(container, bytes)
    ts = sts[K]
    arena, outs, bs, offs, base_offs, _ = _arena(torch, ts, bases)
    sizes, st = orz_amd.decode_planes_into(container, outs, device=0, members=members, elems=elems, bases=bs, links=K, stats=True)  # (no `pieces`)
    assert sizes == [len(d) for d, _ in ts] and [_host(o) for o in outs] == [d for d, _ in ts] and st["host_waits"] == 6
    # no table either: the links' members one behind the other, found from the framing
    flat = b"".join(c[o:o + ln] for c, m in host_links for o, ln in m)
    arena, outs, bs, offs, base_offs, _ = _arena(torch, ts, bases)
    sizes, st = orz_amd.decode_planes_into(flat, outs, device=0, elems=elems, bases=bs, links=K, digests=crcs, stats=True)
    assert [_host(o) for o in outs] == [d for d, _ in ts] and st["host_waits"] == 6
    # without bases: the XOR of the links, which is the last step where link 0 is a keyframe
    arena, outs, _, offs, _, _ = _arena(torch, ts, [None] * J)
    orz_amd.decode_planes_into(flat, outs, device=0, elems=elems, links=K)
    want = [d if b is None else dc.xor(d, b) for (d, _), b in zip(ts, bases)]
    assert [_host(o) for o in outs] == want
    twin = _twin(flat, None, elems, None, ts, offs, None, arena.numel(), [], None)
    assert twin.rc == 0 and twin.arena == _host(arena), twin.err


# ------------------------------------------------------------------------------------------------ digests
@pytest.mark.parametrize("in_place", [False, True])
def test_digests_vouch_for_the_final_tensors(packed, in_place):
    import orz_amd
    import torch

    sts, bases, links, container, members, elems, pieces, crcs = packed
    ts = sts[K]
    kw = dict(device=0, members=members, elems=elems, pieces=pieces, links=K)
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
    assert "orz_decode_tensors_chain failed (-74)" in str(e) and "destination %d " % j in str(e)
    prefill = [(o, wrong[o:o + len(b)]) for o, b in zip(base_offs, bases) if b is not None]
    twin = _twin(container, members, elems, pieces, ts, offs, base_offs, arena.numel(), prefill, crcs)
    assert twin.rc == ch.EBADMSG and twin.err == str(e).split("): ", 1)[1] and twin.arena == _host(arena)
    if not in_place:  # a base given out of place is untouched
        assert all(_host(arena)[o:o + len(b)] == wrong[o:o + len(b)] for o, b in zip(base_offs, bases) if b is not None)


def test_exchanged_table_entries_are_silent_without_digests_and_a_digest_error_with_them(packed):
    import orz_amd
    import torch

    sts, bases, links, container, members, elems, pieces, crcs = packed
    ts = sts[K]
    M1 = len(links[0][1])
    q = pieces[0]  # tensor 0 in link 1: the first piece of plane 0 and the first of plane 1 -- the same size, other bytes
    mixed = list(members)
    mixed[M1], mixed[M1 + q] = members[M1 + q], members[M1]
    kw = dict(device=0, members=mixed, elems=elems, pieces=pieces, links=K)
    arena, outs, d_bases, offs, base_offs, _ = _arena(torch, ts, bases)
    orz_amd.decode_planes_into(container, outs, bases=d_bases, **kw)
    assert _host(outs[0]) != ts[0][0] and [_host(o) for o in outs[1:]] == [d for d, _ in ts[1:]]
    silent = _host(arena)
    arena, outs, d_bases, offs, base_offs, _ = _arena(torch, ts, bases)
    with pytest.raises(orz_amd.OrzDigestError) as info:
        orz_amd.decode_planes_into(container, outs, bases=d_bases, digests=crcs, **kw)
    assert info.value.tensor == 0 and "destination 0 " in str(info.value) and _host(arena) == silent


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing_and_read_like_the_twins(enc, packed):
    import orz_amd
    import torch

    sts, bases, links, container, members, elems, pieces, crcs = packed
    ts = sts[K]
    kw = dict(device=0, elems=elems, pieces=pieces, digests=crcs)
    arena, outs, d_bases, offs, base_offs, before = _arena(torch, ts, bases)
    prefill = [(o, b) for o, b in zip(base_offs, bases) if b is not None]
    u8 = lambda o, n, e: arena[o:o + n].view(getattr(torch, DT[e]))  # noqa: E731

    def refused(pattern, bs=d_bases, twin_offs=base_offs, table=members, n_links=K, src=container):
        with pytest.raises(orz_amd.OrzError) as info:
            orz_amd.decode_planes_into(src, outs, bases=bs, members=table, links=n_links, **kw)
        text = str(info.value)
        assert "orz_decode_tensors_chain failed (-22): " in text and pattern in text and not isinstance(info.value, orz_amd.OrzDigestError)
        assert _host(arena) == before
        twin = _twin(src, table, elems, pieces, ts, offs, twin_offs, arena.numel(), prefill, crcs, links=n_links)
        assert twin.rc == ch.EINVAL and twin.err == text.split("): ", 1)[1] and twin.arena == before

    M1 = len(links[0][1])
    refused("2 links of %d members for %d members" % (M1, K * M1), n_links=2)
    refused("2 links of %d members for %d members" % (M1, 2 * M1 + 1), table=members[:2 * M1 + 1], n_links=2)
    # what plane_piece_count refuses, in link 2: the first and the last piece of plane 0 of tensor 0 exchanged
    f, q = 2 * M1, pieces[0]
    cut = list(members)
    cut[f], cut[f + q - 1] = members[f + q - 1], members[f]
    refused("the pieces of link 2's destination 0 are no multiple of 16 elements: member %d decodes to 5 bytes" % f, table=cut)
    # a link whose tensor has another plane size than in link 0: link 1 made of tensors one element shorter
    short = [_typed(torch, d[:-e] if k == 1 else d, e) for k, (d, e) in enumerate(sts[2])]
    c1, m1, _, q1 = enc.encode_tensor_deltas(short, [None] * J, PIECE)
    assert q1 == pieces
    odd, odd_members = orz_amd.join_links([links[0], (c1, m1), links[2]])
    refused("link 1 has planes of 1028 bytes for destination 1, link 0 of 1029", table=odd_members, src=odd)
    # a base that overlaps its own destination at another address (two bytes in)
    bs, bo = list(d_bases), list(base_offs)
    bs[0], bo[0] = u8(offs[0] + 2, len(ts[0][0]), 2), offs[0] + 2
    refused("the base of destination 0 overlaps destination 0 at another address", bs=bs, twin_offs=bo)
    # what the Python face refuses itself, as ValueErrors
    with pytest.raises(ValueError, match="links is None or"):
        orz_amd.decode_planes_into(container, outs, bases=d_bases, members=members, links=0, **kw)
    with pytest.raises(ValueError, match="one base"):
        orz_amd.decode_planes_into(container, outs, bases=d_bases[:-1], members=members, links=K, **kw)
    assert _host(arena) == before


# ------------------------------------------------------------------------------------------------ one link
def test_one_link_is_the_call_without_links(packed):
    import orz_amd
    import torch

    sts, bases, links, _, _, elems, pieces, _ = packed
    ts = sts[1]
    c, m = links[0]
    crcs = cc.crcs_of(ts)
    got = []
    for extra in (dict(), dict(links=1)):
        arena, outs, d_bases, _, _, _ = _arena(torch, ts, bases)
        sizes, st = orz_amd.decode_planes_into(c, outs, device=0, members=m, elems=elems, pieces=pieces, bases=d_bases, digests=crcs, stats=True, **extra)
        got.append((sizes, st["host_waits"], st["members"], st["launches"], _host(arena)))
    assert got[0] == got[1] and got[0][1] == 6
    assert got[0][0] == [len(d) for d, _ in ts]


# ------------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("e", ch.ELEMS)
def test_the_merge_alone_through_the_hook(e):
    """PlaneMergeChain over K = 3 plane sets of 2^16 + 5 elements with a base: numpy's XOR.  Only the bytes are checked."""
    import torch

    from orz_amd import _native

    lib = _native.load()
    count, guard = (1 << 16) + 5, 64
    pitch = pc.pitch(count)
    links = [pc.tensor_bytes(e, count, 700 + 10 * k + e) for k in range(K)]
    base = pc.tensor_bytes(e, count, 790 + e)
    planes = np.full(K * e * pitch, pc.POISON, dtype=np.uint8)
    for k, d in enumerate(links):
        for p, pl in enumerate(pc.np_split(d, e)):
            at = (k * e + p) * pitch
            planes[at:at + count] = np.frombuffer(pl, dtype=np.uint8)
    d_planes = torch.from_numpy(planes).to("cuda:0")
    d_base = torch.frombuffer(bytearray(base), dtype=torch.uint8).to("cuda:0")
    d_out = torch.full((count * e + 2 * guard,), pc.POISON, dtype=torch.uint8, device="cuda:0")
    inter = d_out[guard:guard + count * e]
    assert inter.data_ptr() % 16 == 0 and d_planes.data_ptr() % 16 == 0 and d_base.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ms = ctypes.c_double()
    rc = lib.orz_plane_chain_move_time(0, ctypes.c_void_p(inter.data_ptr()), ctypes.c_void_p(d_base.data_ptr()), ctypes.c_void_p(d_planes.data_ptr()),
                                       count, e, K, 1, ctypes.byref(ms))
    assert rc == 0, _native.last_error()
    pc.same(_host(d_out), pc.expect_arena(d_out.numel(), [(guard, ch.xor_all(links + [base]))]), "the destination between its guards")
    assert _host(d_planes) == planes.tobytes() and _host(d_base) == base  # neither the planes nor the base is written
