"""GPU tier: element ranges of delta containers read against their bases (orz_reader_set_bases, ElementGatherDelta) through the
Python face.  Bars: a read with bases equals, byte for byte, the read of the same reader with the bases withdrawn XORed in torch
with the base slices, and the input tensors' slices; read_tensor(digest=) vouches for the restored tensor, so no bases or a wrong
base is a digest error; a read in place inside a poisoned arena leaves the restored rows in the base and nothing else changed; a
mixed batch costs the launches and host waits of the same call without bases; with cursors a second walk decodes nothing; bytes,
the refusal's message and host waits agree with the emulation twin (tests/emu/emu_reader_bases.cpp) on the same container.  The
shapes are those of test_gpu_delta.py: a few dozen members of a few KB at most."""
import pytest

import _basecases as bc
import _crccases as cc
import _deltacases as dc
import _elemcases as ec
import _planecases as pc

pytestmark = pytest.mark.gpu

POISON = pc.POISON
PIECE = 512  # 16 x 32: the tensors of 1029 elements are three pieces a plane
# (element size, elements, with a base): every element size with a base, single bytes and int64 without one too, an empty tensor
SHAPES = ((2, 1029, True), (1, 1029, True), (4, 17, True), (8, 33, False), (1, 16, False), (2, 0, False), (4, 1029, True), (8, 15, True))
DT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


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


@pytest.fixture(scope="module")
def enc():
    import orz_amd
    import torch

    torch.cuda.init()  # (torch opens the device before the library does, as in the other GPU tests)
    e = orz_amd.MemberEncoder(device=0, level=1, jobs=3)
    yield e
    e.close()


class Packed:
    pass


@pytest.fixture(scope="module", params=[0, PIECE])
def packed(request, enc):
    """the tensors and bases as bytes and on the device, their delta container at a piece size of P, and its digests"""
    import torch

    p = Packed()
    p.P = request.param
    p.ts, p.bases = _case()
    p.tensors = [_typed(torch, d, e) for d, e in p.ts]
    p.d_bases = [_typed(torch, b, e) if b is not None else None for b, (_, e) in zip(p.bases, p.ts)]
    p.container, p.members, p.elems, p.pieces, p.crcs = enc.encode_tensor_deltas(p.tensors, p.d_bases, p.P, digests=True)
    assert p.crcs == cc.crcs_of(p.ts)  # the digests of the INPUT tensors
    assert (max(p.pieces) > 1) == bool(p.P)
    return p


def _reader(p, bases="own", **kw):
    import orz_amd

    return orz_amd.MemberReader(p.container, device=0, members=p.members, elems=p.elems, pieces=p.pieces,
                                bases=p.d_bases if bases == "own" else bases, **kw)


def _windows(ts):
    """of every tensor: all of it, and a window that starts and ends off the unit and piece borders"""
    out = []
    for j, (d, e) in enumerate(ts):
        c = len(d) // e
        out += [(j, 0, c)] + ([(j, 15, c - 15 - 3), (j, 500, 30)] if c > 600 else [(j, 1, c - 2)] if c > 2 else [])
    return out


def _base_slices(torch, p, ranges):
    """the bytes to XOR into a read of `ranges` without bases: each range's slice of its base, zeros where there is none"""
    parts = []
    for j, f, c in ranges:
        e = p.ts[j][1]
        b = p.d_bases[j]
        parts.append(b.view(torch.uint8)[f * e:(f + c) * e] if b is not None else torch.zeros(c * e, dtype=torch.uint8, device="cuda:0"))
    return torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device="cuda:0")


# ------------------------------------------------------------------------------------------------ bytes
def test_a_read_with_bases_is_the_read_without_them_xored_with_the_base_slices(packed):
    import torch

    p = packed
    rd = _reader(p)
    try:
        assert rd.tensors == [(c, e) for e, c, _ in SHAPES]
        windows = _windows(p.ts)
        for ranges in [windows] + [[w] for w in windows]:
            rd.set_bases(p.d_bases)
            got, st = rd.read_elements(ranges, stats=True)
            rd.set_bases(None)
            plain, st0 = rd.read_elements(ranges, stats=True)
            assert torch.equal(got, plain ^ _base_slices(torch, p, ranges)), ranges
            assert _host(got) == ec.np_elements(p.ts, ranges), ranges
            assert _host(plain) == ec.np_elements(dc.deltas(p.ts, p.bases), ranges)
            assert (st["launches"], st["host_waits"], st["decoded_bytes"]) == (st0["launches"], st0["host_waits"], st0["decoded_bytes"])
        assert [_host(b) for b in p.d_bases if b is not None] == [b for b in p.bases if b is not None]  # the bases are only read
    finally:
        rd.close()


def test_a_mixed_batch_costs_what_it_costs_without_bases(packed):
    p = packed
    # out of order, repeated, overlapping, empty, every element size, with and without a base, across unit and piece borders
    ranges = [(6, 1000, 29), (0, 3, 40), (3, 0, 33), (1, 0, 0), (0, 3, 40), (4, 1, 15), (6, 500, 30), (6, 511, 3), (5, 0, 0), (7, 14, 1),
              (1, 17, 1000), (2, 16, 1), (3, 1, 31), (0, 1029, 0), (1, 1, 1), (0, 510, 519)]
    assert {(p.ts[j][1], p.bases[j] is not None) for j, _, c in ranges if c} == {(1, True), (1, False), (2, True), (4, True), (8, True), (8, False)}
    rd = _reader(p)
    try:
        got, st = rd.read_elements(ranges, stats=True)
        assert _host(got) == ec.np_elements(p.ts, ranges)
        rd.set_bases([])
        plain, st0 = rd.read_elements(ranges, stats=True)
        assert _host(plain) == ec.np_elements(dc.deltas(p.ts, p.bases), ranges)
        assert st["launches"] == st0["launches"] == 1 and st["host_waits"] == st0["host_waits"] == 3
        assert (st["members_decoded"], st["decoded_bytes"], st["out_bytes"]) == (st0["members_decoded"], st0["decoded_bytes"], st0["out_bytes"])
        # ranges of tensors without a base, on a reader that has bases: the delta's bytes, which are the tensor's
        rd.set_bases(p.d_bases)
        lone = [r for r in ranges if p.bases[r[0]] is None]
        got, st = rd.read_elements(lone, stats=True)
        rd.set_bases(None)
        plain, st0 = rd.read_elements(lone, stats=True)
        assert _host(got) == _host(plain) == ec.np_elements(p.ts, lone) and (st["launches"], st["host_waits"]) == (st0["launches"], st0["host_waits"])
    finally:
        rd.close()


# ------------------------------------------------------------------------------------------------ digests
def test_digests_vouch_for_the_restored_tensors(packed):
    import orz_amd
    import torch

    p = packed
    rd = _reader(p)
    try:
        for j, (d, e) in enumerate(p.ts):
            assert _host(rd.read_tensor(j, digest=p.crcs[j])) == d
            out = torch.empty(len(d) // e, dtype=getattr(torch, DT[e]), device="cuda:0")
            assert _host(rd.read_tensor(j, out=out, digest=p.crcs[j])) == d == _host(out)
        based = [j for j, b in enumerate(p.bases) if b is not None]
        # a wrong base: ONE flipped bit
        j = based[-1]
        wrong = list(p.d_bases)
        wrong[j] = p.d_bases[j].clone()
        wrong[j].view(torch.uint8)[len(p.bases[j]) // 2] ^= 0x10
        rd.set_bases(wrong)
        with pytest.raises(orz_amd.OrzDigestError) as info:
            rd.read_tensor(j, digest=p.crcs[j])
        assert info.value.tensor == j and info.value.expected == p.crcs[j] and info.value.computed != p.crcs[j]
        assert _host(rd.read_tensor(based[0], digest=p.crcs[based[0]])) == p.ts[based[0]][0]
        # no bases: the delta has another digest than the tensor
        rd.set_bases(None)
        for j in based:
            with pytest.raises(orz_amd.OrzDigestError) as info:
                rd.read_tensor(j, digest=p.crcs[j])
            assert info.value.tensor == j and info.value.computed == cc.crcs_of(dc.deltas(p.ts, p.bases))[j]
        for j in set(range(len(p.ts))) - set(based):
            assert _host(rd.read_tensor(j, digest=p.crcs[j])) == p.ts[j][0]
    finally:
        rd.close()


def test_a_flipped_payload_bit_is_reported_as_without_bases(packed):
    """the same damaged container through a reader with bases (held to the tensor's digest) and one without (held to the delta's):
    the same kind of error -- the member's decode, or the digest -- for the same member or tensor"""
    import orz_amd
    import torch

    p = packed
    delta_crcs = cc.crcs_of(dc.deltas(p.ts, p.bases))
    m = max(range(len(p.members)), key=lambda k: p.members[k][1])
    at, length = p.members[m]
    firsts = [sum(e * q for e, q in zip(p.elems[:j], p.pieces[:j])) for j in range(len(p.ts) + 1)]
    j = next(k for k in range(len(p.ts)) if firsts[k] <= m < firsts[k + 1])
    kinds = set()
    for k in range(6):
        host = bytearray(_host(p.container))
        bit = 8 * at + 8 * length // 2 + 7 * k
        host[bit // 8] ^= 1 << (bit % 8)
        bad = torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")
        got = []
        for bs, digests in ((p.d_bases, p.crcs), (None, delta_crcs)):
            rd = orz_amd.MemberReader(bad, device=0, members=p.members, elems=p.elems, pieces=p.pieces, bases=bs)
            try:
                with pytest.raises(orz_amd.OrzError) as info:
                    rd.read_tensor(j, digest=digests[j])
            finally:
                rd.close()
            err = info.value
            got.append(("digest", err.tensor) if isinstance(err, orz_amd.OrzDigestError) else ("member", str(err).split("): ", 1)[1]))
        assert got[0] == got[1], (k, got)
        kinds.add(got[0][0])
    print("kinds of error over six flips:", sorted(kinds))


# ------------------------------------------------------------------------------------------------ in place
def _arena_of_bases(torch, p, rem):
    """(a poisoned arena that holds the bases in reverse order at `rem` modulo 16 -- "e": the element size --, the bases as views of
    it, their offsets, what the arena holds)"""
    sizes = [len(b) if b is not None else 0 for b in p.bases]
    offs, total = pc.layout(sizes, dc.rems_for(p.ts, rem), reverse=True)
    before = pc.expect_arena(total, [(o, b) for o, b in zip(offs, p.bases) if b is not None])
    arena = torch.frombuffer(bytearray(before), dtype=torch.uint8).to("cuda:0")
    assert arena.data_ptr() % 16 == 0
    views = [arena[o:o + len(b)].view(getattr(torch, DT[e])) if b is not None else None for o, b, (_, e) in zip(offs, p.bases, p.ts)]
    return arena, views, offs, before


@pytest.mark.parametrize("rem", [0, "e"])
def test_a_read_in_place_restores_the_rows_in_the_base(packed, rem):
    import torch

    p = packed
    arena, views, offs, before = _arena_of_bases(torch, p, rem)
    rd = _reader(p, bases=views)
    try:
        want = bytearray(before)
        for j, (d, e) in enumerate(p.ts):
            if views[j] is None:
                continue
            c = len(d) // e
            for first, count in ((17, c - 17 - 2), (0, 3)) if c > 600 else ((1, c - 2),):
                got = rd.read_tensor(j, first, count, out=views[j][first:first + count])
                assert got.data_ptr() == views[j].data_ptr() + first * e and got.numel() == count
                want[offs[j] + first * e:offs[j] + (first + count) * e] = d[first * e:(first + count) * e]
                pc.same(_host(arena), bytes(want), "the arena of bases after rows %d .. %d of tensor %d" % (first, first + count, j))
    finally:
        rd.close()


def test_refusals_bytes_and_host_waits_agree_with_the_twin(packed):
    import orz_amd
    import torch

    p = packed
    lib = bc.emu_lib()
    twin = bc.BaseReader(lib, _host(p.container), table=p.members)
    held = bc.Held(p.ts, p.bases, rem="e")
    arena, views, offs, before = _arena_of_bases(torch, p, "e")
    rd = _reader(p, bases=views)
    try:
        assert twin.h, twin.err
        assert twin.set_planes_pieces(p.elems, p.pieces) == (0, "") and twin.set_bases(held.addrs) == (0, "")
        ranges = _windows(p.ts)
        got, st = rd.read_elements(ranges, stats=True)
        r = twin.read_elements(ranges, len(ec.np_elements(p.ts, ranges)))
        assert r.rc == 0 and r.out == _host(got) and held.untouched()
        assert (r.host_waits, r.launches, r.members_decoded, r.out_bytes) == (st["host_waits"], st["launches"], st["members_decoded"], st["out_bytes"])
        # a base slice one element off its range's destination: refused with the twin's words, nothing written, the reader usable
        j, first, count = 6, 16, 100
        e = p.ts[j][1]
        with pytest.raises(orz_amd.OrzError) as info:
            rd.read_tensor(j, first, count, out=views[j][first + 1:first + 1 + count])
        text = str(info.value)
        assert "orz_reader_read_elements failed (-22): " in text and "the base slice of range 0 (tensor 6) overlaps" in text
        assert _host(arena) == before
        whole = pc.Arena(len(p.bases[j]), align=16)
        whole.write(0, p.bases[j])
        addrs = list(held.addrs)
        addrs[j] = whole.base
        assert twin.set_bases(addrs) == (0, "")
        r = twin.read_elements([(j, first, count)], raw=(whole.base + (first + 1) * e, count * e))
        assert r.rc == bc.EINVAL and r.err == text.split("): ", 1)[1] and r.host_waits == 0 and whole.bytes() == p.bases[j]
        # what the Python face refuses itself
        with pytest.raises(ValueError, match="one base"):
            rd.set_bases(views[:-1])
        with pytest.raises(ValueError, match="base 0 has"):
            rd.set_bases([views[0][:-1]] + views[1:])
        with pytest.raises(ValueError, match="base 0 lies on cpu"):
            rd.set_bases([views[0].cpu()] + views[1:])
        assert _host(rd.read_tensor(j, first, count)) == ec.np_elements(p.ts, [(j, first, count)])  # (the bases are those set before)
        # a declaration withdraws the bases
        rd.set_planes(p.elems, p.pieces)
        assert _host(rd.read_tensor(j, first, count)) == ec.np_elements(dc.deltas(p.ts, p.bases), [(j, first, count)])
    finally:
        rd.close()
        twin.close()


# ------------------------------------------------------------------------------------------------ cursors
def test_a_second_walk_with_cursors_decodes_nothing(packed):
    import orz_amd

    p = packed
    j, step = 0, 200  # int16, 1029 elements, with a base: at PIECE three pieces a plane
    budget = 8 * (1280 + orz_amd.MemberReader.cursor_state_bytes())
    rd = _reader(p, cache_bytes=budget)
    try:
        windows = [(j, f, min(step, 1029 - f)) for f in range(0, 1029, step)]
        for walk in (0, 1):
            decoded = 0
            for w in windows:
                got, st = rd.read_elements([w], stats=True)
                assert _host(got) == ec.np_elements(p.ts, [w]), w
                assert st["host_waits"] == 2
                decoded += st["decoded_bytes"]
                if walk:
                    cs = rd.cache_stats()
                    assert st["launches"] == 0 and st["members_decoded"] == 0 and cs["hits"] > 0 and cs["resumed"] == cs["fresh"] == cs["uncached"] == 0
            assert (decoded == 0) == bool(walk), decoded
        # another base between two reads of one range: the cursors serve both
        other = p.d_bases[j] ^ 0x55
        rd.set_bases([other if k == j else b for k, b in enumerate(p.d_bases)])
        got, st = rd.read_elements([windows[2]], stats=True)
        assert st["decoded_bytes"] == 0 and _host(got) == dc.xor(ec.np_elements(dc.deltas(p.ts, p.bases), [windows[2]]), _host(other)[800:1200])
    finally:
        rd.close()
