"""The verified decode (decode_members_planes with a digest check: orz_amd/csrc/orz_planes.h, orz_crc.h) on the emulation backend,
on containers the ORACLE's encoder made: the three layouts inside poisoned arenas with guard gaps -- digests against zlib, host
waits and ALL launches against the same call without a check --, the two kinds of damage no decoder reports (a member table whose
entries are mixed up, a payload bit that flips), damage the decoder does report, and every refusal before a byte is written."""
import zlib

import pytest

import _crccases as cc
import _piececases as pp
import _planecases as pc
from _crccases import EBADMSG, EINVAL, ENOMEM, POISON


@pytest.fixture(scope="module")
def lib():
    return cc.emu_lib()


@pytest.fixture(scope="module")
def stream(oracle):
    """the oracle's stream of some bytes at level 1, remembered"""
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


def _layout(stream, which):
    """(tensors, container, elems or None, pieces or None) of a layout"""
    if which == "whole":  # a member per tensor, no element sizes
        ts = pc.mixed_tensors(counts=cc.COUNTS)
        return ts, b"".join(stream(d) for d, _ in ts), None, None
    if which == "planes":
        ts = pc.mixed_tensors(counts=cc.COUNTS)
        return ts, b"".join(stream(pl) for pl in pc.planes_of(ts)), [e for _, e in ts], None
    ts = pp.tensors(cc.PIECE, seed=1) + pc.mixed_tensors(counts=(17,))
    blob, _, _, qs = pp.container(stream, ts, cc.PIECE)
    return ts, blob, [e for _, e in ts], qs


# ------------------------------------------------------------------------------------------------ good containers
@pytest.mark.parametrize("which", ["whole", "planes", "pieces"])
def test_a_good_container_passes(lib, stream, which):
    ts, blob, elems, pieces = _layout(stream, which)
    offs, caps, total = cc.places(ts)
    want = cc.crcs_of(ts)
    r = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), elems, pieces, want, total)
    assert r.rc == 0, r.err
    assert r.out_crcs == want and r.out_lens == [len(d) for d, _ in ts]
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations")
    plain = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), elems, pieces, want, total, verify=False)
    assert plain.rc == 0 and plain.arena == r.arena and plain.out_crcs == [0xDEADBEEF] * len(ts)
    assert r.host_waits == plain.host_waits + 1 == 5
    # the index's two launches, the plan, its scan, one round of decodes and -- unless every element is a byte -- the merge; the
    # digests add their table, the tiles, the fold and the sums
    assert plain.launches == (5 if which == "whole" else 6) and r.launches == plain.launches + 4
    if pieces is not None:  # the emulation twin of the unverified entry point counts the same waits
        twin = pp.decode_pieces(pp.emu_lib(), blob, None, list(zip(offs, caps)), elems, pieces, total)
        assert twin.rc == 0 and twin.host_waits == plain.host_waits and twin.arena == r.arena


def test_a_host_container_with_a_permuted_table(lib, stream):
    ts = pc.mixed_tensors(counts=(1, 17))
    blob, table = pc.table_of([stream(pl) for pl in pc.planes_of(ts)], order=list(reversed(range(sum(e for _, e in ts)))))
    offs, caps, total = cc.places(ts)
    args = (lib, blob, table, list(zip(offs, caps)), [e for _, e in ts], None, cc.crcs_of(ts), total)
    r, plain = cc.decode_verified(*args, on_device=False), cc.decode_verified(*args, on_device=False, verify=False)
    assert r.rc == plain.rc == 0, r.err
    assert r.out_crcs == cc.crcs_of(ts) and r.host_waits == plain.host_waits + 1 == 7
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations")


def test_few_members_in_flight(lib, stream):
    ts, blob, elems, pieces = _layout(stream, "pieces")
    offs, caps, total = cc.places(ts)
    r = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), elems, pieces, cc.crcs_of(ts), total, slots=3)
    assert r.rc == 0 and r.out_crcs == cc.crcs_of(ts) and r.host_waits == 5
    assert r.launches == 4 + -(-r.members // 3) + 1 + 4


# ------------------------------------------------------------------------------------------------ silent damage
def test_a_mixed_up_table_is_silent_without_digests(lib, stream):
    """the table entries of plane 0 of an int16 tensor and plane 1 of an int32 tensor, 17 bytes each, exchanged"""
    ts = pc.mixed_tensors(counts=(1, 17))
    planes = pc.planes_of(ts)
    first = pp.first_members(ts, [1] * len(ts))
    a = next(j for j, (d, e) in enumerate(ts) if e == 2 and len(d) == 34)
    b = next(j for j, (d, e) in enumerate(ts) if e == 4 and len(d) == 68)
    ma, mb = first[a], first[b] + 1
    assert len(planes[ma]) == len(planes[mb]) == 17 and planes[ma] != planes[mb]
    blob, table = pc.table_of([stream(pl) for pl in planes])
    table[ma], table[mb] = table[mb], table[ma]
    wrong = list(planes)
    wrong[ma], wrong[mb] = planes[mb], planes[ma]
    got = {j: pc.np_merge(wrong[first[j]:first[j] + ts[j][1]]) for j in (a, b)}
    offs, caps, total = cc.places(ts)
    want = cc.crcs_of(ts)
    args = (lib, blob, table, list(zip(offs, caps)), [e for _, e in ts], None, want, total)
    plain = cc.decode_verified(*args, verify=False)
    # the gap: the unverified call reports success and two tensors hold wrong bytes
    assert plain.rc == 0, plain.err
    wrong_arena = pc.expect_arena(total, [(o, got.get(j, d)) for j, ((d, _), o) in enumerate(zip(ts, offs))])
    pc.same(plain.arena, wrong_arena, "the arena of the mixed-up decode")
    assert got[a] != ts[a][0] and got[b] != ts[b][0]
    r = cc.decode_verified(*args)
    low = min(a, b)
    assert r.rc == EBADMSG, r.err
    assert r.bad == (low, want[low], zlib.crc32(got[low])) and r.out_crcs[low] == zlib.crc32(got[low])
    assert "destination %d " % low in r.err and "0x%08x" % want[low] in r.err and "0x%08x" % zlib.crc32(got[low]) in r.err
    assert [j for j in range(len(ts)) if r.out_crcs[j] != want[j]] == sorted((a, b))
    assert r.arena == plain.arena and r.host_waits == plain.host_waits + 1


def _silent_flip(lib, stream, head, weights):
    """(the damaged container, the flipped bit's number among those tried): the first flip of every 7th bit of the low plane's
    stream, from its middle on, whose UNVERIFIED decode succeeds with other bytes"""
    low, high = pc.np_split(weights, 2)
    blobs = [stream(head), stream(low), stream(high)]
    at = 8 * len(blobs[0])
    offs, caps, total = cc.places([(head, 1), (weights, 2)], room=0)
    for k in range(32):
        bit = at + 8 * len(blobs[1]) // 2 + 7 * k
        assert bit < at + 8 * len(blobs[1])
        bad = cc.flip(b"".join(blobs), bit)
        plain = cc.decode_verified(lib, bad, None, list(zip(offs, caps)), [1, 2], None, [0, 0], total, verify=False)
        if plain.rc == 0 and plain.arena[offs[1]:offs[1] + len(weights)] != weights:
            assert plain.out_lens == [len(head), len(weights)] and plain.arena[offs[0]:offs[0] + len(head)] == head
            return bad, k, plain
    raise AssertionError("no silent flip within 32 tries: the set-up broke")


def test_a_silent_flip_is_caught(lib, stream):
    head, weights = pc.tensor_bytes(1, 33, 4), cc.bf16_weights()
    assert len(weights) == 8192
    bad, k, plain = _silent_flip(lib, stream, head, weights)
    offs, caps, total = cc.places([(head, 1), (weights, 2)], room=0)
    want = cc.crcs_of([(head, 1), (weights, 2)])
    r = cc.decode_verified(lib, bad, None, list(zip(offs, caps)), [1, 2], None, want, total)
    assert r.rc == EBADMSG and r.bad[0] == 1 and r.bad[1] == want[1] and r.bad[2] != want[1], r.err
    assert r.out_crcs[0] == want[0] and r.out_crcs[1] == zlib.crc32(r.arena[offs[1]:offs[1] + len(weights)])
    assert r.arena == plain.arena
    good = cc.decode_verified(lib, b"".join(stream(m) for m in (head,) + tuple(pc.np_split(weights, 2))), None, list(zip(offs, caps)), [1, 2], None, want, total)
    assert good.rc == 0 and good.out_crcs == want


def test_damage_the_decoder_sees_is_reported_as_the_member(lib, stream):
    """a flip in the high plane's stream whose decode FAILS: ORZ_EINVAL naming the member comes first, though the digests differ too"""
    head, weights = pc.tensor_bytes(1, 33, 4), cc.bf16_weights()
    blobs = [stream(m) for m in (head,) + tuple(pc.np_split(weights, 2))]
    at = 8 * (len(blobs[0]) + len(blobs[1]))
    offs, caps, total = cc.places([(head, 1), (weights, 2)], room=0)
    want = cc.crcs_of([(head, 1), (weights, 2)])
    for k in range(64):
        bad = cc.flip(b"".join(blobs), at + 8 * len(blobs[2]) // 2 + 7 * k)
        r = cc.decode_verified(lib, bad, None, list(zip(offs, caps)), [1, 2], None, want, total)
        if r.rc == EINVAL and "status" in r.err:
            break
    else:
        raise AssertionError("no flip within 64 tries fails the decode: the set-up broke")
    assert "member 2," in r.err and "digest" not in r.err, r.err
    assert r.out_crcs[0] == want[0] and r.out_crcs[1] == zlib.crc32(r.arena[offs[1]:offs[1] + len(weights)])  # the digest launches ran


def test_a_wrong_digest_for_the_last_of_many_names_it(lib, stream):
    ts, blob, elems, pieces = _layout(stream, "planes")
    offs, caps, total = cc.places(ts)
    want = cc.crcs_of(ts)
    last = max(j for j, (d, _) in enumerate(ts) if d)
    for j in (last, len(ts) - 1):  # (the very last tensor is empty: its digest is 0)
        given = list(want)
        given[j] ^= 1
        r = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), elems, pieces, given, total)
        assert r.rc == EBADMSG and r.bad == (j, given[j], want[j]) and "destination %d " % j in r.err, r.err
        assert r.out_crcs == want
    assert want[-1] == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(lib, stream):
    ts = pc.mixed_tensors(counts=(17,))
    blob = b"".join(stream(pl) for pl in pc.planes_of(ts))
    elems = [e for _, e in ts]
    offs, caps, total = cc.places(ts, room=0)
    want = cc.crcs_of(ts)
    untouched = bytes([POISON]) * total
    # a short destination
    short = list(caps)
    short[1] -= 1
    r = cc.decode_verified(lib, blob, None, list(zip(offs, short)), elems, None, want, total)
    assert r.rc == ENOMEM and "destination 1 " in r.err and r.launches == 4 and r.arena == untouched, r.err  # (the index, the plan and its scan)
    assert r.out_crcs == [0xDEADBEEF] * len(ts)
    # overlapping destinations
    over = list(offs)
    over[2] = offs[1] + 1
    r = cc.decode_verified(lib, blob, None, list(zip(over, caps)), elems, None, want, total)
    assert r.rc == EINVAL and "overlap" in r.err and r.arena == untouched, r.err
    # no digests
    r = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), elems, None, want, total, null_crcs=True)
    assert r.rc == EINVAL and "without digests" in r.err and r.launches == 0 and r.arena == untouched, r.err
    # planes that do not match the members
    r = cc.decode_verified(lib, blob, None, list(zip(offs, caps)), None, None, want, total)
    assert r.rc == EINVAL and "planes for" in r.err and r.arena == untouched, r.err


def test_a_sizing_call_ignores_the_digests(lib, stream):
    ts, blob, elems, pieces = _layout(stream, "pieces")
    for null in (True, False):
        r = cc.decode_verified(lib, blob, None, [(None, 0)] * len(ts), elems, pieces, [0] * len(ts), 64, sizing=True, null_crcs=null)
        assert r.rc == 0, r.err
        assert r.out_lens == [len(d) for d, _ in ts] and r.launches == 2 and r.arena == bytes([POISON]) * 64  # (the index's two launches)
        assert r.out_crcs == [0xDEADBEEF] * len(ts)
