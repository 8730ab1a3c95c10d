"""The delta layout (orz_amd/csrc/orz_planes.h: PlaneSplitDelta, PlaneMergeDelta, decode_members_planes with bases) on the emulation
backend.  The kernels alone: every element size at every count in ONE launch, rows with and without a base mixed, tensor and base
addresses at every remainder independently, inside poisoned arenas with guard gaps -- the split against numpy's (t ^ b) planes, the
merge as its inverse out of place and in place.  The driver on containers the ORACLE's encoder made of numpy's XOR planes: bytes,
sizes, launches and host waits against the same call without bases, digests, a wrong base, every refusal before a byte changes.
And the size the issue's table states for the bf16 step, from the oracle alone."""
import pytest

import _crccases as cc
import _deltacases as dc
import _piececases as pp
import _planecases as pc
from _deltacases import EBADMSG, EINVAL, POISON


@pytest.fixture(scope="module")
def lib():
    return dc.emu_lib()


@pytest.fixture(scope="module")
def stream(oracle):
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


# ------------------------------------------------------------------------------------------------ the kernels
def _arenas(ts, bases, rows, inter_rem, base_rem):
    """(the tensors' arena, its offsets, the bases' arena, its offsets or None, the staging arena, its offsets)"""
    inter_offs, ilen = pc.layout([len(d) for d, _ in ts], dc.rems_for(ts, inter_rem))
    base_offs, blen = pc.layout([len(d) for d, _ in ts], dc.rems_for(ts, base_rem), reverse=True)
    base_offs = [o if b is not None else None for o, b in zip(base_offs, bases)]
    stage_offs, slen = dc.staging_layout(ts, rows)
    return pc.Arena(ilen, align=16), inter_offs, pc.Arena(blen, align=16), base_offs, pc.Arena(slen), stage_offs


@pytest.mark.parametrize("base_rem", dc.REMS)
@pytest.mark.parametrize("inter_rem", dc.REMS)
def test_split_writes_the_planes_of_tensor_xor_base(lib, inter_rem, base_rem):
    ts, bases = dc.mixed()
    rows = dc.staged(ts, bases)
    inter, inter_offs, base, base_offs, stage, stage_offs = _arenas(ts, bases, rows, inter_rem, base_rem)
    for (d, _), io, b, bo in zip(ts, inter_offs, bases, base_offs):
        inter.write(io, d)
        if b is not None:
            base.write(bo, b)
    inter_before, base_before = inter.bytes(), base.bytes()
    units = dc.move(lib, False, ts, rows, inter, inter_offs, base, base_offs, stage, stage_offs)
    assert units == sum(-(-(len(d) // e) // 16) for (d, e), row in zip(ts, rows) if row)
    # the planes of numpy's XOR, and the padding up to each pitch still poison
    pc.same(stage.bytes(), pc.expect_arena(stage.length, dc.plane_pieces(dc.deltas(ts, bases), rows, stage_offs)), "the staging arena")
    assert inter.bytes() == inter_before and base.bytes() == base_before  # neither the source nor the base is written


def test_an_aligned_tensor_with_a_misaligned_base_goes_byte_by_byte_and_is_right(lib):
    """the base's address alone is off 16: the unit may not take the 16-byte path, whose base loads would be misaligned"""
    ts = [(pc.tensor_bytes(e, 4097, 5 + e), e) for e in dc.ELEMS]
    bases = [pc.tensor_bytes(e, 4097, 50 + e) for _, e in ts]
    rows = [True] * len(ts)
    for base_rem in (1, 8):
        inter, inter_offs, base, base_offs, stage, stage_offs = _arenas(ts, bases, rows, 0, base_rem)
        assert all((inter.base + o) % 16 == 0 for o in inter_offs) and all((base.base + o) % 16 == base_rem for o in base_offs)
        for (d, _), io, b, bo in zip(ts, inter_offs, bases, base_offs):
            inter.write(io, d)
            base.write(bo, b)
        dc.move(lib, False, ts, rows, inter, inter_offs, base, base_offs, stage, stage_offs)
        pc.same(stage.bytes(), pc.expect_arena(stage.length, dc.plane_pieces(dc.deltas(ts, bases), rows, stage_offs)), "the staging arena")
        dst = pc.Arena(inter.length, align=16)
        dc.move(lib, True, ts, rows, dst, inter_offs, base, base_offs, stage, stage_offs)
        pc.same(dst.bytes(), inter.bytes(), "the merged tensors")


@pytest.mark.parametrize("base_rem", dc.REMS)
@pytest.mark.parametrize("inter_rem", dc.REMS)
def test_merge_is_the_inverse_out_of_place(lib, inter_rem, base_rem):
    ts, bases = dc.mixed()
    rows = dc.staged(ts, bases)
    dst, dst_offs, base, base_offs, stage, stage_offs = _arenas(ts, bases, rows, inter_rem, base_rem)
    for b, bo in zip(bases, base_offs):
        if b is not None:
            base.write(bo, b)
    for o, pl in dc.plane_pieces(dc.deltas(ts, bases), rows, stage_offs):
        stage.write(o, pl)
    base_before, stage_before = base.bytes(), stage.bytes()
    dc.move(lib, True, ts, rows, dst, dst_offs, base, base_offs, stage, stage_offs)
    # the tensors, and nothing outside each destination's size
    pc.same(dst.bytes(), pc.expect_arena(dst.length, [(o, d) for (d, _), o, row in zip(ts, dst_offs, rows) if row]), "the arena of destinations")
    assert base.bytes() == base_before and stage.bytes() == stage_before


@pytest.mark.parametrize("rem", dc.REMS)
def test_merge_in_place(lib, rem):
    """base == destination: the destinations hold the bases on entry and the tensors on return"""
    ts, bases = dc.mixed()
    rows = dc.staged(ts, bases)
    dst, dst_offs, _, _, stage, stage_offs = _arenas(ts, bases, rows, rem, rem)
    for b, o in zip(bases, dst_offs):
        if b is not None:
            dst.write(o, b)
    for o, pl in dc.plane_pieces(dc.deltas(ts, bases), rows, stage_offs):
        stage.write(o, pl)
    stage_before = stage.bytes()
    dc.move(lib, True, ts, rows, dst, dst_offs, dst, [o if b is not None else None for o, b in zip(dst_offs, bases)], stage, stage_offs)
    pc.same(dst.bytes(), pc.expect_arena(dst.length, [(o, d) for (d, _), o, row in zip(ts, dst_offs, rows) if row]), "the arena of destinations")
    assert stage.bytes() == stage_before


# ------------------------------------------------------------------------------------------------ the driver
def _case(stream, S):
    """(tensors, bases, the oracle's container of numpy's XOR planes cut at S, elems, pieces)"""
    if S:
        ts = pp.tensors(S, seed=1) + pc.mixed_tensors(counts=(17,))
        bases = dc.with_bases(ts)
    else:
        ts, bases = dc.mixed()
    blob, _, _, qs = pp.container(stream, dc.deltas(ts, bases), S)
    return ts, bases, blob, [e for _, e in ts], qs


@pytest.mark.parametrize("S", [0, dc.PIECE])
def test_the_driver_restores_the_tensors_like_the_pieces_driver_its_deltas(lib, stream, S):
    ts, bases, blob, elems, pieces = _case(stream, S)
    assert any(e == 1 and b is not None and d for (d, e), b in zip(ts, bases))  # a single-byte destination with a base
    offs, caps, base_offs, total, prefill = dc.places(ts, bases)
    spots = list(zip(offs, caps))
    r = dc.decode_delta(lib, blob, None, spots, base_offs, elems, pieces, None, total, prefill=prefill)
    assert r.rc == 0, r.err
    assert r.out_lens == [len(d) for d, _ in ts]
    # the tensors in their places, the bases as they were, poison everywhere else
    pc.same(r.arena, pc.expect_arena(total, prefill + [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations and bases")
    # the same container through the same driver without bases: the deltas, in the same launches and host waits
    plain = dc.decode_delta(lib, blob, None, spots, None, elems, pieces, None, total, prefill=prefill)
    assert plain.rc == 0, plain.err
    pc.same(plain.arena, pc.expect_arena(total, prefill + [(o, d) for (d, _), o in zip(dc.deltas(ts, bases), offs)]), "the arena of deltas")
    assert (r.launches, r.host_waits, r.out_lens, r.members) == (plain.launches, plain.host_waits, plain.out_lens, plain.members)
    assert r.host_waits == 4 and r.launches == 6
    twin = pp.decode_pieces(pp.emu_lib(), blob, None, spots, elems, pieces, total)  # the pieces entry point's own twin
    assert twin.rc == 0 and twin.host_waits == r.host_waits and twin.out_lens == r.out_lens
    # with digests of the TENSORS: one wait and four launches more
    want = cc.crcs_of(ts)
    v = dc.decode_delta(lib, blob, None, spots, base_offs, elems, pieces, want, total, prefill=prefill)
    assert v.rc == 0, v.err
    assert v.arena == r.arena and v.out_crcs == want
    assert (v.host_waits, v.launches) == (r.host_waits + 1, r.launches + 4)


def test_the_driver_restores_in_place(lib, stream):
    ts, bases, blob, elems, pieces = _case(stream, dc.PIECE)
    offs, caps, total = cc.places(ts)
    prefill = [(o, b) for o, b in zip(offs, bases) if b is not None]
    in_place = [o if b is not None else None for o, b in zip(offs, bases)]
    want = cc.crcs_of(ts)
    r = dc.decode_delta(lib, blob, None, list(zip(offs, caps)), in_place, elems, pieces, want, total, prefill=prefill)
    assert r.rc == 0, r.err
    assert r.before != r.arena and r.out_crcs == want
    pc.same(r.arena, pc.expect_arena(total, [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations")


def test_a_host_container_with_a_table_and_few_members_in_flight(lib, stream):
    ts, bases, _, elems, _ = _case(stream, 0)
    ts, bases, elems = ts[:12], bases[:12], elems[:12]
    blobs = [stream(pl) for pl in pc.planes_of(dc.deltas(ts, bases))]
    blob, table = pc.table_of(blobs, order=list(reversed(range(len(blobs)))))
    offs, caps, base_offs, total, prefill = dc.places(ts, bases)
    r = dc.decode_delta(lib, blob, table, list(zip(offs, caps)), base_offs, elems, None, cc.crcs_of(ts), total, prefill=prefill, on_device=False, slots=3)
    assert r.rc == 0, r.err
    pc.same(r.arena, pc.expect_arena(total, prefill + [(o, d) for (d, _), o in zip(ts, offs)]), "the arena of destinations and bases")
    assert r.host_waits == 7 and r.launches == 4 + -(-r.members // 3) + 1 + 4


def test_a_wrong_base_is_a_digest_error_naming_the_tensor(lib, stream):
    ts, bases, blob, elems, pieces = _case(stream, dc.PIECE)
    offs, caps, base_offs, total, prefill = dc.places(ts, bases)
    want = cc.crcs_of(ts)
    j = max(k for k, b in enumerate(bases) if b is not None)
    wrong = [(o, cc.flip(b, 8 * (len(b) // 2) + 3) if o == base_offs[j] else b) for o, b in prefill]
    r = dc.decode_delta(lib, blob, None, list(zip(offs, caps)), base_offs, elems, pieces, want, total, prefill=wrong)
    assert r.rc == EBADMSG, r.err
    assert r.bad[0] == j and r.bad[1] == want[j] and r.bad[2] != want[j] and "destination %d " % j in r.err
    assert [k for k in range(len(ts)) if r.out_crcs[k] != want[k]] == [j]
    # the base, given out of place, is untouched
    assert all(r.arena[o:o + len(b)] == b for o, b in wrong)


def test_refusals_change_no_byte(lib, stream):
    ts = [(pc.tensor_bytes(e, 17, 3 + e), e) for e in (2, 1, 4)]
    bases = [pc.tensor_bytes(e, 17, 30 + e) for _, e in ts]
    blob = b"".join(stream(pl) for pl in pc.planes_of(dc.deltas(ts, bases)))
    elems = [e for _, e in ts]
    offs, caps, base_offs, total, prefill = dc.places(ts, bases)
    # destination 1 in place, so that an in-place base stands among the bytes that may not change
    base_offs[1] = offs[1]
    prefill = [(o, b) for o, b in zip(base_offs, bases)]
    spots = list(zip(offs, caps))
    good = dc.decode_delta(lib, blob, None, spots, base_offs, elems, None, cc.crcs_of(ts), total, prefill=prefill)
    assert good.rc == 0, good.err

    def refused(bs, pattern, sp=spots):
        r = dc.decode_delta(lib, blob, None, sp, bs, elems, None, cc.crcs_of(ts), total, prefill=prefill)
        assert r.rc == EINVAL and pattern in r.err, r.err
        assert r.arena == r.before and r.launches == 4  # (the index's two launches, the plan and its scan: no decode launch)
        assert r.out_crcs == [0xDEADBEEF] * len(ts)

    # a base that wraps the address space
    refused([base_offs[0], base_offs[1], ("abs", (1 << 64) - 16)], "the base of destination 2 wraps the address space")
    # one that overlaps its own destination at another address: one byte in, and from in front of it
    refused([offs[0] + 1, base_offs[1], base_offs[2]], "the base of destination 0 overlaps destination 0 at another address")
    refused([offs[0] - 2, base_offs[1], base_offs[2]], "the base of destination 0 overlaps destination 0 at another address")
    # one that overlaps another destination: its bytes, and its capacity behind them
    refused([base_offs[0], base_offs[1], offs[0]], "the base of destination 2 overlaps destination 0")
    refused([base_offs[0], offs[2] + caps[2] - 1, base_offs[2]], "the base of destination 1 overlaps destination 2")
    # what the driver refuses without bases is refused with them, before a byte changes
    short = list(spots)
    short[2] = (offs[2], len(ts[2][0]) - 1)
    r = dc.decode_delta(lib, blob, None, short, base_offs, elems, None, cc.crcs_of(ts), total, prefill=prefill)
    assert r.rc == dc.ENOMEM and "destination 2 " in r.err and r.arena == r.before


def test_bases_may_overlap_each_other_and_the_container(lib, stream):
    """all of them are only read: two destinations share one base, and a third's base lies inside the container's bytes"""
    shared = pc.tensor_bytes(2, 17, 9)
    ts = [(pc.tensor_bytes(2, 17, 1), 2), (pc.tensor_bytes(2, 17, 2), 2)]
    blob = b"".join(stream(pl) for pl in pc.planes_of(dc.deltas(ts, [shared, shared])))
    offs, caps, base_offs, total, prefill = dc.places(ts, [shared, None])
    r = dc.decode_delta(lib, blob, None, list(zip(offs, caps)), [base_offs[0], base_offs[0]], [2, 2], None, cc.crcs_of(ts), total, prefill=prefill)
    assert r.rc == 0, r.err
    pc.same(r.arena, pc.expect_arena(total, prefill + [(o, d) for (d, _), o in zip(ts, offs)]), "the arena")


def test_a_payload_flip_is_reported_as_today(lib, stream):
    """damage the decoder sees names the member; a base given out of place is untouched"""
    w, tuned = dc.bf16_step(4096)
    low, high = pc.np_split(dc.xor(tuned, w), 2)
    blobs = [stream(low), stream(high)]
    offs, caps, base_offs, total, prefill = dc.places([(tuned, 2)], [w], room=0)
    want = cc.crcs_of([(tuned, 2)])
    for k in range(64):
        bad = cc.flip(b"".join(blobs), 8 * len(blobs[0]) // 2 + 7 * k)
        r = dc.decode_delta(lib, bad, None, list(zip(offs, caps)), base_offs, [2], None, want, total, prefill=prefill)
        if r.rc == EINVAL and "status" in r.err:
            break
    else:
        raise AssertionError("no flip within 64 tries fails the decode: the set-up broke")
    assert "member 0," in r.err and "digest" not in r.err, r.err
    assert r.arena[base_offs[0]:base_offs[0] + len(w)] == w


# ------------------------------------------------------------------------------------------------ the size pin
def test_the_oracles_xor_planes_of_the_bf16_step_are_below_045_of_its_plain_planes(stream):
    """the issue's table: bf16, lr 1e-4, 2^19 elements -- 0.297 against 0.698 of the tensor's size, 0.43 of one another"""
    w, tuned = dc.bf16_step()
    plain = dc.planes_size(stream, tuned, 2)
    delta = dc.planes_size(stream, dc.xor(tuned, w), 2)
    print("plain planes %d, XOR planes %d: %.3f" % (plain, delta, delta / plain))
    assert delta < 0.45 * plain
