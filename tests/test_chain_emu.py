"""Chains of delta links (orz_amd/csrc/orz_chain.h: PlaneMergeChain, ChainPlan, decode_members_chain) on the emulation backend.
The kernel alone: every element size at every count in ONE launch over K plane sets, rows with and without a base mixed,
destination and base addresses at every remainder independently, inside poisoned arenas with guard gaps, against numpy's XOR, out
of place and in place; one link's planes off 16; K = 1 against PlaneMergeDelta.  The driver on containers the ORACLE's encoder made
of numpy's XOR planes of the steps of a run: bytes against the last step and against K sequential in-place delta calls, launches
and host waits against ONE delta call on as many members, no bases, link order, digests, every refusal before a byte changes,
damage.  And the plan alone on invented size columns beyond 32 bits."""
import pytest

import _chaincases as ch
import _crccases as cc
import _deltacases as dc
import _planecases as pc
from _chaincases import EBADMSG, EINVAL, ENOMEM, MASK


@pytest.fixture(scope="module")
def lib():
    return ch.emu_lib()


@pytest.fixture(scope="module")
def stream(oracle):
    memo = {}

    def get(data):
        if data not in memo:
            memo[data] = oracle.encode(data, 1)
        return memo[data]

    return get


# ------------------------------------------------------------------------------------------------ the kernel
def _mixed():
    """(tensors, bases): every element size at every count of the issue in ONE list, with and without a base"""
    ts = pc.mixed_tensors(counts=ch.COUNTS)
    bases = dc.with_bases(ts)
    # every element size with and without a base, among the tensors with a full unit and a partial one
    assert {(e, b is not None) for (d, e), b in zip(ts, bases) if len(d) // e > 16} =={(e, h) for e in ch.ELEMS for h in (False, True)}
    return ts, bases


def _arenas(ts, bases, inter_rem, base_rem):
    inter_offs, ilen = pc.layout([len(d) for d, _ in ts], dc.rems_for(ts, inter_rem))
    base_offs, blen = pc.layout([len(d) for d, _ in ts], dc.rems_for(ts, base_rem), reverse=True)
    base_offs = [o if b is not None else None for o, b in zip(base_offs, bases)]
    return pc.Arena(ilen, align=16), inter_offs, pc.Arena(blen, align=16), base_offs


@pytest.mark.parametrize("K", ch.LINKS)
@pytest.mark.parametrize("base_rem", dc.REMS)
@pytest.mark.parametrize("inter_rem", dc.REMS)
def test_merge_is_the_xor_of_the_links_and_the_base_out_of_place(lib, inter_rem, base_rem, K):
    ts, bases = _mixed()
    links = ch.link_tensors(ts, K)
    dst, dst_offs, base, base_offs = _arenas(ts, bases, inter_rem, base_rem)
    for b, bo in zip(bases, base_offs):
        if b is not None:
            base.write(bo, b)
    stage, link_offs = ch.stage_links(ts, links)
    base_before, stage_before = base.bytes(), stage.bytes()
    units = ch.chain_move(lib, ts, dst, dst_offs, base, base_offs, stage, link_offs)
    assert units == sum(-(-(len(d) // e) // 16) for d, e in ts)
    # numpy's XOR in every destination, poison in the guards and everywhere else
    pc.same(dst.bytes(), pc.expect_arena(dst.length, list(zip(dst_offs, ch.merged(links, bases)))), "the arena of destinations")
    # neither the planes nor a base is written, and the poison between count and pitch is intact
    assert base.bytes() == base_before and stage.bytes() == stage_before


@pytest.mark.parametrize("K", ch.LINKS)
@pytest.mark.parametrize("rem", dc.REMS)
def test_merge_in_place(lib, rem, K):
    """base == destination: the destinations hold the bases on entry and the XOR on return"""
    ts, bases = _mixed()
    links = ch.link_tensors(ts, K)
    dst, dst_offs, _, _ = _arenas(ts, bases, rem, rem)
    for b, o in zip(bases, dst_offs):
        if b is not None:
            dst.write(o, b)
    stage, link_offs = ch.stage_links(ts, links)
    stage_before = stage.bytes()
    ch.chain_move(lib, ts, dst, dst_offs, dst, [o if b is not None else None for o, b in zip(dst_offs, bases)], stage, link_offs)
    pc.same(dst.bytes(), pc.expect_arena(dst.length, list(zip(dst_offs, ch.merged(links, bases)))), "the arena of destinations")
    assert stage.bytes() == stage_before


@pytest.mark.parametrize("off", [1, 8])
def test_one_links_planes_off_16_send_the_whole_unit_byte_by_byte(lib, off):
    """everything at multiples of 16 but the planes of ONE link of each tensor: 16-byte loads of them would be misaligned"""
    ts = [(pc.tensor_bytes(e, 4097, 5 + e), e) for e in ch.ELEMS]
    bases = [pc.tensor_bytes(e, 4097, 50 + e) if e != 4 else None for _, e in ts]
    links = ch.link_tensors(ts, 3)
    dst, dst_offs, base, base_offs = _arenas(ts, bases, 0, 0)
    for b, bo in zip(bases, base_offs):
        if b is not None:
            base.write(bo, b)
    stage, link_offs = ch.stage_links(ts, links, shift={(j % 3, j): off for j in range(len(ts))})
    assert all((dst.base + o) % 16 == 0 for o in dst_offs) and all((base.base + o) % 16 == 0 for o in base_offs if o is not None)
    assert all(sorted((stage.base + link_offs[k][j]) % 16 for k in range(3)) == [0, 0, off] for j in range(len(ts)))
    stage_before = stage.bytes()
    ch.chain_move(lib, ts, dst, dst_offs, base, base_offs, stage, link_offs)
    pc.same(dst.bytes(), pc.expect_arena(dst.length, list(zip(dst_offs, ch.merged(links, bases)))), "the arena of destinations")
    assert stage.bytes() == stage_before


@pytest.mark.parametrize("rem", dc.REMS)
def test_one_link_is_the_delta_merge_byte_for_byte(lib, rem):
    ts, bases = _mixed()
    links = ch.link_tensors(ts, 1)
    rows = [True] * len(ts)
    arenas = []
    for chain in (True, False):
        dst, dst_offs, base, base_offs = _arenas(ts, bases, rem, rem)
        for b, bo in zip(bases, base_offs):
            if b is not None:
                base.write(bo, b)
        stage, link_offs = ch.stage_links(ts, links)
        if chain:
            ch.chain_move(lib, ts, dst, dst_offs, base, base_offs, stage, link_offs)
        else:
            dc.move(lib, True, ts, rows, dst, dst_offs, base, base_offs, stage, link_offs[0])
        arenas.append((dst.bytes(), base.bytes(), stage.bytes()))
    assert arenas[0] == arenas[1]


# ------------------------------------------------------------------------------------------------ the driver
K = 3
ELS = [e for e, _, _ in ch.SHAPES]
M1 = 2 * 1 + 4 * 5 + 1 * 1  # the members of a link


@pytest.fixture(scope="module")
def run():
    """(steps, links): K + 1 steps of three tensors and the K deltas between them"""
    sts = ch.steps(K)
    assert all(a != b for s, t in zip(sts, sts[1:]) for (a, _), (b, _) in zip(s, t))
    return sts, ch.deltas_of(sts)


def _places(ts, in_place=False):
    """destinations, and their bases behind them (or in them): (spots, base offsets, arena length)"""
    if in_place:
        offs, caps, total = cc.places(ts)
        return list(zip(offs, caps)), list(offs), total
    offs, caps, base_offs, total, _ = dc.places(ts, [d for d, _ in ts])
    return list(zip(offs, caps)), base_offs, total


def _expect(total, spots, datas, base_offs=None, bases=None):
    kept = [] if bases is None else [(o, b) for o, (b, _) in zip(base_offs, bases)]
    return pc.expect_arena(total, kept + [(o, d) for (o, _), d in zip(spots, datas)])


def _one_delta_call(lib, blob, table, k, crcs_per_link, **kw):
    """ONE delta call on the same container, its k links' tensors as k x J destinations of their own: (launches, host waits, members)"""
    ts = [(b"\0" * (c * e), e) for e, c, _ in ch.SHAPES] * k
    offs, caps, total = cc.places(ts)
    qs = [5 if e == 4 else 1 for e in ELS] * k
    r = dc.decode_delta(lib, blob, table, list(zip(offs, caps)), [None] * len(ts), ELS * k, qs, crcs_per_link, total, **kw)
    return r


@pytest.mark.parametrize("in_place", [False, True])
def test_the_chain_restores_the_last_step(lib, stream, run, in_place):
    sts, links = run
    blob, _, qs, per_link = ch.chain_container(stream, links)
    assert qs == [1, 5, 1] and len(per_link[0]) == M1
    spots, base_offs, total = _places(sts[0], in_place)
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    r = ch.decode_chain(lib, blob, None, spots, base_offs, ELS, qs, None, total, K, prefill=prefill)
    assert r.rc == 0, r.err
    assert r.members == K * M1 and r.out_lens == [len(d) for d, _ in sts[0]]
    want = _expect(total, spots, [d for d, _ in sts[K]], base_offs, None if in_place else sts[0])
    pc.same(r.arena, want, "the arena of destinations and bases")
    # K sequential in-place delta calls, one link each: the same bytes
    arena = _expect(total, spots, [d for d, _ in sts[0]], base_offs, None if in_place else sts[0])
    in_offs = [o for o, _ in spots]
    for k in range(K):
        s = dc.decode_delta(lib, b"".join(per_link[k]), None, spots, in_offs, ELS, qs, None, total, prefill=[(0, arena)])
        assert s.rc == 0, s.err
        arena = s.arena
    assert arena == r.arena


@pytest.mark.parametrize("k", [1, 2, 3])
def test_launches_and_host_waits_are_those_of_one_delta_call_on_as_many_members(lib, stream, run, k):
    sts, links = run
    links = links[:k]
    spots, base_offs, total = _places(sts[0])
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    want = cc.crcs_of(sts[k])
    link_crcs = [c for ln in links for c in cc.crcs_of(ln)]
    for table, on_device, slots, waits in ((False, True, 0, 4), (True, True, 0, 5), (False, False, 0, 5), (True, False, 2, 6)):
        blob, tab, qs, _ = ch.chain_container(stream, links, table=table)
        for crcs, one_crcs in ((None, None), (want, link_crcs)):
            r = ch.decode_chain(lib, blob, tab, spots, base_offs, ELS, qs, crcs, total, k, prefill=prefill, on_device=on_device, slots=slots)
            assert r.rc == 0, r.err
            pc.same(r.arena, _expect(total, spots, [d for d, _ in sts[k]], base_offs, sts[0]), "the arena of destinations and bases")
            one = _one_delta_call(lib, blob, tab, k, one_crcs, on_device=on_device, slots=slots)
            assert one.rc == 0, one.err
            assert (r.launches, r.host_waits, r.members) == (one.launches, one.host_waits, one.members)
            assert r.members == k * M1 and r.host_waits == waits + (crcs is not None)
            if crcs is not None:
                assert r.out_crcs == want


def test_without_bases_the_result_is_the_xor_of_the_links(lib, stream, run):
    sts, links = run
    blob, _, qs, _ = ch.chain_container(stream, links)
    offs, caps, total = cc.places(sts[0])
    spots = list(zip(offs, caps))
    composed = [dc.xor(a, b) for (a, _), (b, _) in zip(sts[K], sts[0])]
    r = ch.decode_chain(lib, blob, None, spots, None, ELS, qs, None, total, K)
    assert r.rc == 0, r.err
    pc.same(r.arena, _expect(total, spots, composed), "the arena of destinations")
    # a chain whose link 0 is a plain keyframe restores without a base
    keyed = [sts[0]] + links
    blob, _, qs, _ = ch.chain_container(stream, keyed)
    r = ch.decode_chain(lib, blob, None, spots, None, ELS, qs, cc.crcs_of(sts[K]), total, K + 1)
    assert r.rc == 0, r.err
    pc.same(r.arena, _expect(total, spots, [d for d, _ in sts[K]]), "the arena of destinations")


def test_the_order_of_the_links_does_not_matter(lib, stream, run):
    sts, links = run
    spots, base_offs, total = _places(sts[0])
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    arenas = []
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):
        blob, tab, qs, _ = ch.chain_container(stream, links, table=True, order=order)
        r = ch.decode_chain(lib, blob, tab, spots, base_offs, ELS, qs, cc.crcs_of(sts[K]), total, K, prefill=prefill)
        assert r.rc == 0, r.err
        arenas.append(r.arena)
    assert all(a == arenas[0] for a in arenas)
    pc.same(arenas[0], _expect(total, spots, [d for d, _ in sts[K]], base_offs, sts[0]), "the arena of destinations and bases")


def test_digests_vouch_for_the_final_tensors(lib, stream, run):
    sts, links = run
    blob, tab, qs, _ = ch.chain_container(stream, links, table=True)
    spots, base_offs, total = _places(sts[0])
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    want = cc.crcs_of(sts[K])
    r = ch.decode_chain(lib, blob, tab, spots, base_offs, ELS, qs, want, total, K, prefill=prefill)
    assert r.rc == 0 and r.out_crcs == want, r.err
    # a wrong base: ONE flipped bit in the base of tensor 1
    j = 1
    wrong = [(o, cc.flip(d, 8 * (len(d) // 2) + 3) if k == j else d) for k, (o, d) in enumerate(prefill)]
    r = ch.decode_chain(lib, blob, tab, spots, base_offs, ELS, qs, want, total, K, prefill=wrong)
    assert r.rc == EBADMSG, r.err
    assert r.bad[0] == j and r.bad[1] == want[j] and r.bad[2] != want[j] and "destination %d " % j in r.err
    assert [k for k in range(len(ELS)) if r.out_crcs[k] != want[k]] == [j]
    assert all(r.arena[o:o + len(b)] == b for o, b in wrong)  # the bases, given out of place, are untouched
    # the table entries of plane 0 and plane 1 of tensor 0 in link 1 exchanged: the same sizes, other bytes
    mixed = list(tab)
    mixed[M1], mixed[M1 + 1] = tab[M1 + 1], tab[M1]
    silent = ch.decode_chain(lib, blob, mixed, spots, base_offs, ELS, qs, None, total, K, prefill=prefill)
    assert silent.rc == 0, silent.err
    assert silent.arena != _expect(total, spots, [d for d, _ in sts[K]], base_offs, sts[0])
    r = ch.decode_chain(lib, blob, mixed, spots, base_offs, ELS, qs, want, total, K, prefill=prefill)
    assert r.rc == EBADMSG and r.bad[0] == 0 and "destination 0 " in r.err, r.err
    assert r.arena == silent.arena


def test_refusals_change_no_byte(lib, stream, run):
    sts, links = run
    blob, tab, qs, _ = ch.chain_container(stream, links, table=True)
    spots, base_offs, total = _places(sts[0])
    base_offs = list(base_offs)
    base_offs[2] = spots[2][0]  # destination 2 in place: an in-place base stands among the bytes that may not change
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    want = cc.crcs_of(sts[K])
    good = ch.decode_chain(lib, blob, tab, spots, base_offs, ELS, qs, want, total, K, prefill=prefill)
    assert good.rc == 0, good.err

    def refused(pattern, table=tab, sp=spots, bs=base_offs, links_=K, rc=EINVAL, launches=4, the_blob=blob, pieces=qs):
        r = ch.decode_chain(lib, the_blob, table, sp, bs, ELS, pieces, want, total, links_, prefill=prefill)
        assert r.rc == rc and pattern in r.err, r.err
        assert r.arena == r.before and r.launches == launches  # (at most the index's two launches, the plan and its scan)
        assert r.out_crcs == [0xDEADBEEF] * len(ELS)

    refused("a chain of 0 links", links_=0, launches=0)
    refused("2 links of %d members for %d members" % (M1, K * M1), links_=2, launches=2)
    refused("4 links of %d members for %d members" % (M1, K * M1), links_=4, launches=2)
    refused("%d links of %d members for %d members" % (K, M1 - 4, K * M1), pieces=[1, 4, 1], launches=2)
    refused("destination 2 has no pieces", pieces=[1, 5, 0], launches=0)
    # what plane_piece_count refuses, in link 1: the first and the last piece of plane 0 of tensor 1 exchanged
    f = M1 + 2
    cut = list(tab)
    cut[f], cut[f + 4] = tab[f + 4], tab[f]
    refused("the pieces of link 1's destination 1 are no multiple of 16 elements: member %d decodes to 5 bytes" % f, table=cut)
    # a link whose tensor has another plane size than in link 0
    other = [[(d[:-1], e) if j == 2 else (d, e) for j, (d, e) in enumerate(ln)] if k == 2 else ln for k, ln in enumerate(links)]
    blob2, tab2, _, _ = ch.chain_container(stream, other, table=True)
    refused("link 2 has planes of 99 bytes for destination 2, link 0 of 100", table=tab2, the_blob=blob2)
    # what the delta call refuses of destinations and bases
    refused("no destination 1 for its planes", sp=[spots[0], (None, spots[1][1]), spots[2]])
    refused("destinations 0 and 1 overlap", sp=[spots[0], (spots[0][0] + 2, spots[1][1]), spots[2]], bs=[base_offs[0], None, base_offs[2]])
    refused("the base of destination 0 wraps the address space", bs=[("abs", (1 << 64) - 16), base_offs[1], base_offs[2]])
    refused("the base of destination 0 overlaps destination 0 at another address", bs=[spots[0][0] + 2, base_offs[1], base_offs[2]])
    refused("the base of destination 1 overlaps destination 0", bs=[base_offs[0], spots[0][0] + spots[0][1] - 1, base_offs[2]])
    short = list(spots)
    short[1] = (spots[1][0], len(sts[0][1][0]) - 1)
    refused("destination 1 holds %d bytes, too small for %d" % (short[1][1], short[1][1] + 1), sp=short, rc=ENOMEM)


def test_damage_in_link_1_is_reported_as_the_delta_call_reports_it(lib, stream, run):
    """a flipped bit in the last tenth of link 1: the member named, or a digest mismatch of its tensor -- what ONE delta call over
    the same container, held to the digests of the single links, says of the same member or tensor"""
    sts, links = run
    blob, _, qs, per_link = ch.chain_container(stream, links)
    spots, base_offs, total = _places(sts[0])
    prefill = [(o, d) for o, (d, _) in zip(base_offs, sts[0])]
    want = cc.crcs_of(sts[K])
    link_crcs = [c for ln in links for c in cc.crcs_of(ln)]
    at, size = sum(len(s) for s in per_link[0]), sum(len(s) for s in per_link[1])
    kinds = set()
    for t in range(12):
        bad = cc.flip(blob, 8 * (at + size - size // 10) + 8 * (size // 10) * t // 12 + t % 8)
        r = ch.decode_chain(lib, bad, None, spots, base_offs, ELS, qs, want, total, K, prefill=prefill)
        one = _one_delta_call(lib, bad, None, K, link_crcs)
        assert r.rc in (0, EINVAL, EBADMSG) and one.rc == r.rc, (r.err, one.err)
        if r.rc == 0:  # (a bit no decoder reads: the digests have vouched for the bytes)
            assert r.out_crcs == want
        elif r.rc == EINVAL:
            assert "member " in r.err and r.err == one.err
            kinds.add("member")
        else:
            assert one.bad[0] == len(ELS) + r.bad[0] and "destination %d " % r.bad[0] in r.err  # link 1's tensor
            kinds.add("digest")
        assert all(r.arena[o:o + len(b)] == b for o, b in prefill)  # the bases, given out of place, are untouched
    print("kinds of error over twelve flips:", sorted(kinds))
    assert kinds, "no flip within twelve is seen at all: the set-up broke"


# ------------------------------------------------------------------------------------------------ the plan alone
def _check_plan(lib, dsts, caps, elems, pieces, links, out_len, base, stage):
    got = ch.plan(lib, dsts, caps, elems, pieces, links, out_len, base, stage)
    want = ch.np_plan(dsts, caps, elems, pieces, links, out_len, base, stage)
    for name in sorted(want):
        assert got[name] == want[name], name
    return got


def test_the_plan_counts_beyond_32_bits(lib):
    """size columns nobody decodes: S = 2^31 and Q = 3 make 2^32 + 5 elements to a plane, 8 bytes each, in each of two links; the
    offsets, the pitch, the units and the verdict are 64-bit sums of 32-bit sizes, and plane0 has an entry per link and tensor"""
    S = 1 << 31
    elems, pieces, links = [2, 8, 1, 4], [1, 3, 3, 2], 2
    one = [17, 17] + [S, S, 5] * 8 + [S, S, S] + [S, 16] * 4
    out_len = one * links
    count = [17, 2 * S + 5, 3 * S, S + 16]
    dsts = [0x7F00_0000_0010, 0x7E00_0000_0001, 0x7D00_0000_0008, 0x7C00_0000_0004]
    caps = [c * e for c, e in zip(count, elems)]
    stage = 0x1000_0000_0100
    got = _check_plan(lib, dsts, caps, elems, pieces, links, out_len, stage, stage)
    assert got["count"] == count and got["count"][1] > 1 << 32  # every destination is staged, the bytes too
    assert got["pitch"][1] == 2 * S + 16 and got["units"] == [(c + 15) // 16 for c in count]
    assert not got["status"] and got["bad"] == 4 and got["total_units"] == sum(got["units"])
    # plane0[k J + j]: every virtual destination's planes at a multiple of 16, one behind the other, inside plane_stage_bound
    bound = lib.emu_plane_stage_bound(ch.ctypes.c_uint64(sum(out_len)), ch.ctypes.c_uint64(len(out_len)))
    flat = [(got["plane0"][k * 4 + j], elems[j] * got["pitch"][j]) for k in range(links) for j in range(4)]
    assert all(p % 16 == 0 for p, _ in flat) and flat[0][0] >= stage and flat[-1][0] + flat[-1][1] <= stage + bound
    assert all(a + n <= b for (a, n), (b, _) in zip(flat, flat[1:]))
    # link 1's members lie where link 1's planes are, not link 0's
    assert (got["out_off"][len(one)] + stage) & MASK == got["plane0"][4]
    # one byte short of 8 x (2^32 + 5): the verdict needs all 64 bits too
    for short in (1, 3, 2):
        less = list(caps)
        less[short] -= 1
        got = _check_plan(lib, dsts, less, elems, pieces, links, out_len, 0, stage)
        assert got["status"] and got["bad"] == short and got["verdict"] == [j == short for j in range(4)]


def test_the_plan_of_the_run(lib, run):
    sts, links = run
    members = [len(m) for ln in links for m in ch.link_members(ln)[0]]
    dsts = [0x5000_0000 + 0x10_0000 * j + (j % 3) for j in range(len(ELS))]
    _check_plan(lib, dsts, [len(d) for d, _ in sts[0]], ELS, [1, 5, 1], K, members, 0x4000_0000, 0x4000_0000)
