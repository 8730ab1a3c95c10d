"""Members decoded each into a destination of its own (orz_amd/csrc/orz_decode_scatter.h) on the emulation backend: ScatterPlan
and ScatterVerdict against a restatement in plain Python, the driver's bytes against the host decoder's inside a poisoned arena
with guard gaps, and every refusal made before a byte of any destination is written."""
import os
import random

import pytest

import _scattercases as sc
from _scattercases import EINVAL, ENOMEM, GUARD, OK, SHORT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mixed30k", "text20k", "zeros20k")


@pytest.fixture(scope="module")
def lib():
    return sc.emu_lib()


def _golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name), "rb").read()


@pytest.fixture(scope="module")
def members(oracle):
    """(what each member decodes to by the host decoder, the members' streams): the three golden streams and an empty member"""
    blobs = [_golden(n + ".l1.orz") for n in NAMES] + [oracle.encode(b"", 1)]
    parts = [oracle.decode(b)[0] for b in blobs]
    assert parts[:3] == [_golden(n + ".in") for n in NAMES] and parts[3] == b""
    return parts, blobs


def _table(blobs, order=None, gap=7):
    """the members in one buffer in `order` with gaps of garbage: (buffer, [(offset, length)] in member order)"""
    order = list(range(len(blobs))) if order is None else order
    buf, table = bytearray(b"\xff" * 3), [None] * len(blobs)
    for k in order:
        table[k] = (len(buf), len(blobs[k]))
        buf += blobs[k] + b"\x07" * gap
    return bytes(buf), table


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_plan_equals_its_restatement(lib, n):
    rng = random.Random(n)
    base = 0x7F00_0000_1000
    for case in ("in order", "permuted"):
        # destinations below and above `base`: the offsets wrap modulo 2^64 for those below
        dsts = [base + (k - n // 2) * 4096 + rng.randrange(16) for k in range(n)]
        if case == "permuted":
            rng.shuffle(dsts)
        out_len = [rng.choice([0, 1, 4095, 4096, rng.randrange(1 << 32)]) for _ in range(n)]
        caps = list(out_len)
        assert sc.plan_emulated(lib, dsts, caps, out_len, base) == sc.plan_reference(dsts, caps, out_len, base)
        off, verdict, rec = sc.plan_emulated(lib, dsts, caps, out_len, base)
        assert rec == (n, n, OK) and all((base + o) & sc.MASK == d for o, d in zip(off, dsts))
        if n > 1:
            assert any(d < base for d in dsts) and any(o >> 63 for o in off)
        # one short destination at each edge of the ballot, then several: the FIRST is named
        for bad in sorted({0, n - 1, min(63, n - 1), min(64, n - 1), n // 2}):
            c = list(caps)
            out_len_b = list(out_len)
            out_len_b[bad] = max(out_len_b[bad], 1)
            c[bad] = out_len_b[bad] - 1
            got = sc.plan_emulated(lib, dsts, c, out_len_b, base)
            assert got == sc.plan_reference(dsts, c, out_len_b, base)
            assert got[2] == (n, bad, SHORT)
            c[n - 1] = 0
            out_len_b[n - 1] = max(out_len_b[n - 1], 1)
            assert sc.plan_emulated(lib, dsts, c, out_len_b, base)[2] == (n, bad, SHORT)
    # capacity above the size, and a member of no bytes in a destination of none, are never short
    assert sc.plan_emulated(lib, [base] * n, [5] * n, [4] * n, base)[2] == (n, n, OK)
    assert sc.plan_emulated(lib, [0] * n, [0] * n, [0] * n, base)[2] == (n, n, OK)


# ------------------------------------------------------------------------------------------------ the driver
@pytest.mark.parametrize("layout", ["table", "permuted table", "concatenation", "host container"])
def test_members_land_in_their_own_destinations(lib, members, layout):
    parts, blobs = members
    if layout in ("table", "permuted table"):
        blob, table = _table(blobs, order=[2, 0, 3, 1] if layout == "permuted table" else None)
    else:
        blob, table = b"".join(blobs), None
    caps = [len(p) + 9 for p in parts[:3]] + [0]  # (room behind each member: it must stay poison; the empty member gets none)
    offs, total = sc.reverse_layout(caps)
    assert offs == sorted(offs, reverse=True)
    r = sc.scatter(lib, blob, table, list(zip(offs, caps)), total, on_device=layout != "host container")
    assert r.rc == 0, r.err
    assert r.members == 4 and r.out_lens == [len(p) for p in parts]
    sc.check_arena(r.arena, offs, caps, parts)
    # a constant number of host waits: index record, destinations, plan record, statuses; the table's and the container's uploads
    assert r.host_waits == 4 + (table is not None) + (layout == "host container")
    assert r.launches == 1
    # the output does not depend on what the buffers held
    z = sc.scatter(lib, blob, table, list(zip(offs, caps)), total, fill=0x00)
    sc.check_arena(z.arena, offs, caps, parts, fill=0x00)


def test_members_in_permuted_member_order(lib, members):
    """the table lists the members in another order: destination k takes member k of THAT order"""
    parts, blobs = members
    blob, table = _table(blobs)
    perm = [3, 1, 0, 2]
    caps = [len(parts[k]) for k in perm]
    offs, total = sc.reverse_layout(caps)
    r = sc.scatter(lib, blob, [table[k] for k in perm], list(zip(offs, caps)), total, slots=3)
    assert r.rc == 0, r.err
    assert r.out_lens == caps and r.launches == 2  # (four members, three at a time)
    sc.check_arena(r.arena, offs, caps, [parts[k] for k in perm])


def test_host_waits_do_not_grow_with_the_members(lib, oracle):
    small = [bytes([65 + k % 26]) * (k % 5) for k in range(130)]
    blobs = [oracle.encode(p, 1) for p in small]
    blob, table = _table(blobs, gap=1)
    caps = [len(p) for p in small]
    offs, total = sc.reverse_layout(caps, guard=3)
    r = sc.scatter(lib, blob, table, [(o if c else None, c) for o, c in zip(offs, caps)], total)
    assert r.rc == 0, r.err
    assert r.host_waits == 5 and r.out_lens == caps
    sc.check_arena(r.arena, offs, caps, small)


def test_a_destination_one_byte_short_writes_nothing(lib, members):
    parts, blobs = members
    blob, table = _table(blobs)
    for short in (0, 2):
        caps = [len(p) for p in parts]
        caps[short] -= 1
        offs, total = sc.reverse_layout(caps)
        r = sc.scatter(lib, blob, table, list(zip(offs, caps)), total)
        assert r.rc == ENOMEM and r.launches == 0
        assert "member %d " % short in r.err, r.err
        assert r.arena == bytes([sc.POISON]) * total
        assert r.out_lens == [len(p) for p in parts]  # (the sizes come back with the refusal)
    caps = [len(p) - 1 for p in parts[:3]] + [0]
    offs, total = sc.reverse_layout(caps)
    r = sc.scatter(lib, blob, table, list(zip(offs, caps)), total)
    assert r.rc == ENOMEM and "member 0 " in r.err and r.arena == bytes([sc.POISON]) * total  # the FIRST short one is named


def test_overlapping_destinations_are_refused(lib, members):
    parts, blobs = members
    blob, table = _table(blobs)
    caps = [len(p) for p in parts]
    offs, total = sc.reverse_layout(caps)
    for a, b, shift in ((0, 1, 1), (2, 1, -1), (0, 2, 0)):
        o = list(offs)
        o[a] = offs[b] + caps[b] - shift if shift > 0 else (offs[b] - caps[a] + 1 if shift < 0 else offs[b])
        r = sc.scatter(lib, blob, table, list(zip(o, caps)), total + max(caps))
        assert r.rc == EINVAL and "overlap" in r.err and r.launches == 0, (a, b, r.err)
        assert r.arena == bytes([sc.POISON]) * (total + max(caps))
    # the empty member's destination may lie anywhere, inside another included
    o = list(offs)
    o[3] = offs[0] + 5
    r = sc.scatter(lib, blob, table, list(zip(o, caps)), total)
    assert r.rc == 0, r.err
    sc.check_arena(r.arena, offs, caps, parts)
    # touching destinations do not overlap
    caps2 = [len(p) for p in parts]
    offs2, total2 = sc.reverse_layout(caps2, guard=0)
    r = sc.scatter(lib, blob, table, list(zip(offs2, caps2)), total2)
    assert r.rc == 0, r.err
    sc.check_arena(r.arena, offs2, caps2, parts)


def test_wrong_count_and_null_destinations_are_refused(lib, members):
    parts, blobs = members
    blob, table = _table(blobs)
    caps = [len(p) for p in parts]
    offs, total = sc.reverse_layout(caps)
    places = list(zip(offs, caps))
    for use_table in (True, False):
        b, t = (blob, table) if use_table else (b"".join(blobs), None)
        for nd in (3, 5):
            r = sc.scatter(lib, b, t, places + [(0, 0)], total, n_dsts=nd)
            assert r.rc == EINVAL and "destinations for 4 members" in r.err and r.launches == 0, r.err
            assert r.arena == bytes([sc.POISON]) * total
    null = list(places)
    null[1] = (None, caps[1])
    r = sc.scatter(lib, blob, table, null, total)
    assert r.rc == EINVAL and "member 1" in r.err and r.launches == 0 and r.arena == bytes([sc.POISON]) * total
    null = list(places)
    null[3] = (None, 0)  # a member of no bytes needs no destination
    r = sc.scatter(lib, blob, table, null, total)
    assert r.rc == 0, r.err


def test_a_destination_inside_the_container_is_refused(lib, members):
    parts, blobs = members
    blob, table = _table(blobs)
    caps = [len(p) for p in parts]
    offs, total = sc.reverse_layout(caps)
    src_at = total + max(caps)  # the container lies in the arena behind the destinations, free room in front of it
    for o1 in (src_at + 10, src_at - caps[1] + 1, src_at + len(blob) - 1):
        o = list(offs)
        o[1] = o1
        r = sc.scatter(lib, blob, table, list(zip(o, caps)), src_at + len(blob) + max(caps), src_at=src_at)
        assert r.rc == EINVAL and "container" in r.err and "member 1" in r.err and r.launches == 0, r.err
        assert r.arena[:total] == bytes([sc.POISON]) * total and r.arena[src_at:src_at + len(blob)] == blob
    r = sc.scatter(lib, blob, table, list(zip(offs, caps)), src_at + len(blob) + GUARD, src_at=src_at)  # next to it is fine
    assert r.rc == 0, r.err
    sc.check_arena(r.arena[:total], offs, caps, parts)


def test_a_damaged_member_is_named(lib, members):
    parts, blobs = members
    bad = bytearray(blobs[1])
    rng = random.Random(4)
    for _ in range(40):  # payload bits in the last tenth of the stream, in front of its EOF byte: the framing stays whole
        bad[len(bad) - 6 - rng.randrange(len(bad) // 10)] ^= 1 << rng.randrange(8)
    damaged = [blobs[0], bytes(bad), blobs[2], blobs[3]]
    blob, table = _table(damaged)
    caps = [len(p) + 300 for p in parts]
    offs, total = sc.reverse_layout(caps)
    r = sc.scatter(lib, blob, table, list(zip(offs, caps)), total)
    assert r.rc == EINVAL and "(member 1," in r.err, r.err
    # framing damage is found by the index, before any launch
    blob, table = _table([blobs[0], blobs[1], blobs[2][:-1], blobs[3]])  # (member 2 without its EOF byte)
    r = sc.scatter(lib, blob, table, list(zip(offs, caps)), total)
    assert r.rc == EINVAL and "(member 2)" in r.err and r.launches == 0 and r.arena == bytes([sc.POISON]) * total


def test_sizing_call_decodes_nothing(lib, members):
    parts, blobs = members
    blob, table = _table(blobs)
    for b, t in ((blob, table), (b"".join(blobs), None)):
        r = sc.scatter(lib, b, t, [(None, 0)] * 4, 16, sizing=True)
        assert r.rc == 0 and r.members == 4 and r.out_lens == [len(p) for p in parts] and r.launches == 0
        assert r.arena == bytes([sc.POISON]) * 16
        r = sc.scatter(lib, b, t, [(None, 0)] * 2, 16, sizing=True)  # (a shorter array takes the first sizes)
        assert r.rc == 0 and r.members == 4 and r.out_lens == [len(p) for p in parts[:2]]
    e = sc.scatter(lib, b"", None, [], 16, sizing=True)
    assert e.rc == 0 and e.members == 0
    e = sc.scatter(lib, b"", None, [], 16)
    assert e.rc == 0 and e.members == 0 and e.launches == 0
