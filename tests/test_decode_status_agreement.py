"""The five host drivers of the device decoder (orz_amd/csrc/orz_decode_drive.h lists them) name a damaged member in one and the
same way.  One container of three members -- a good one, the damaged member of _rangecases, a good one -- goes through all five
on the emulation backend, two members in flight: each fails with exactly `invalid orz data (member 1, status S)`, one S for
all, and leaves the good members' bytes where that driver leaves them; with the member's good stream in its place each decodes
to the input."""
import ctypes
import os
import re

import pytest

import _cachecases as cc
import _data
import _rangecases as rc
import _scattercases as sc
import test_decode_to_device_emu as whole

SLOTS = 2  # three members, two at a time: a second round over a state that is zeroed again
FILL = 0xA5
DRIVERS = ("decode_members_device", "decode_members_to_device", "decode_members_scatter", "reader", "reader with a cache")


class Case:
    """the container's parts: parts[k] = (what member k decodes to, its stream); `bad` = the damaged stream of member 1"""

    def __init__(self, oracle):
        data, good, self.bad = rc.damaged_text_member(oracle)
        a, b = _data.mixed(5_000, seed=21), _data.text(3_001, seed=22)
        self.parts = [(a, oracle.encode(a, 1)), (data, good), (b, oracle.encode(b, 0))]
        self.plain = [p for p, _ in self.parts]
        self.starts = rc.starts([len(p) for p in self.plain])
        self.total = sum(len(p) for p in self.plain)

    def blob(self, damaged):
        return self.parts[0][1] + (self.bad if damaged else self.parts[1][1]) + self.parts[2][1]


class Outcome:
    """err: the driver's message ('' when it succeeded); members: what lies where member k's bytes go (None: the driver hands
    nothing back after a failure); clean: nothing outside the members' places was written"""

    def __init__(self, err, members, clean=True):
        self.err, self.members, self.clean = err, members, clean


def _device(case, blob):
    lib = ctypes.CDLL(os.path.join(rc.ROOT, "build", "libemu.so"))
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n, m = ctypes.c_size_t(), ctypes.c_size_t()
    err = ctypes.create_string_buffer(256)
    if lib.emu_decode_members(blob, ctypes.c_size_t(len(blob)), SLOTS, ctypes.byref(dst), ctypes.byref(n), ctypes.byref(m), err, ctypes.c_size_t(256)):
        return Outcome(err.value.decode(), None)
    out = ctypes.string_at(dst, n.value)
    lib.emu_free(dst)
    assert m.value == 3 and len(out) == case.total
    return Outcome("", [out[s:s + len(p)] for s, p in zip(case.starts, case.plain)])


def _to_device(case, blob):
    r = whole.decode(rc.whole_lib(), blob, cap=case.total + 16, slots=SLOTS, fill=FILL)
    assert r.launches == 2 and r.members == 3 and r.dst_len == case.total
    return Outcome(r.err, [r.buf[s:s + len(p)] for s, p in zip(case.starts, case.plain)], r.canary_ok and r.buf[case.total:] == bytes([FILL]) * 16)


def _scatter(case, blob):
    caps = [len(p) + 9 for p in case.plain]
    offs, total = sc.reverse_layout(caps)
    r = sc.scatter(sc.emu_lib(), blob, None, list(zip(offs, caps)), total, slots=SLOTS, fill=FILL)
    assert r.launches == 2 and r.members == 3 and r.out_lens == [len(p) for p in case.plain]
    members = [r.arena[o:o + len(p)] for o, p in zip(offs, case.plain)]
    expect = bytearray(bytes([FILL]) * total)  # (guards, and the room behind each member in its destination)
    arena = bytearray(r.arena)
    for o, p in zip(offs, case.plain):
        arena[o:o + len(p)] = expect[o:o + len(p)]
    return Outcome(r.err, members, arena == expect)


def _reader(case, blob, budget=None):
    rd = cc.CachedEmuReader(cc.emu_lib(), blob) if budget else rc.EmuReader(rc.emu_lib(), blob)
    assert rd.h, rd.err
    try:
        if budget:
            rd.set_cache(budget)
        r = rd.read([(0, case.total)], cap=case.total + 16, slots=SLOTS, fill=FILL)
        assert r.launches == 2 and r.members_decoded == 3 and r.dst_len == case.total
        if budget:  # every member got a cursor; the one whose decode failed lost it
            st = rd.cache_stats()
            assert (st["fresh"], st["uncached"], st["cursors"]) == (3, 0, 3 if r.rc == 0 else 2), st
        return Outcome(r.err, [r.buf[s:s + len(p)] for s, p in zip(case.starts, case.plain)], r.canary_ok and r.buf[case.total:] == bytes([FILL]) * 16)
    finally:
        rd.close()


def _reader_cached(case, blob):
    return _reader(case, blob, budget=sum(cc.cost(len(p), cc.emu_lib().emu_reader_cursor_state_bytes()) for p in case.plain))


RUN = dict(zip(DRIVERS, (_device, _to_device, _scatter, _reader, _reader_cached)))


@pytest.fixture(scope="module")
def case(oracle):
    return Case(oracle)


@pytest.fixture(scope="module")
def outcomes(emu, case):
    """every driver on the emulation, once: {driver: (outcome on the damaged container, outcome on the good one)}"""
    return {name: (RUN[name](case, case.blob(True)), RUN[name](case, case.blob(False))) for name in DRIVERS}


def test_the_case_is_what_it_claims(case):
    assert len(case.plain[1]) >= 1_000_000 and all(3_000 <= len(case.plain[k]) <= 9_000 for k in (0, 2))
    assert len(case.bad) == len(case.parts[1][1]) and case.bad != case.parts[1][1]


def test_every_driver_names_the_damaged_member_alike(outcomes):
    texts = {name: bad.err for name, (bad, _) in outcomes.items()}
    first = texts[DRIVERS[0]]
    assert re.fullmatch(r"invalid orz data \(member 1, status [0-9]+\)", first), first
    assert all(t == first for t in texts.values()), texts


@pytest.mark.parametrize("name", DRIVERS)
def test_the_good_members_of_the_damaged_container(outcomes, case, name):
    bad = outcomes[name][0]
    if name == "decode_members_device":  # (its output is a host buffer it makes on success only)
        assert bad.members is None
        return
    assert bad.members[0] == case.plain[0] and bad.members[2] == case.plain[2] and bad.clean
    if name.startswith("reader"):  # the gather skips the pieces of a member whose decode failed
        assert bad.members[1] == bytes([FILL]) * len(case.plain[1])


@pytest.mark.parametrize("name", DRIVERS)
def test_the_good_container_decodes_to_the_input(outcomes, case, name):
    good = outcomes[name][1]
    assert good.err == "" and good.members == case.plain and good.clean
