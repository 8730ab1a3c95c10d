"""CPU tier: the repair passes of the fast parse on the emulation backend, pass by pass, held to the serial replay of
tests/_repaircases.py -- exactly: the decisions, previous-item types and item-start flags at every position, the source of every
match, the `edge` flags of the sources a pass assigns, the per-context growth counters and `cok` flags, the lists' entry counts and
the control block after every pass; the committed arrays after the last; and the stream decodes with the oracle.  Natural cases
(few rounds, so that the passes have work) and injected decision fields that reach the lists' capacities, the round-3 shape, recuts
with WORD items and clamped matches, the two sides of the ring's end and of the edge margin.  The forms of the stage (lists, grid,
full passes, no source cap) each run in a child process (their knobs are read once per process)."""
import functools

import numpy as np
import pytest

import _oracle
import _repaircases as rc

_REPLAYS = {}


def held_to_replay(data, k, probe, trace, out, level=1, cap=None):
    B = rc.Block(data, k, trace)
    b = probe["before"]
    key = (bytes(data), k, b["ty"].tobytes(), b["nl"].tobytes(), cap)
    if key not in _REPLAYS:
        _REPLAYS[key] = rc.replay(B, b["ty"], b["nl"], b["pt"], b["sbits"], K=probe["K"], cap=rc.src_cap(probe["depth"]) if cap is None else cap)
    passes = _REPLAYS[key]
    assert probe["depth"] == rc.DEPTH[level]
    bad = rc.compare(probe, B, passes, lt0=rc.last_type_before(trace, k))
    assert not bad, "\n".join(bad)
    back, used = _oracle.decode(out)
    assert back == bytes(data) and used == len(out), "the oracle's decoder does not reproduce the input"
    return passes


NATURAL = [(name, rounds, 1) for name in sorted(rc.natural_inputs()) if name != "noise_65537" for rounds in (1, 2)] + \
    [("noise_65537", 1, 1), ("mixed_12305", 2, 0), ("mixed_12305", 2, 2)]


@functools.lru_cache(maxsize=None)
def natural_run(name, rounds, level):
    """the replay of a natural case, held to the emulation's probe"""
    data = rc.natural_inputs()[name]
    plain, _, _ = rc.emu_encode(data, None, level=level, tile=rc.COARSE["tile"], rounds=rounds)
    out, probe, trace = rc.emu_encode(data, 0, level=level, tile=rc.COARSE["tile"], rounds=rounds)
    assert out == plain, "an armed probe changed the stream"
    return held_to_replay(data, 0, probe, trace, out, level=level)


@pytest.mark.parametrize("name,rounds,level", NATURAL)
def test_natural_passes_equal_the_replay(name, rounds, level):
    natural_run(name, rounds, level)


def test_the_natural_cases_give_the_passes_work():
    """asserted on the replays alone, case by case.  Hundreds of repairs in one block: the WORD fixes of zeros with noise after one
    round (tiles are 4096 positions at these sizes whatever the mode asks for, so text and "mixed" need about a hundred at two
    rounds, cuts and fixes over four passes; the 1 MiB unit of the next test needs two thousand, half of them cuts)"""
    noise = [r for _, _, r in natural_run("noise_65537", 1, 1)]
    assert sum(r["nfix"] for r in noise) >= 1000 and len(noise) >= 3
    for name in ("mixed_65537", "text_65537"):
        reps = [r for _, _, r in natural_run(name, 2, 1)]
        assert len(reps) >= 4 and sum(r["ncut"] for r in reps) >= 20 and sum(r["clamped"] for r in reps) >= 1, name
    mixed = [r for _, _, r in natural_run("mixed_65537", 2, 1)]
    assert sum(r["chg"] for r in mixed) >= 100 and sum(r["far_found"] for r in mixed) >= 10 and sum(r["recut_words"] for r in mixed) >= 5


def test_a_unit_behind_a_history_equals_the_replay(monkeypatch):
    """the second 1 MiB unit of a text: sources and the ring reach into the history, words[] starts from the first unit's"""
    import corpus

    monkeypatch.setenv("ORZ_FAST_UNIT", str(1 << 20))
    data = corpus.enwik_like(2 << 20)
    out, probe, trace = rc.emu_encode(data, 1, level=1, **rc.COARSE)
    assert probe["n"] == 1 << 20 and probe["block"] == 1
    passes = held_to_replay(data, 1, probe, trace, out)
    assert sum(r["ncut"] for _, _, r in passes) >= 500 and sum(r["nfix"] for _, _, r in passes) >= 500, "not hundreds of cuts and of fixes"
    assert sum(r["ring_stops"] for _, _, r in passes) >= 100 and sum(r["cap_stops"] for _, _, r in passes) >= 10
    B = rc.Block(data, 1, trace)
    m = np.nonzero((passes[-1][0].s[:B.n] == 1) & (passes[-1][0].ty[:B.n] == rc.MATCH))[0]
    assert (passes[-1][1][m] < rc.KPRE).sum() >= 1000, "few sources in the history"


@pytest.mark.parametrize("name", sorted(rc.injected()))
def test_injected_fields_equal_the_replay(name):
    c = rc.injected()[name]
    passes = c.passes()
    c.reached(passes)                                # (on the replay alone: the case reaches its edge)
    out, probe, trace = rc.emu_encode(c.data, 0, ty=c.ty, nl=c.nl)
    bad = rc.compare(probe, c.block(), passes)
    assert not bad, "\n".join(bad)
    back, used = _oracle.decode(out)
    assert back == c.data and used == len(out)


def test_a_field_that_breaks_the_contract_is_refused():
    data = rc.natural_inputs()["text_4096"]
    n = len(data)
    ty, nl = rc._literals(n)
    for at, t, l in ((5, 3, 1), (5, rc.LIT, 2), (5, rc.WORD, 1), (5, rc.MATCH, 3), (5, rc.MATCH, 241), (n - 1, rc.WORD, 2), (n - 100, rc.MATCH, 101)):
        bt, bl = ty.copy(), nl.copy()
        bt[at] = t
        bl[at] = l
        with pytest.raises(rc.FieldRefused):
            rc.emu_encode(data, 0, ty=bt, nl=bl)
    plain, _, _ = rc.emu_encode(data, None)
    with pytest.raises(rc.FieldRefused, match="size"):
        rc.emu_encode(data, 0, ty=ty[:-1], nl=nl[:-1])     # (not the armed block's size: refused when the encode reaches the block)
    assert rc.emu_encode(data, None)[0] == plain           # ... and the encoder is as it was
    ty[7] = rc.MATCH
    nl[7] = 0                                              # undecided: read as a literal
    out, probe, _ = rc.emu_encode(data, 0, ty=ty, nl=nl)
    assert probe["before"]["ty"][7] == rc.LIT and probe["before"]["nl"][7] == 1
    assert _oracle.decode(out)[0] == data


@pytest.fixture(scope="module")
def forms():
    return {f: rc.run_form("emu", f) for f in rc.FORMS}


def test_the_forms_write_one_stream_and_leave_one_state(forms):
    """lists (default), grids over all positions, and full passes (no incremental shortcut): the same stream, the same state after
    every pass, the same committed arrays"""
    rc.forms_agree(forms)


@pytest.mark.parametrize("name", [n for n, _ in rc.FORM_INPUTS])
@pytest.mark.parametrize("form,cap", [("default", None), ("grid", None), ("fullpass", None), ("nocap", 0)])
def test_every_form_equals_the_replay(forms, form, cap, name):
    data = rc.natural_inputs()[name]
    out, probe = forms[form][name]
    held_to_replay(data, 0, probe, rc.NO_TRACE, out, cap=cap)
