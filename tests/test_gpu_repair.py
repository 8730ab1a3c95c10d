"""GPU tier: the repair passes of the fast parse as the PRODUCT library runs them on the device (read through
orz_stream_arm_repair_probe / orz_stream_repair_probe), pass by pass, held exactly to the serial replay of tests/_repaircases.py --
not to the emulation: decisions, previous-item types and item-start flags at every position, every match's source, the `edge`
flags, the per-context counters and `cok`, the lists' entry counts, the control block after every pass, the committed arrays; the
stream decodes with the oracle.  The injected decision fields are those the CPU tier runs on the emulation.  The forms of the stage
each run in a child process.  One process, one encoder at a time; every device step under a time limit that ends the process."""
import numpy as np
import pytest

import _oracle
import _repaircases as rc
from _stepcases import limit

pytestmark = pytest.mark.gpu

_REPLAYS = {}


@pytest.fixture(scope="module")
def gpu():
    from orz_amd import _native

    if _native.load().orz_device_count() <= 0:
        pytest.fail("GPU test selected but liborz_hip.so found no HIP device (no CPU fallback exists)")
    import orz_amd

    return orz_amd


def gpu_encode(gpu, data, k, level=1, tile=0, rounds=0, ty=None, nl=None, plain=False):
    """(stream, probe, trace[, stream of an unarmed encode before it]) of an encoder of its own"""
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=level)
    try:
        assert enc.config()["mode"] == 1
        if tile or rounds:
            with limit(300):
                enc.set_mode("fast", tile, rounds)
        before = None
        if plain:
            with limit(120):
                before = enc.encode(data)
        enc.set_item_trace(True)
        enc.arm_repair_probe(k, ty, nl)
        with limit(120):
            out = enc.encode(data)
        probe = rc.probe_tables(enc.repair_probe)
        trace = rc.gpu_trace(enc.item_trace())
        if plain:
            with limit(120):
                again = enc.encode(data)     # the probe was for one encode
            assert again == before
    finally:
        enc.close()
    return (out, probe, trace, before) if plain else (out, probe, trace)


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
_RUNS = {}


def natural_run(gpu, name, rounds, level):
    """the replay of a natural case, held to the device's probe (once per case)"""
    if (name, rounds, level) not in _RUNS:
        data = rc.natural_inputs()[name]
        out, probe, trace, plain = gpu_encode(gpu, data, 0, level=level, tile=rc.COARSE["tile"], rounds=rounds, plain=True)
        assert out == plain, "an armed probe changed the stream"
        _RUNS[(name, rounds, level)] = held_to_replay(data, 0, probe, trace, out, level=level)
    return _RUNS[(name, rounds, level)]


@pytest.mark.parametrize("name,rounds,level", NATURAL)
def test_natural_passes_equal_the_replay(gpu, name, rounds, level):
    natural_run(gpu, name, rounds, level)


def test_the_natural_cases_give_the_passes_work(gpu):
    """asserted on the replays alone, case by case (tests/test_repair_emu.py says why text and "mixed" need about a hundred repairs)"""
    noise = [r for _, _, r in natural_run(gpu, "noise_65537", 1, 1)]
    assert sum(r["nfix"] for r in noise) >= 1000 and len(noise) >= 3
    for name in ("mixed_65537", "text_65537"):
        reps = [r for _, _, r in natural_run(gpu, name, 2, 1)]
        assert len(reps) >= 4 and sum(r["ncut"] for r in reps) >= 20 and sum(r["clamped"] for r in reps) >= 1, name
    mixed = [r for _, _, r in natural_run(gpu, "mixed_65537", 2, 1)]
    assert sum(r["chg"] for r in mixed) >= 100 and sum(r["far_found"] for r in mixed) >= 10 and sum(r["recut_words"] for r in mixed) >= 5


def test_a_unit_behind_a_history_equals_the_replay(gpu, monkeypatch):
    """the second 1 MiB unit of a text: sources and the ring reach into the history; a full unit, so the unarmed encode replays its
    rounds and passes as a captured graph and the armed one runs them launch by launch -- the same stream"""
    import corpus

    monkeypatch.setenv("ORZ_FAST_UNIT", str(1 << 20))
    data = corpus.enwik_like(2 << 20)
    out, probe, trace, plain = gpu_encode(gpu, data, 1, level=1, plain=True, **rc.COARSE)
    assert out == plain, "an armed probe changed the stream"
    assert probe["n"] == 1 << 20 and probe["block"] == 1
    passes = held_to_replay(data, 1, probe, trace, out)
    assert sum(r["ncut"] for _, _, r in passes) >= 500 and sum(r["nfix"] for _, _, r in passes) >= 500, "not hundreds of cuts and of fixes"
    assert sum(r["ring_stops"] for _, _, r in passes) >= 100 and sum(r["cap_stops"] for _, _, r in passes) >= 10


@pytest.mark.parametrize("name", sorted(rc.injected()))
def test_injected_fields_equal_the_replay(gpu, name):
    c = rc.injected()[name]
    passes = c.passes()
    c.reached(passes)
    out, probe, trace = gpu_encode(gpu, c.data, 0, ty=c.ty, nl=c.nl)
    bad = rc.compare(probe, c.block(), passes)
    assert not bad, "\n".join(bad)
    back, used = _oracle.decode(out)
    assert back == c.data and used == len(out)


@pytest.fixture(scope="module")
def forms(gpu):
    return {f: rc.run_form("gpu", f) for f in rc.FORMS}


def test_the_forms_write_one_stream_and_leave_one_state(forms):
    rc.forms_agree(forms)


@pytest.mark.parametrize("name", [n for n, _ in rc.FORM_INPUTS])
@pytest.mark.parametrize("form,cap", [("default", None), ("grid", None), ("fullpass", None), ("nocap", 0)])
def test_every_form_equals_the_replay(forms, form, cap, name):
    data = rc.natural_inputs()[name]
    out, probe = forms[form][name]
    held_to_replay(data, 0, probe, rc.NO_TRACE, out, cap=cap)


def test_refusals(gpu):
    data = rc.natural_inputs()["text_4096"]
    n = len(data)
    ty, nl = rc._literals(n)
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=1, mode="exact")
    try:
        with pytest.raises(gpu.OrzError):
            enc.arm_repair_probe(0)                  # the exact mode has no repair stage
        with limit(300):
            enc.set_mode("fast")
        with pytest.raises(gpu.OrzError):
            enc.repair_probe("scalars")              # nothing probed yet
        with pytest.raises(gpu.OrzError):
            enc.arm_repair_probe(70000)
        for at, t, l in ((5, 3, 1), (5, rc.LIT, 2), (5, rc.WORD, 1), (5, rc.MATCH, 3), (5, rc.MATCH, 241), (n - 1, rc.WORD, 2), (n - 100, rc.MATCH, 101)):
            bt, bl = ty.copy(), nl.copy()
            bt[at] = t
            bl[at] = l
            with pytest.raises(gpu.OrzError):
                enc.arm_repair_probe(0, bt, bl)
        lib = enc._lib
        assert lib.orz_stream_arm_repair_probe(None, 0, None, None, 0) == -22
        assert lib.orz_stream_arm_repair_probe(enc._h, 0, ty.ctypes.data, None, n) == -22
        assert lib.orz_stream_repair_probe(enc._h, b"no_such_table", None, 0) == -22
        with limit(120):
            plain = enc.encode(data)                 # (a refused arming leaves the encoder unarmed)
        with pytest.raises(gpu.OrzError):
            enc.repair_probe("scalars")
        enc.arm_repair_probe(0, ty[:-1], nl[:-1])    # not the armed block's size: refused when the encode reaches the block,
        with limit(120):
            with pytest.raises(gpu.OrzError, match="size"):
                enc.encode(data)
        with limit(120):
            assert enc.encode(data) == plain         # ... the encoder is as it was, the probe disarmed
        enc.arm_repair_probe(0, ty, nl)
        with limit(120):
            out = enc.encode(data)                   # (a field of literals: nothing to repair)
        probe = rc.probe_tables(enc.repair_probe)
        assert len(probe["passes"]) == 1 and probe["final"]["items"] == n and _oracle.decode(out)[0] == data
    finally:
        enc.close()
