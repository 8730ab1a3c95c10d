"""GPU tier: the static per-block tables of the fast parse as the PRODUCT library's prep kernels build them on the device
(FastSlotInitWave, FastRowsWave, FastKw, FastWordMasks, HistCountWave, the column scan; read through orz_stream_fast_tables), held
entry for entry to the numpy references of tests/_fasttables.py -- not to the emulation -- on the inputs of that module; at -l0,
-l1 and -l2 for one of them (K and the tables do not depend on the level today: the test says so by passing), and on one
17 MiB input whose captured unit has the whole window as history.  An armed capture
changes no byte of the stream, and an unarmed encoder writes the streams recorded before the capture existed.
One process, one encoder at a time; every step on the GPU runs under a time limit of its own that ends the process."""
import contextlib
import faulthandler
import hashlib
import json
import os

import numpy as np
import pytest

import _data
import _fasttables as ft

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@contextlib.contextmanager
def limit(seconds):
    """a step that is still running after `seconds` ends the whole process (a hung device call cannot be interrupted from Python)"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gpu():
    from orz_amd import _native

    if _native.load().orz_device_count() <= 0:
        pytest.fail("GPU test selected but liborz_hip.so found no HIP device (no CPU fallback exists)")
    import orz_amd

    return orz_amd


@pytest.fixture(autouse=True)
def _one_mib_units(monkeypatch):
    monkeypatch.setenv("ORZ_FAST_UNIT", str(ft.UNIT))


def gpu_capture(gpu, data, k, level=1):
    """(stream, captured tables, items of the units before unit k) of one armed encode"""
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=level)  # (the library's default mode is the fast one)
    try:
        assert enc.config()["mode"] == 1
        enc.set_item_trace(True)
        enc.arm_fast_tables(k)
        with limit(300):
            out = enc.encode(data)
        cap = enc.fast_tables()
        it = enc.item_trace()
    finally:
        enc.close()
    trace = {"block": it["block"], "pos": it["pos"], "word": it["symbol"] == 388,
             "mlen": np.where(it["after_literal"] & 2, it["match_len"], 0)}
    return out, cap, trace


_DISTANCES = {}   # input -> the distances behind its reference's distance codes (the coverage test at the end reads them)


def held_to_reference(data, k, cap, trace, name=None):
    hpos, wsnap = ft.history_from_trace(data, k, trace)
    assert cap["n"] == ft.unit_sizes(len(data))[k] and cap["block"] == k and cap["new_at"] == ft.KPRE
    assert np.array_equal(cap["hpos"], hpos), "history item starts differ from the trace of the earlier units"
    assert np.array_equal(cap["wsnap"], wsnap), "words[] at the block start differs from the replay of the traced items"
    ref = ft.reference(data, k, hpos, wsnap)
    if name:
        _DISTANCES[name] = ft.sampled_distances(ref)
    bad = ft.compare(cap, ref)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", sorted(ft.inputs()))
def test_device_tables_equal_their_definitions(gpu, name):
    data, k = ft.inputs()[name]
    _, cap, trace = gpu_capture(gpu, data, k)
    held_to_reference(data, k, cap, trace, name)


def test_device_tables_behind_a_full_window(gpu):
    """the first unit of a second block: 16 MiB of history, tail keys from a block boundary, distances up to 2^24 + 1"""
    data, k = ft.gpu_inputs()["far"]
    _, cap, trace = gpu_capture(gpu, data, k)
    assert cap["stream_off"] == ft.BLOCK and cap["n"] == ft.UNIT + 64 * 1024
    held_to_reference(data, k, cap, trace, "far")


def test_the_references_hold_both_sides_of_every_rounding_step_up_to_2_24(gpu):
    """asserted on the references alone: over the inputs of this tier the distance codes stand for a distance v and a distance
    v + 1 for every code value v of dist_code_up from 16 to 2^24"""
    todo = dict(ft.inputs())
    todo.update(ft.gpu_inputs())
    for name, (data, k) in todo.items():
        if name not in _DISTANCES:
            _, cap, trace = gpu_capture(gpu, data, k)
            hpos, wsnap = ft.history_from_trace(data, k, trace)
            _DISTANCES[name] = ft.sampled_distances(ft.reference(data, k, hpos, wsnap))
    have = set().union(*_DISTANCES.values())
    missing = ft.dist_gaps(have, 1 << 24)
    assert not missing, "no sampled distances v and v + 1 for the code values %s" % missing


@pytest.mark.parametrize("level", [0, 2])
def test_device_tables_at_the_other_levels(gpu, level):
    """(-l1 is the parametrised test above)"""
    data, k = ft.inputs()["planted"]
    _, cap, trace = gpu_capture(gpu, data, k, level=level)
    assert cap["K"] == ft.K
    held_to_reference(data, k, cap, trace)


def test_an_armed_capture_changes_no_byte_of_the_stream(gpu):
    data, k = ft.inputs()["text_last_unit"]
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=1)
    try:
        with limit(300):
            plain = enc.encode(data)
        enc.arm_fast_tables(k)
        with limit(300):
            armed = enc.encode(data)
        assert enc.fast_tables()["n"] == ft.unit_sizes(len(data))[k]
        with limit(300):
            again = enc.encode(data)       # the capture was for one encode
        with pytest.raises(gpu.OrzError):
            enc.arm_fast_tables(70000)
    finally:
        enc.close()
    assert armed == plain and again == plain


def test_an_unarmed_encoder_writes_the_streams_recorded_before_the_capture_existed(gpu):
    """tests/golden/fast_small_cases.json: SHA-256 of the fast mode's -l1 streams of _data.SMALL_CASES, written by the host
    emulation of the commit before the capture hook (the GPU's bytes equal the emulation's: DESIGN 2, bar (4))"""
    want = json.load(open(os.path.join(HERE, "golden", "fast_small_cases.json")))
    assert sorted(want) == sorted(_data.SMALL_CASES)
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=1)
    try:
        for name, data in sorted(_data.SMALL_CASES.items()):
            with limit(120):
                out = enc.encode(data)
            assert hashlib.sha256(out).hexdigest() == want[name], name
    finally:
        enc.close()


def test_refusals(gpu):
    with limit(300):
        enc = gpu.StreamEncoder(device=0, level=1, mode="exact")
    try:
        with pytest.raises(gpu.OrzError):
            enc.arm_fast_tables(0)
        enc.set_mode("fast")
        with pytest.raises(gpu.OrzError):
            enc.fast_tables()               # nothing captured yet
        lib = enc._lib
        assert lib.orz_stream_fast_tables(None, 0, None, None, 0) == -22
        assert lib.orz_stream_fast_tables(enc._h, 0, b"no_such_table", None, 0) == -22
    finally:
        enc.close()
