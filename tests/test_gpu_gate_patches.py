"""The validity gate (orz_amd/csrc/orz_verify.h) on the GPU, held to the oracle's verdict on PATCHED parses, through the C ABI
(orz_stream_set_item_patches).  The cases, the targets and the one rule of judging are those of the emulation's tier
(tests/_gatecases.py, tests/test_gate_patches_emu.py); here the sweep runs in full on the three-unit input -- every family in
every unit, the first and the last item of a unit included, state carried over two slides --, on the overlap input and on the
whole-block configuration.  One encoder serves a sweep: it must live on after every finding (checked after the first and at
the end).  Rules checked: LZDecoder::decode, src/lz.rs:417-474; rings src/matcher.rs:62-80."""
import pytest

import _gatecases as G

pytestmark = pytest.mark.gpu

FIRED = set()
WITNESS = {G.TILING: "match_to_literal", G.AFTER_LIT: "al", G.CONTEXT: "ctx", G.SYMBOL: "sym", G.NO_START: "src_no_item_start",
           G.OTHER_RING: "src_other_ring", G.BYTES: "src_bytes_short", G.OUTSIDE: "src_4094", G.OFFSET_CODE: "rob", G.ORDINAL: "ord",
           G.LEN_MIN: "src_len_min_above", G.LEN_CODE: "lmv", G.UNLIKELY: "unl", G.WORD_PRED: "literals_to_word"}
WHOLE = 16777216


def _gate(unit, mode="fast"):
    mp = pytest.MonkeyPatch()
    mp.setenv("ORZ_FAST_UNIT", str(unit))   # (read when the encoder is built)
    try:
        return G.GpuGate(mode)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def units():
    """input (a) in units of 1 MiB (three units, the last one short): the sweep's encoder, the clean parse, a fresh encoder's stream"""
    gate = _gate(1 << 20)
    data = G.input_a()
    fresh = _gate(1 << 20)
    try:
        clean, tr, msg = fresh.encode(data, want_trace=True)
    finally:
        fresh.close()
    assert clean is not None, msg
    ps = G.Parse(data, tr)
    assert len(ps.units) == 3
    state = {"checked_after_first_finding": False}
    yield gate, ps, clean, state
    gate.close()


@pytest.fixture(scope="module")
def whole():
    """inputs (c) and (b) in one unit each (whole blocks)"""
    gate = _gate(WHOLE)
    yield gate
    gate.close()


def _run(gate, ps, oracle, cases, clean=None, state=None):
    for c in cases:
        out, _, msg = gate.encode(ps.data, c.patches)
        FIRED.update(G.judge(ps, oracle, c, out, msg))
        if out is None and state is not None and not state["checked_after_first_finding"]:
            state["checked_after_first_finding"] = True
            assert gate.encode(ps.data)[0] == clean, "after a finding the encoder does not write a fresh encoder's stream"


@pytest.mark.parametrize("unit", [0, 1, 2])
@pytest.mark.parametrize("family", G.LEGAL_SRC_FAMILIES + G.ILLEGAL_SRC_FAMILIES + G.SHAPE_FAMILIES + G.ITEM_FAMILIES)
def test_single_patches_in_every_unit(units, oracle, family, unit):
    """one patch per encode: the first and the last eligible item of the unit, its items 0 and n - 1, those around 64, 256 and 4096,
    three random ones"""
    gate, ps, clean, state = units
    cases = G.targets(ps, ps.units[unit], family)
    if family == "src_earlier_unit" and unit == 0:
        assert not cases   # (nothing before the first unit)
        return
    assert cases, "no item of unit %d is eligible for %s" % (unit, family)
    _run(gate, ps, oracle, cases, clean, state)


@pytest.mark.parametrize("unit", [0, 1, 2])
@pytest.mark.parametrize("side", ["below", "at"])
def test_sources_on_both_sides_of_every_reduced_offset_base(units, oracle, side, unit):
    gate, ps, clean, state = units
    fams = [f for f in G.ROID_FAMILIES if f.endswith(side)]
    lo, hi = ps.unit_items[ps.units[unit]]
    cases = [c for f in fams for c in G.targets(ps, ps.units[unit], f, nrandom=0, edges=False, reach=hi - lo)[:1]]
    assert len(cases) >= len(fams) - 2, "only %d of %d bases have a match with an equal node at that distance" % (len(cases), len(fams))
    _run(gate, ps, oracle, cases, clean, state)


def test_many_legal_patches_at_once_over_three_units(units, oracle):
    """per unit 100+ legal sources no parser writes, 5+ at ring distance 4093, 5+ (behind the first unit) in an EARLIER unit"""
    gate, ps, clean, _ = units
    chosen, patches, _ = G.legal_set(ps, oracle)
    G.legal_floors(ps, chosen)
    out, _, msg = gate.encode(ps.data, patches)
    assert out is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
    assert oracle.decode(out)[0] == ps.data and out != clean


def test_whole_block_stream_is_the_oracles_for_the_patched_plan(whole, oracle):
    """input (c) in one unit: the stream of 100+ legal patches equals oracle.encode_plan(patched plan) byte for byte"""
    data = G.input_c()
    clean, tr, msg = whole.encode(data, want_trace=True)
    assert clean is not None, msg
    ps = G.Parse(data, tr)
    assert G.oracle_verdict(oracle, data, ps.plan())[0] == clean
    chosen, patches, want = G.legal_set(ps, oracle)
    G.legal_floors(ps, chosen)
    out, _, msg = whole.encode(data, patches)
    assert out is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
    assert out == want and out != clean and oracle.decode(out)[0] == data
    assert whole.encode(data)[0] == clean   # (the list held for one encode)


def test_overlapping_sources(whole, oracle):
    """input (b): sources that overlap their item, moved to ANOTHER overlapping node -- singly, and 5+ among 100+ legal patches"""
    data = G.input_b()
    clean, tr, msg = whole.encode(data, want_trace=True)
    assert clean is not None, msg
    ps = G.Parse(data, tr)
    singles = G.targets(ps, 0, "src_overlap", nrandom=0, edges=False, reach=ps.n)
    assert singles, "no match of the input has a second overlapping source"
    _run(whole, ps, oracle, singles)
    chosen, patches, want = G.legal_set(ps, oracle, overlap=True)
    G.legal_floors(ps, chosen, overlap=True)
    got, _, msg = whole.encode(data, patches)
    assert got is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
    assert oracle.decode(got)[0] == data and got == want


def test_exact_mode_shares_the_gate(oracle):
    gate = _gate(WHOLE, "exact")
    try:
        data = G.input_c()
        out, tr, msg = gate.encode(data, exact=True, want_trace=True)
        assert out is not None, msg
        ps = G.Parse(data, tr)
        bad = G.targets(ps, 0, "src_other_ring", nrandom=0, edges=False)[:1]
        good = [G.accepted_src_case(ps, oracle)]
        assert bad and good[0] is not None
        for c in bad + good:
            got, _, msg = gate.encode(data, c.patches, exact=True)
            FIRED.update(G.judge(ps, oracle, c, got, msg))
        assert gate.encode(data, exact=True)[0] == out
    finally:
        gate.close()


def test_refusals_of_the_hook(whole, oracle):
    """ORZ_EINVAL for every value a later kernel would index with out of range; an unapplied patch fails the encode in words of its
    own; the list does not survive into the next encode"""
    import orz_amd

    data = G.input_c()
    clean, tr, msg = whole.encode(data, want_trace=True)
    ps = G.Parse(data, tr)
    i = int(G.targets(ps, 0, "len_minus", nrandom=0)[0].item)
    b, p = ps.where(i)
    bad = [("TYPE", 3), ("TYPE", 2), ("LEN", 241), ("SRC", 0), ("SRC", p), ("SRC", p + 1), ("SYM", 389), ("CTX", 512), ("AL", 2), ("ENC", 240),
           ("UNL", 256), ("LMV", 128), ("ROB", 0x1001 | 2), ("ROB", 13 << 12), (11, 0)]
    for patches in [[(b, p, f, v)] for f, v in bad] + [[(b, G.P - 1, "LEN", 5)]]:
        with pytest.raises(orz_amd.OrzError, match=r"orz_stream_set_item_patches failed \(-22\): item patches"):   # ORZ_EINVAL
            whole.encode(data, patches)
    inside = p + 1   # (a match is at least four bytes long: no item starts here)
    assert ps.item_at[ps.so[i] + 1] < 0
    for patches in ([(b, inside, "LEN", 5)], [(b + 7, p, "LEN", 5)], [(b, p, "UNL", int(ps.tr["unlikely"][i])), (b, inside, "AL", 0)]):
        out, _, msg = whole.encode(data, patches)
        assert out is None and "item patches: 1 of %d patches were not applied" % len(patches) in msg, msg
    assert whole.encode(data)[0] == clean


def test_every_class_of_finding_fires_and_the_encoder_lives_on(units, oracle):
    """each of the fourteen classes of VerErr has produced a finding in the sweeps (run alone: one witness each is encoded here); at
    the end of the sweep the one encoder still writes a fresh encoder's stream"""
    gate, ps, clean, state = units
    for cls in G.ALL_CLASSES:
        if cls not in FIRED:
            _run(gate, ps, oracle, G.targets(ps, ps.units[1], WITNESS[cls], nrandom=0, edges=False)[:1], clean, state)
    assert not [c for c in G.ALL_CLASSES if c not in FIRED]
    assert state["checked_after_first_finding"]
    assert gate.encode(ps.data)[0] == clean
