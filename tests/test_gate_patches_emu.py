"""The validity gate (orz_amd/csrc/orz_verify.h) held to the oracle's verdict on PATCHED parses, on the host emulation.

tests/test_emu_verify.py injects seven kinds of defect at one place of one block.  Here every item of a parse can be aimed at
(item patches: orz_verify.h ItemPatchApply, tests/emu emu_encode_fast_patched), and the judge of a patched parse is the oracle's
plan-driven encoder, not the gate's author: tests/_gatecases.py has the families, the targets and the one rule (`judge`) -- what
the oracle accepts the gate passes and the stream decodes; what it rejects the gate rejects, at that item, under the matching
class.  Every class of VerErr fires here but for the arm DESIGN.md names (a source at or above its item: the hook holds SRC
below pos).  Rules checked: LZDecoder::decode, src/lz.rs:417-474; rings src/matcher.rs:62-80.

Cost: an emulated encode of the 300 KB input takes about 2 s, of the 2.5 MB three-unit input about 40 s -- the full sweep runs on
the small one, the large one and the overlap input get 11 encodes between them (units behind a slide, many legal patches at once)."""
import os

import pytest

import _gatecases as G

FIRED = set()   # classes of findings the sweeps below have seen (test_every_class_of_finding_fires)
WITNESS = {G.TILING: "match_to_literal", G.AFTER_LIT: "al", G.CONTEXT: "ctx", G.SYMBOL: "sym", G.NO_START: "src_no_item_start",
           G.OTHER_RING: "src_other_ring", G.BYTES: "src_bytes_short", G.OUTSIDE: "src_4094", G.OFFSET_CODE: "rob", G.ORDINAL: "ord",
           G.LEN_MIN: "src_len_min_above", G.LEN_CODE: "lmv", G.UNLIKELY: "unl", G.WORD_PRED: "literals_to_word"}


class _Unit:
    """ORZ_FAST_UNIT for the encodes of a test (the emulation's kept encoder is rebuilt when it changes)"""

    def __init__(self, value):
        self.value = str(value)

    def __enter__(self):
        self.old = os.environ.get("ORZ_FAST_UNIT")
        os.environ["ORZ_FAST_UNIT"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["ORZ_FAST_UNIT"]
        else:
            os.environ["ORZ_FAST_UNIT"] = self.old


WHOLE = 16777216


@pytest.fixture(scope="module")
def gate(emu):
    return G.EmuGate(emu)


@pytest.fixture(scope="module")
def small(gate, oracle):
    """input (c), one whole-block unit: its clean parse from a FRESH encoder, and that encoder's stream"""
    data = G.input_c()
    with _Unit(WHOLE):
        out, tr, msg = gate.encode(data, want_trace=True, fresh=True)
    assert out is not None, msg
    ps = G.Parse(data, tr)
    assert G.oracle_verdict(oracle, data, ps.plan())[0] == out   # the clean parse is a valid plan, and the post stage writes the oracle's bytes
    return ps, out


def _run(gate, ps, oracle, cases, exact=False):
    for c in cases:
        out, _, msg = gate.encode(ps.data, c.patches, exact=exact)
        FIRED.update(G.judge(ps, oracle, c, out, msg))


@pytest.mark.parametrize("family", G.LEGAL_SRC_FAMILIES + G.ILLEGAL_SRC_FAMILIES + G.SHAPE_FAMILIES + G.ITEM_FAMILIES)
def test_single_patches_on_the_small_input(gate, oracle, small, family):
    """one patch per encode: the first and the last eligible item, items 0 and n - 1, the items around 64, 256 and 4096, a random one"""
    ps, _ = small
    cases = G.targets(ps, 0, family, nrandom=1)
    if family == "src_earlier_unit":
        assert not cases   # (one unit: nothing before it -- the three-unit input below)
        return
    assert cases, "no item of the input is eligible for " + family
    with _Unit(WHOLE):
        _run(gate, ps, oracle, cases)


@pytest.mark.parametrize("side", ["below", "at"])
def test_sources_on_both_sides_of_every_reduced_offset_base(gate, oracle, small, side):
    """the last ring distance of one offset code and the first of the next (roid_encode): legal both, coded differently"""
    ps, _ = small
    fams = [f for f in G.ROID_FAMILIES if f.endswith(side)]
    cases = [c for f in fams for c in G.targets(ps, 0, f, nrandom=0, edges=False, reach=ps.n)[:1]]
    assert len(cases) >= len(fams) - 2, "only %d of %d bases have a match with an equal node at that distance" % (len(cases), len(fams))
    with _Unit(WHOLE):
        _run(gate, ps, oracle, cases)


def test_the_encoder_lives_on_after_a_finding_and_the_list_does_not(gate, oracle, small):
    """after a gate finding the SAME encoder encodes the clean input to the bytes of a fresh encoder's stream (orz_members callers
    rely on it; the sweeps here share one encoder because of it) -- the patch list held for the failed encode only"""
    ps, clean = small
    case = G.targets(ps, 0, "match_to_literal", nrandom=0)[0]
    with _Unit(WHOLE):
        out, _, msg = gate.encode(ps.data, case.patches)
        assert out is None and "validity gate" in msg, msg
        again, _, msg = gate.encode(ps.data)
    assert again == clean, msg


def test_many_legal_patches_at_once_on_the_small_input(gate, oracle, small):
    """another LEGAL parse no parser writes: 100+ sources moved to other nodes of their rings, 5+ of them to ring distance 4093 --
    the gate passes, the stream decodes, and in this whole-block configuration it is the oracle's stream for that plan, byte for byte"""
    ps, clean = small
    chosen, patches, want = G.legal_set(ps, oracle)
    G.legal_floors(ps, chosen)
    with _Unit(WHOLE):
        out, _, msg = gate.encode(ps.data, patches)
        assert out is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
        assert oracle.decode(out)[0] == ps.data
        assert out == want and out != clean
        assert gate.encode(ps.data)[0] == clean   # (the list is gone)


def test_refusals_of_the_hook(gate, oracle, small):
    """every value a later kernel would index with out of range is refused before anything runs; a patch that finds no item start
    fails the encode in words of its own; neither leaves anything behind"""
    ps, clean = small
    i = int(G.targets(ps, 0, "len_minus", nrandom=0)[0].item)
    b, p = ps.where(i)
    bad = [("TYPE", 3), ("TYPE", 2), ("LEN", 241), ("SRC", 0), ("SRC", p), ("SRC", p + 1), ("SYM", 389), ("CTX", 512), ("AL", 2), ("ENC", 240),
           ("UNL", 256), ("LMV", 128), ("ROB", 0x1001 | 2), ("ROB", 13 << 12), (11, 0)]
    with _Unit(WHOLE):
        for f, v in bad:
            with pytest.raises(ValueError, match="item patches"):
                gate.encode(ps.data, [(b, p, f, v)])
        with pytest.raises(ValueError, match="item patches"):
            gate.encode(ps.data, [(b, G.P - 1, "LEN", 5)])
        inside = p + 1   # (a match is at least four bytes long: no item starts here)
        assert ps.item_at[ps.so[i] + 1] < 0
        for patches in ([(b, inside, "LEN", 5)], [(b + 7, p, "LEN", 5)], [(b, p, "UNL", int(ps.tr["unlikely"][i])), (b, inside, "AL", 0)]):
            out, _, msg = gate.encode(ps.data, patches)
            assert out is None and "item patches: 1 of %d patches were not applied" % len(patches) in msg, msg
        assert gate.encode(ps.data)[0] == clean


def test_exact_mode_shares_the_gate(gate, oracle):
    """the post stage and the gate are the exact mode's too: one rejected and one accepted SRC patch on its parse"""
    data = G.input_c()[:120_000]
    out, tr, msg = gate.encode(data, exact=True, want_trace=True)
    assert out is not None, msg
    ps = G.Parse(data, tr)
    bad = G.targets(ps, 0, "src_other_ring", nrandom=0, edges=False)[:1]
    good = [G.accepted_src_case(ps, oracle)]
    assert bad and good[0] is not None
    _run(gate, ps, oracle, bad + good, exact=True)
    assert gate.encode(data, exact=True)[0] == out


@pytest.fixture(scope="module")
def large(gate):
    """input (a) in units of 1 MiB: three units, the last one short -- what the gate carries from unit to unit is judged here"""
    data = G.input_a()
    with _Unit(1 << 20):
        out, tr, msg = gate.encode(data, want_trace=True)
    assert out is not None, msg
    ps = G.Parse(data, tr)
    assert len(ps.units) == 3
    return ps, out


def test_findings_behind_a_slide(gate, oracle, large):
    """the first items of the later units (after_literal and the ordinal: vlast, vctx carried over the slide) and sources judged against
    records and ordinals that slid (vrec, vord, the len_min kept in vrec); the many legal patches below add vwords and the rest"""
    ps, _ = large
    cases = []
    for unit, fams in ((1, ("al", "src_4094")), (2, ("ord", "src_len_min_above"))):
        for f in fams:
            cs = G.targets(ps, unit, f, nrandom=0, edges=True)
            assert cs and (f.startswith("src_") or cs[0].item == ps.unit_items[unit][0]), (unit, f)
            cases.append(cs[0])
    with _Unit(1 << 20):
        _run(gate, ps, oracle, cases)


def test_many_legal_patches_at_once_over_three_units(gate, oracle, large):
    """per unit 100+ legal sources no parser writes, 5+ at ring distance 4093, 5+ (behind the first unit) in an EARLIER unit: the gate
    passes what the oracle accepts, and the stream decodes"""
    ps, clean = large
    chosen, patches, _ = G.legal_set(ps, oracle)
    G.legal_floors(ps, chosen)
    with _Unit(1 << 20):
        out, _, msg = gate.encode(ps.data, patches)
    assert out is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
    assert oracle.decode(out)[0] == ps.data and out != clean


def test_overlapping_sources(gate, oracle):
    """input (b): sources that overlap their item, moved to ANOTHER overlapping node -- singly, and 5+ among 100+ legal patches"""
    data = G.input_b()
    with _Unit(WHOLE):
        out, tr, msg = gate.encode(data, want_trace=True)
        assert out is not None, msg
        ps = G.Parse(data, tr)
        singles = G.targets(ps, 0, "src_overlap", nrandom=0, edges=False, reach=ps.n)
        assert singles, "no match of the input has a second overlapping source"
        _run(gate, ps, oracle, singles)
        chosen, patches, want = G.legal_set(ps, oracle, overlap=True)
        G.legal_floors(ps, chosen, overlap=True)
        got, _, msg = gate.encode(data, patches)
    assert got is not None, "the oracle accepts the patched plan, the gate refuses it: " + msg
    assert oracle.decode(got)[0] == data and got == want


def test_every_class_of_finding_fires(gate, oracle, small):
    """each of the fourteen classes of VerErr has produced a finding above (run alone: one witness each is encoded here)"""
    ps, _ = small
    with _Unit(WHOLE):
        for cls in G.ALL_CLASSES:
            if cls not in FIRED:
                _run(gate, ps, oracle, G.targets(ps, 0, WITNESS[cls], nrandom=0, edges=False)[:1])
    assert not [c for c in G.ALL_CLASSES if c not in FIRED]
