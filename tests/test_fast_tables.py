"""CPU tier: the static per-block tables of the fast parse (orz_amd/csrc/orz_fast.h, prep kernels) as the host emulation of the
very same kernel bodies builds them, held entry for entry to the brute-force references of tests/_fasttables.py; coverage of the
cases the kernels' paths split on, asserted on the references alone; the bracket property of dist_valid; the refusals of the
capture.  tests/test_gpu_fast_tables.py holds the product library to the same references."""
import ctypes

import numpy as np
import pytest

import _fasttables as ft


class EmuItem(ctypes.Structure):
    _fields_ = [("block", ctypes.c_uint32), ("pos", ctypes.c_uint32), ("src", ctypes.c_uint32), ("sym", ctypes.c_uint16),
                ("rank", ctypes.c_uint16), ("ctx", ctypes.c_uint16), ("mlen", ctypes.c_uint8), ("al", ctypes.c_uint8),
                ("unl", ctypes.c_uint8), ("enc", ctypes.c_uint8)]


DTYPES = {"hpos": "<u4", "wsnap": "u1", "epos": "<u4", "keys": "<u4", "idx": "<u4", "runstart": "<u4", "rlen": "u1", "vbits": "<u8",
          "stext": "<u8", "cl": "<u8", "ccnt": "<u4", "rows": "u1", "rdist": "<u8", "kpos": "<u4", "kkeys": "<u4", "krun": "<u4",
          "kw": "<u2", "wmask": "<u8", "kmeta": "<u2", "hcm": "<u4", "hpre": "<u4"}


@pytest.fixture(autouse=True)
def _one_mib_units(monkeypatch):
    monkeypatch.setenv("ORZ_FAST_UNIT", str(ft.UNIT))


def emu_capture(emu, data, k, cfg=(15, 9, 6)):
    """(captured tables, items of the units before unit k) from the emulation"""
    lib = emu.lib
    lib.emu_fast_tables.restype = ctypes.c_long
    lib.emu_fast_table.restype = ctypes.c_long
    cap = len(data) + 16
    items = (EmuItem * cap)()
    data = bytes(data)
    got = lib.emu_fast_tables(data, ctypes.c_size_t(len(data)), cfg[0], cfg[1], cfg[2], int(k), items, ctypes.c_size_t(cap))
    if got < 0:
        return None, got
    arr = np.frombuffer(items, dtype=np.dtype([("block", "<u4"), ("pos", "<u4"), ("src", "<u4"), ("sym", "<u2"), ("rank", "<u2"),
                                               ("ctx", "<u2"), ("mlen", "u1"), ("al", "u1"), ("unl", "u1"), ("enc", "u1")], align=True))[:got]
    trace = {"block": arr["block"], "pos": arr["pos"], "word": arr["sym"] == 388, "mlen": np.where(arr["al"] & 2, arr["mlen"], 0)}

    def table(name, dtype):
        size = lib.emu_fast_table(name.encode(), None, ctypes.c_size_t(0))
        assert size >= 0, name
        buf = np.empty(size, dtype=np.uint8)
        lib.emu_fast_table(name.encode(), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(size))
        return buf.view(dtype)

    sc = table("scalars", "<u8")
    out = {key: int(sc[i]) for i, key in enumerate(("n", "nhist", "nent", "nk", "K", "stream_off", "block", "new_at"))}
    for name, dtype in DTYPES.items():
        out[name] = table(name, dtype)
    return out, trace


_REFS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_references_afterwards():
    yield
    _REFS.clear()   # (hundreds of MB: the coverage test reads them, nothing after this module does)


def held_to_reference(name, cap, trace):
    """the captured block against the reference; the reference is kept for the coverage test"""
    data, k = ft.inputs()[name]
    hpos, wsnap = ft.history_from_trace(data, k, trace)
    assert np.array_equal(cap["hpos"], hpos), "history item starts differ from the trace of the earlier units"
    assert np.array_equal(cap["wsnap"], wsnap), "words[] at the block start differs from the replay of the traced items"
    ref = ft.reference(data, k, hpos, wsnap)
    _REFS[name] = ref
    bad = ft.compare(cap, ref)
    assert not bad, "\n".join(bad)
    return ref


@pytest.mark.parametrize("name", sorted(ft.inputs()))
def test_emulated_tables_equal_their_definitions(emu, name):
    data, k = ft.inputs()[name]
    cap, trace = emu_capture(emu, data, k)
    assert cap is not None
    assert cap["n"] == ft.unit_sizes(len(data))[k] and cap["block"] == k and cap["new_at"] == ft.KPRE
    held_to_reference(name, cap, trace)


def coverage_gaps(refs):
    """classes the issue lists that no reference table contains (empty = all there)"""
    gaps = []
    sizes = {r["n"] for r in refs.values()}
    for n in (1, 63, 64, 65, 4095, 4097, ft.UNIT):
        if n not in sizes:
            gaps.append("block of %d bytes" % n)
    if not {0, 1, 63} <= {r["nent"] % 64 for r in refs.values()}:
        gaps.append("nent % 64 in {0, 1, 63}")
    pref = {}
    depth_classes, kinds, lanes, rks, flags = set(), set(), set(), set(), set()
    codes = set()
    near_end = set()
    past_end = False
    for r in refs.values():
        v, pa, qa = ft.true_prefixes(r)
        for L in ft.PREFIXES:
            sel = v == L
            pref.setdefault(L, set()).update(zip(pa[sel].tolist(), qa[sel].tolist()))
        d = r["depth"]
        for c in (0, 1, 31, 32, 33):
            if (d == c).any():
                depth_classes.add(c)
        if (d >= 255).any():
            depth_classes.add(255)
        rr = np.minimum(ft.K, d)
        hp = r["hist_pred"]
        nh = hp.sum(axis=1)
        has = rr > 0
        if (has & (nh == rr)).any():
            kinds.add("history")
        if (has & (nh == 0)).any():
            kinds.add("new")
        if ((nh > 0) & (nh < rr)).any():
            kinds.add("mixed")
        slot = r["idx"].astype(np.int64)
        for lane in (0, 63):   # a position in that lane of its 64-slot group with predecessors in the group before
            if (((slot & 63) == lane) & (d > lane)).any():
                lanes.add(lane)
        km = r["kmeta"]
        rks.update(np.unique(km & 0x7f).tolist())
        flags.update(("excl", int(x)) for x in np.unique((km >> 7) & 1))
        flags.update(("snap", int(x)) for x in np.unique((km >> 8) & 1))
        codes.update(ft.sampled_distances(r))
        # prefixes that end within 8 / 20 / 240 bytes of the block's end, and one that runs past it
        p = np.arange(ft.KPRE, ft.KPRE + r["n"], dtype=np.int64)
        ends = p[:, None] + r["rows"].astype(np.int64)
        live = np.arange(ft.K)[None, :] < rr[:, None]
        gap = r["end"] - ends
        for g in (8, 20, 240):
            if (live & (r["rows"] >= 4) & (gap >= 0) & (gap <= g)).any():
                near_end.add(g)
        if (live & (gap < 0)).any():
            past_end = True
    for L in ft.PREFIXES:
        if len(pref.get(L, ())) < 64:
            gaps.append("true common prefix %d at every alignment of both positions (have %d of 64)" % (L, len(pref.get(L, ()))))
    if depth_classes != {0, 1, 31, 32, 33, 255}:
        gaps.append("run depths 0, 1, 31, 32, 33, >= 255 (have %s)" % sorted(depth_classes))
    if kinds != {"history", "new", "mixed"}:
        gaps.append("rows with all-history / all-new / mixed predecessors (have %s)" % sorted(kinds))
    if lanes != {0, 63}:
        gaps.append("lane 0 and lane 63 with predecessors in the group before (have %s)" % sorted(lanes))
    if not {0, 1, 63, 64} <= rks:
        gaps.append("rk in {0, 1, 63, 64}")
    if len(flags) != 4:
        gaps.append("both values of each kmeta flag (have %s)" % sorted(flags))
    if near_end != {8, 20, 240} or not past_end:
        gaps.append("prefixes ending within 8 / 20 / 240 bytes of the block's end and past it (have %s, past %s)" % (sorted(near_end), past_end))
    # a distance on each side of every rounding step of dist_code_up: the exact value of a code, and one more (rounded up to the next)
    missing = ft.dist_gaps(codes, DIST_TOP)
    if missing:
        gaps.append("sampled distances v and v + 1 for the code values %s" % missing)
    return gaps


# The windows of this tier hold 2.4 MiB (a 16 MiB history takes the emulation minutes), so the tables here reach the rounding steps
# up to 2^20.  The steps from there to 2^24 are held twice elsewhere: test_distance_codes_equal_their_definition below runs the
# kernels' dist_code_up / dist_code_down over EVERY distance up to 2^25, and the GPU tier's input `far` (tests/_fasttables.py) puts
# a predecessor on each side of every step up to 2^24 into a captured block and asserts that coverage there.
DIST_TOP = 1 << 20


def test_distance_codes_equal_their_definition(emu):
    """dist_code_up(d) is the smallest code whose distance is not below d, dist_code_down(d) the largest whose distance is not
    above it (orz_fast.h: 'a distance is coded rounded UP, a budget rounded DOWN'), for every d a window can hold and beyond"""
    lib = emu.lib
    step = 1 << 22
    for d0 in range(0, 1 << 25, step):
        n = step + (1 if d0 + step == 1 << 25 else 0)
        up = np.empty(n, dtype=np.uint8)
        down = np.empty(n, dtype=np.uint8)
        lib.emu_dist_codes(ctypes.c_uint(d0), ctypes.c_size_t(n), up.ctypes.data_as(ctypes.c_void_p), down.ctypes.data_as(ctypes.c_void_p))
        d = np.arange(d0, d0 + n, dtype=np.int64)
        want_up = np.searchsorted(ft.CODE_VALUES, d, side="left")
        want_down = np.searchsorted(ft.CODE_VALUES, d, side="right") - 1
        bad = np.nonzero(up != want_up)[0]
        assert not len(bad), "dist_code_up(%d) = %d, want %d" % (d[bad[0]], up[bad[0]], want_up[bad[0]])
        bad = np.nonzero(down != want_down)[0]
        assert not len(bad), "dist_code_down(%d) = %d, want %d" % (d[bad[0]], down[bad[0]], want_down[bad[0]])


def test_the_emulation_writes_the_recorded_small_streams(emu):
    """tests/golden/fast_small_cases.json (what the GPU tier holds an unarmed encoder to) is what the emulation writes"""
    import hashlib
    import json
    import os

    import _data

    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fast_small_cases.json")))
    assert sorted(want) == sorted(_data.SMALL_CASES)
    for name, data in sorted(_data.SMALL_CASES.items()):
        assert hashlib.sha256(emu.fast(data)[0]).hexdigest() == want[name], name


def test_the_references_cover_the_cases_the_kernels_split_on(emu):
    """asserted on the reference tables alone (they are built by the comparison tests above; alone, this test builds them)"""
    for name, (data, k) in ft.inputs().items():
        if name not in _REFS:
            cap, trace = emu_capture(emu, data, k)
            hpos, wsnap = ft.history_from_trace(data, k, trace)
            _REFS[name] = ft.reference(data, k, hpos, wsnap)
    gaps = coverage_gaps(_REFS)
    assert not gaps, "\n".join(gaps)


def test_dist_valid_brackets_the_true_positions(emu):
    """for every position of a captured block and a spread of budgets: the `sure` newest predecessors lie within the budget and
    none from `limit` on does, by the positions themselves (predecessors beyond the tabulated ones are not claimed: every reader
    clamps by the tabulated depth)"""
    name = "text_last_unit"
    data, k = ft.inputs()[name]
    if name not in _REFS:
        cap, trace = emu_capture(emu, data, k)
        hpos, wsnap = ft.history_from_trace(data, k, trace)
        _REFS[name] = ft.reference(data, k, hpos, wsnap)
    r = _REFS[name]
    lib = emu.lib
    n = r["n"]
    rr = np.minimum(ft.K, r["depth"])
    idx, epos = r["idx"].astype(np.int64), r["epos"].astype(np.int64)
    p = np.arange(ft.KPRE, ft.KPRE + n, dtype=np.int64)
    codes = np.ascontiguousarray(r["rdist"], dtype=np.uint64)
    budgets = [0, 1, 15, 16, 17, 18, 31, 32, 33] + [v for e in range(6, 25) for v in ((1 << e) - 1, 1 << e, (1 << e) + 1)] + [3 << 18, 5 << 19]
    sure = np.empty(n, dtype=np.uint32)
    limit = np.empty(n, dtype=np.uint32)
    for b in budgets:
        bud = np.full(n, b, dtype=np.uint32)
        lib.emu_dist_valid_many(codes.ctypes.data_as(ctypes.c_void_p), bud.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n),
                                sure.ctypes.data_as(ctypes.c_void_p), limit.ctypes.data_as(ctypes.c_void_p))
        s = np.minimum(sure.astype(np.int64), rr)
        has = s > 0
        far = p[has] - epos[idx[has] - s[has]]              # the oldest of the `sure` ones
        assert (far <= b).all(), (b, int((far > b).sum()))
        lim = limit.astype(np.int64)
        has = lim < rr
        near = p[has] - epos[idx[has] - 1 - lim[has]]       # the newest from `limit` on
        assert (near > b).all(), (b, int((near <= b).sum()))
        assert (sure <= 64).all() and (limit <= 64).all()


def test_the_capture_refuses_a_block_the_stream_does_not_have(emu):
    cap, rc = emu_capture(emu, b"abc" * 100, 5)
    assert cap is None and rc == -2
    assert emu.lib.emu_fast_table(b"rows", None, ctypes.c_size_t(0)) < 0
