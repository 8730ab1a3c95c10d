"""GPU tier: orz_symrank_kernel -- the encoder's whole ranking sequence (HipBackend::symrank: backup, kernel, SymCheck,
guarded rerun) through orz_symrank_chains -- against the reference loop (tests/pyref SymRank) on the adversarial launches of
tests/_symchains.py, and against the oracle's own ranks on recorded blocks.  Every item's rank and every context's table
(count and sum included, untouched contexts too) must match; the guard must have found nothing, and with a wrong rank
injected it must repair the block.  tests/test_symrank_chains.py shows, by the path model, that these launches reach every
regime of the kernel, and holds the host emulation to the same results."""
import ctypes
import json

import numpy as np
import pytest

import _symchains as sc

pytestmark = pytest.mark.gpu

ORZ_EINVAL = -22


@pytest.fixture(scope="module")
def gpu():
    from orz_amd import _native

    if _native.load().orz_device_count() <= 0:
        pytest.fail("GPU test selected but liborz_hip.so found no HIP device (no CPU fallback exists)")
    import orz_amd

    return orz_amd


@pytest.fixture(scope="module")
def launches():
    out = []
    for L in sc.launches_a_to_d():
        gsym, rstart = L.arrays()
        ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
        out.append((L, gsym, rstart, ref_ranks, ref_tables))
    return out


def _assert_same(name, ranks, tables, ref_ranks, ref_tables):
    bad = np.nonzero(ranks != ref_ranks)[0]
    assert bad.size == 0, "%s: %d ranks differ, first at item %d: %d vs reference %d" % (
        name, bad.size, bad[0], ranks[bad[0]], ref_ranks[bad[0]])
    badc = np.nonzero((tables != ref_tables).any(axis=1))[0]
    assert badc.size == 0, "%s: tables of %d contexts differ, first context %d (cnt/sum %s vs %s)" % (
        name, badc.size, badc[0], tables[badc[0], -4:].tolist(), ref_tables[badc[0], -4:].tolist())


def test_kernel_equals_the_reference_on_families_a_to_d(gpu, launches):
    for L, gsym, rstart, ref_ranks, ref_tables in launches:
        before = L.tables.copy()
        ranks, tables, flags, _ = gpu.symrank_chains(L.tables, gsym, rstart)
        _assert_same(L.name, ranks, tables, ref_ranks, ref_tables)
        assert flags == (0, 0), (L.name, flags)
        assert (L.tables == before).all(), "symrank_chains wrote into the caller's tables"


def test_kernel_equals_the_reference_across_launches(gpu):
    A, B = sc.family_e()
    ga, ra = A.arrays()
    gb, rb = B.arrays()
    ref_a, ref_ta, _ = sc.reference(A.tables, ga, ra)
    ref_b, ref_tb, _ = sc.reference(ref_ta, gb, rb)
    ranks_a, ta, fa, _ = gpu.symrank_chains(A.tables, ga, ra)
    _assert_same(A.name, ranks_a, ta, ref_a, ref_ta)
    ranks_b, tb, fb, _ = gpu.symrank_chains(ta, gb, rb)
    _assert_same(B.name, ranks_b, tb, ref_b, ref_tb)
    assert fa == (0, 0) and fb == (0, 0)


@pytest.mark.parametrize("kind", ["text", "random"])
def test_kernel_equals_the_oracle_on_a_recorded_block(gpu, oracle, emu, kind):
    """the oracle's trace ranks of a single-block input; the final tables against the host emulation's"""
    tables, gsym, rstart, want = sc.recorded_block(oracle, sc.recorded_inputs()[kind])
    ranks, tout, flags, us = gpu.symrank_chains(tables, gsym, rstart)
    bad = np.nonzero(ranks != want)[0]
    assert bad.size == 0, "%s: %d of %d ranks differ from the oracle's, first at %d" % (kind, bad.size, want.size, bad[0])
    assert flags == (0, 0)
    lib = emu.lib
    t = tables.copy()
    er = np.zeros(gsym.size, dtype=np.uint16)
    fl = np.zeros(2, dtype=np.uint32)
    assert lib.emu_symrank(0, ctypes.c_void_p(t.ctypes.data), ctypes.c_void_p(gsym.ctypes.data), ctypes.c_void_p(rstart.ctypes.data),
                           ctypes.c_size_t(gsym.size), ctypes.c_void_p(er.ctypes.data), ctypes.c_void_p(fl.ctypes.data), None) == 0
    assert (er == want).all()
    assert (tout == t).all(), "%s: final tables differ from the emulation's" % kind
    print(json.dumps({"kernel": "orz_symrank_kernel (+ guard)", "input": kind, "items": int(gsym.size),
                      "hottest_context": int(np.max(np.diff(rstart.astype(np.int64)))), "sequence_us": round(us, 1),
                      "items_per_s": round(gsym.size / (us * 1e-6)) if us > 0 else None}))


def test_guarded_rerun_repairs_an_injected_rank(gpu, launches, monkeypatch):
    """ORZ_SYMRANK_INJECT=k: item k's first-run rank reads 388 although its symbol is not the excluded one -- the check
    counts it, the second run from the saved tables (state_in / only_if) puts every rank and table right"""
    L, gsym, rstart, ref_ranks, ref_tables = launches[0]
    g = gsym.astype(np.int64)
    eligible = np.nonzero((g & 0xFFFF) != (g >> 16))[0]
    picks = [eligible[0], eligible[len(eligible) // 3], eligible[len(eligible) // 2], eligible[-1]]
    for k in picks:
        monkeypatch.setenv("ORZ_SYMRANK_INJECT", str(int(k)))
        ranks, tables, flags, _ = gpu.symrank_chains(L.tables, gsym, rstart)
        assert flags[0] >= 1 and flags[1] == 0, (int(k), flags)
        _assert_same("%s, rank %d injected" % (L.name, k), ranks, tables, ref_ranks, ref_tables)
    monkeypatch.delenv("ORZ_SYMRANK_INJECT")
    ranks, tables, flags, _ = gpu.symrank_chains(L.tables, gsym, rstart)
    assert flags == (0, 0)
    _assert_same(L.name, ranks, tables, ref_ranks, ref_tables)


def test_the_library_refuses_invalid_input(gpu):
    """the C ABI's own checks, past the Python wrapper's: ORZ_EINVAL, the tables untouched, and the next call still works"""
    from orz_amd import _native

    lib = _native.load()
    L = sc.Launch("refusals")
    L.items[3] = [(1, 2), (5, 5), (7, 1)]
    L.items[9] = [(388, 0)]
    gsym, rstart = L.arrays()
    ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)

    def call(tables, g, r):
        t = np.ascontiguousarray(tables, dtype=np.uint16).copy()
        ranks = np.zeros(g.size, dtype=np.uint16)
        flags = np.zeros(2, dtype=np.uint32)
        rc = lib.orz_symrank_chains(0, t.ctypes.data, g.ctypes.data, r.ctypes.data, g.size, ranks.ctypes.data, flags.ctypes.data, None)
        return rc, ranks, t

    t = L.tables.copy()
    t[9, 0], t[9, 1] = t[9, 1], t[9, 0]  # value[] and index[] disagree
    g = gsym.copy()
    g[1] = 389  # symbol out of range
    g2 = gsym.copy()
    g2[2] = 7 | (389 << 16)  # excluded symbol out of range
    r = rstart.copy()
    r[4], r[5] = r[5] + 1, r[4]  # not monotone
    r2 = rstart.copy()
    r2[512] -= 1  # not ending at nitems
    t3 = L.tables.copy()
    t3[3, 778] = 391  # count above 390
    for tt, gg, rr in [(t, gsym, rstart), (L.tables, g, rstart), (L.tables, g2, rstart), (L.tables, gsym, r), (L.tables, gsym, r2),
                       (t3, gsym, rstart)]:
        rc, _, tout = call(tt, gg, rr)
        assert rc == ORZ_EINVAL
        assert (tout == tt).all()
        rc, ranks, tout = call(L.tables, gsym, rstart)
        assert rc == 0
        _assert_same("after a refusal", ranks, tout, ref_ranks, ref_tables)
