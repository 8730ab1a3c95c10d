"""The symbol-ranking chain on the host emulation (emu_symrank: the backend's symrank, the plain loop of orz_kernels.h) against
the reference loop (tests/pyref SymRank) and the oracle's recorded ranks, on the adversarial launches of tests/_symchains.py;
the path model's proof that those launches reach every place where orz_symrank_kernel changes regime; and the Python
refusals of orz_amd.symrank_chains.  tests/test_gpu_symrank.py runs the same launches through the kernel itself."""
import ctypes

import numpy as np
import pytest

import _symchains as sc


def _emu_run(emu, tables, gsym, rstart):
    lib = emu.lib
    t = np.ascontiguousarray(tables, dtype=np.uint16).copy()
    g = np.ascontiguousarray(gsym, dtype=np.uint32)
    r = np.ascontiguousarray(rstart, dtype=np.uint32)
    ranks = np.zeros(max(1, g.size), dtype=np.uint16)
    flags = np.zeros(2, dtype=np.uint32)
    us = ctypes.c_double()
    rc = lib.emu_symrank(0, ctypes.c_void_p(t.ctypes.data), ctypes.c_void_p(g.ctypes.data), ctypes.c_void_p(r.ctypes.data),
                         ctypes.c_size_t(g.size), ctypes.c_void_p(ranks.ctypes.data), ctypes.c_void_p(flags.ctypes.data),
                         ctypes.byref(us))
    return rc, ranks[:g.size], t, (int(flags[0]), int(flags[1]))


def _assert_same(name, ranks, tables, ref_ranks, ref_tables):
    bad = np.nonzero(ranks != ref_ranks)[0]
    assert bad.size == 0, "%s: %d ranks differ, first at item %d: %d vs reference %d" % (
        name, bad.size, bad[0], ranks[bad[0]], ref_ranks[bad[0]])
    badc = np.nonzero((tables != ref_tables).any(axis=1))[0]
    assert badc.size == 0, "%s: tables of %d contexts differ, first context %d (cnt/sum %s vs %s)" % (
        name, badc.size, badc[0], tables[badc[0], -4:].tolist(), ref_tables[badc[0], -4:].tolist())


@pytest.fixture(scope="module")
def launches():
    out = []
    for L in sc.launches_a_to_d():
        gsym, rstart = L.arrays()
        ref_ranks, ref_tables, raw = sc.reference(L.tables, gsym, rstart)
        out.append((L, gsym, rstart, ref_ranks, ref_tables, raw))
    return out


def test_emulation_equals_the_reference_on_families_a_to_d(emu, launches):
    for L, gsym, rstart, ref_ranks, ref_tables, _ in launches:
        rc, ranks, tables, flags = _emu_run(emu, L.tables, gsym, rstart)
        assert rc == 0, L.name
        _assert_same(L.name, ranks, tables, ref_ranks, ref_tables)
        assert flags == (0, 0), L.name


def test_emulation_equals_the_reference_across_launches(emu):
    A, B = sc.family_e()
    ga, ra = A.arrays()
    gb, rb = B.arrays()
    ref_a, ref_ta, _ = sc.reference(A.tables, ga, ra)
    ref_b, ref_tb, _ = sc.reference(ref_ta, gb, rb)
    rc, ranks_a, ta, _ = _emu_run(emu, A.tables, ga, ra)
    assert rc == 0
    _assert_same(A.name, ranks_a, ta, ref_a, ref_ta)
    rc, ranks_b, tb, _ = _emu_run(emu, ta, gb, rb)
    assert rc == 0
    _assert_same(B.name, ranks_b, tb, ref_b, ref_tb)


@pytest.mark.parametrize("kind", ["text", "random"])
def test_emulation_equals_the_oracle_on_a_recorded_block(emu, oracle, kind):
    tables, gsym, rstart, want = sc.recorded_block(oracle, sc.recorded_inputs()[kind])
    rc, ranks, _, flags = _emu_run(emu, tables, gsym, rstart)
    assert rc == 0
    bad = np.nonzero(ranks != want)[0]
    assert bad.size == 0, "%s: %d of %d ranks differ from the oracle's, first at %d" % (kind, bad.size, want.size, bad[0])
    assert flags == (0, 0)


def test_the_launches_reach_every_path_of_the_kernel(launches, capsys):
    """by the path model: the launches of families a-d make the kernel take every regime and side path it has"""
    cov = sc.Coverage()
    for _, _, _, ref_ranks, _, raw in launches:
        cov.add(raw, ref_ranks)
    s = cov.summary()
    with capsys.disabled():
        print("\nsymrank path coverage:", s)
    assert cov.spec_ok > 500 and cov.spec_fail > 100, s
    r_any = set(range(32))
    assert cov.edge_only > 20, s  # (sums exactly on the edge the check's strict compare exists for)
    assert {0, 31}.issubset(cov.fail_lanes) and {"r-1", "r"}.issubset(cov.fail_lanes), s
    assert cov.r_ok == r_any, "scaling lanes of passing speculative groups: missing %s" % sorted(r_any - cov.r_ok)
    assert cov.r_checked == r_any, "scaling lanes of checked groups: missing %s" % sorted(r_any - cov.r_checked)
    assert cov.tails == r_any, "tails: missing %s" % sorted(r_any - cov.tails)
    assert 192 in cov.start_cnts and 327 in cov.start_cnts, s
    assert cov.checked_q32 > 0, s
    assert {0, 387, 388}.issubset(cov.out_ranks), s


def test_the_path_model_on_hand_made_chains():
    """the model's rules themselves, on chains whose split is known without it"""
    m = sc.path_model(0, 1000000, [0] * 191)
    assert m["plain"] == 191 and m["groups"] == [] and m["tail"] is None
    m = sc.path_model(0, 1000000, [0] * (192 + 64 + 5))
    assert m["plain"] == 192 + 5 and len(m["groups"]) == 2 and m["tail"] == 5
    assert m["groups"][0]["cnt"] == 192 and not m["groups"][0]["spec"]  # a fresh context's quotient is far above 32
    # a steady context whose quotient cannot move: rank 16 q every item at q = 1 keeps sum / 16 / count at 1
    m = sc.path_model(350, 16 * 350 + 8, [16] * 32)
    g = m["groups"][0]
    assert g["spec"] and g["ok"] and g["r"] == 40 and m["tail"] == 0
    # rank 388 at item 0 of a group at the top of q = 0's interval moves the quotient there
    m = sc.path_model(350, 16 * 350 - 1, [388] + [0] * 31)
    assert m["groups"][0]["spec"] and m["groups"][0]["bad"] == 0 and not m["groups"][0]["ok"]
    # count 390: the group's first item scales by 9/10
    assert sc.path_model(390, 5000, [3] * 32)["groups"][0]["r"] == 0


def _valid():
    L = sc.Launch("valid")
    L.items[3] = [(1, 2), (5, 5)]
    L.items[7] = [(388, 0)]
    gsym, rstart = L.arrays()
    return L.tables.copy(), gsym, rstart


def test_symrank_chains_refuses_invalid_input_in_python():
    import orz_amd

    tables, gsym, rstart = _valid()
    orz_amd.api._symrank_inputs(tables, gsym, rstart)  # (the valid launch passes)
    bad = []
    r = rstart.copy(); r[5], r[6] = r[6], r[5] + 1; bad.append((tables, gsym, r))          # not monotone
    r = rstart.copy(); r[512] += 1; bad.append((tables, gsym, r))                          # not ending at nitems
    r = rstart.copy(); r[0] = 1; bad.append((tables, gsym, r))                             # not starting at 0
    bad.append((tables, gsym, rstart[:512]))                                               # not 513 entries
    g = gsym.copy(); g[0] = 389; bad.append((tables, g, rstart))                           # symbol 389
    g = gsym.copy(); g[0] = 1 | (389 << 16); bad.append((tables, g, rstart))               # excluded symbol 389
    t = tables.copy(); t[9, 0], t[9, 1] = t[9, 1], t[9, 0]; bad.append((t, gsym, rstart))  # value[] / index[] disagree
    t = tables.copy(); t[9, 0] = 389; bad.append((t, gsym, rstart))                        # value out of range
    t = tables.copy(); t[9, 778] = 391; bad.append((t, gsym, rstart))                      # count 391
    t = tables.copy(); s = sc.MAX_SUM + 1; t[9, 780], t[9, 781] = s & 0xFFFF, s >> 16; bad.append((t, gsym, rstart))
    bad.append((tables[:511], gsym, rstart))                                               # 511 contexts
    for t, g, r in bad:
        with pytest.raises(ValueError):
            orz_amd.api._symrank_inputs(t, g, r)
        with pytest.raises(ValueError):
            orz_amd.symrank_chains(t, g, r)
    t = tables.copy(); s = sc.MAX_SUM; t[9, 778] = 390; t[9, 780], t[9, 781] = s & 0xFFFF, s >> 16
    orz_amd.api._symrank_inputs(t, gsym, rstart)  # (the largest count and sum pass)


def test_emu_symrank_refuses_what_the_library_refuses(emu):
    tables, gsym, rstart = _valid()
    assert _emu_run(emu, tables, gsym, rstart)[0] == 0
    r = rstart.copy(); r[5], r[6] = r[6], r[5] + 1
    assert _emu_run(emu, tables, gsym, r)[0] != 0
    g = gsym.copy(); g[1] = 7 | (400 << 16)
    assert _emu_run(emu, tables, g, rstart)[0] != 0
    t = tables.copy(); t[0, 0], t[0, 1] = t[0, 1], t[0, 0]
    assert _emu_run(emu, t, gsym, rstart)[0] != 0
    t = tables.copy(); s = sc.MAX_SUM + 1; t[4, 780], t[4, 781] = s & 0xFFFF, s >> 16
    assert _emu_run(emu, t, gsym, rstart)[0] != 0
