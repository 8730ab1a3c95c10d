"""CPU tier: the ranking kernel's two-wavefront split, restated with arrays (tests/_symsplit.py), against the reference coder.

Ranks are tracked per group; value[] is touched only by the two displaced moves an item, a sub-batch late, with the
entries of tracked symbols stale until the group's end.  If that scheme were wrong -- a displaced entry read too late, a
tracked symbol's stale entry moved somewhere it is not rewritten, a failed group's restore missing a move -- the model's
ranks or tables would differ from tests/pyref's SymRank on these chains.  The same launches go through the kernel in
tests/test_gpu_symrank_two_wave.py; here the path model also shows that each case is what its name says."""
import numpy as np
import pytest

import _symchains as sc
import _symsplit as sp
from pyref.orz_py import NSYMS


@pytest.fixture(scope="module")
def cases():
    out = []
    for L in sp.launches():
        gsym, rstart = L.arrays()
        ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
        out.append((L, gsym, rstart, ref_ranks, ref_tables, sp.describe(L, gsym, rstart)))
    return out


def _same(name, ranks, tables, ref_ranks, ref_tables):
    bad = np.nonzero(ranks != ref_ranks)[0]
    assert bad.size == 0, "%s: %d ranks differ, first at item %d" % (name, bad.size, bad[0])
    badc = np.nonzero((tables != ref_tables).any(axis=1))[0]
    assert badc.size == 0, "%s: tables of %d contexts differ, first context %d" % (name, badc.size, badc[0])


@pytest.mark.parametrize("m", sp.SUBS)
def test_the_split_reproduces_the_reference_on_the_aimed_cases(cases, m):
    for L, gsym, rstart, ref_ranks, ref_tables, what in cases:
        ranks, tables, passed = sp.model_launch(L.tables, gsym, rstart, m)
        _same("%s, m = %d" % (L.name, m), ranks, tables, ref_ranks, ref_tables)
        assert passed == sum(g["ok"] for w in what.values() for g in w["groups"]), L.name


@pytest.mark.parametrize("m", sp.SUBS)
def test_the_split_reproduces_the_reference_across_two_launches(m):
    L, cuts = sp.split_chain()
    gsym, rstart = L.arrays()
    ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
    A, B = sp.halves(L, cuts)
    ga, ra = A.arrays()
    gb, rb = B.arrays()
    ranks_a, ta, pa = sp.model_launch(A.tables, ga, ra, m)
    ranks_b, tb, pb = sp.model_launch(ta, gb, rb, m)
    assert pa > 0 and pb > 0
    for ctx, n in cuts.items():
        whole = ref_ranks[rstart[ctx]:rstart[ctx + 1]]
        assert (np.concatenate([ranks_a[ra[ctx]:ra[ctx + 1]], ranks_b[rb[ctx]:rb[ctx + 1]]]) == whole).all(), ctx
    assert (tb == ref_tables).all()


def test_the_split_reproduces_the_reference_on_families_a_to_d():
    for L in sc.launches_a_to_d():
        gsym, rstart = L.arrays()
        ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
        ranks, tables, _ = sp.model_launch(L.tables, gsym, rstart, 8)
        _same(L.name, ranks, tables, ref_ranks, ref_tables)


def test_every_case_is_what_its_name_says(cases):
    by_name = {L.name.split(";")[0].split(",")[0][:12]: (L, what) for L, _, _, _, _, what in cases}
    L, what = by_name["lengths 32"]
    for ctx, n in enumerate([32, 33, 63, 64, 65, 36, 40]):
        w = what[ctx]
        assert len(w["groups"]) == n // 32 and all(g["ok"] for g in w["groups"]) and w["tail"] == n % 32, (ctx, n)
    L, what = by_name["the 9/10 sca"]
    for ctx, r in enumerate([0, 3, 4, 7, 8, 31]):
        assert what[ctx]["groups"][0]["r"] == r and all(g["ok"] for g in what[ctx]["groups"]), (ctx, r)
    L, what = by_name["a failed spe"]
    for ctx, lane in enumerate([1, 30, 2, 29, 0, 31]):
        g0, g1 = what[ctx]["groups"]
        assert g0["spec"] and not g0["ok"] and g0["bad"] == lane and g1["ok"], (ctx, g0, g1)
    for key in ("one symbol i", "items whose ", "ranks 0"):
        L, what = by_name[key]
        assert all(g["ok"] for w in what.values() for g in w["groups"]) and all(len(w["groups"]) == 2 for w in what.values()), key
    L, what = by_name["one symbol i"]
    for ctx, w in what.items():
        pairs = L.items[ctx][:32]
        assert any(a[0] == b[0] for a, b in zip(pairs, pairs[1:])) or ctx % 2 == 1
        assert {v for v, _ in pairs} & {u for _, u in pairs}, "no symbol is also an excluded symbol of its group"
    L, what = by_name["items whose "]
    for ctx, w in what.items():
        # the symbols at next_i and at the mid point of an item's rotation belong to later items of the same group
        coder = sc.coder_of(L.tables[ctx])
        hits = 0
        for k, (v, u) in enumerate(L.items[ctx][:32]):
            i = coder.index[v]
            nx, y = sp._targets(i, w["groups"][0]["q"])
            later = {s for vu in L.items[ctx][k + 1:32] for s in vu}
            hits += nx != i and coder.value[nx] in later and coder.value[y] in later
            coder.encode(v, u)
        assert hits >= 8, (ctx, hits)
    L, what = by_name["ranks 0"]
    assert all({0, 1, NSYMS - 1} <= set(w["ranks"][:32]) for w in what.values())
    L, what = by_name["one hot cont"]
    assert list(what) == [200] and sum(g["ok"] for g in what[200]["groups"]) >= 40
    L, what = by_name["every contex"]
    assert len(what) == 512 and all(len(w["groups"]) == 1 and w["groups"][0]["ok"] and w["tail"] == 8 for w in what.values())
