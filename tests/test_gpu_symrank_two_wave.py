"""GPU tier: orz_symrank_kernel on two wavefronts -- wave 0 the chain, wave 1 value[]'s upkeep in unchecked groups, a sub-batch
behind -- through orz_symrank_chains on launches aimed at what the split adds (tests/_symsplit.py; the CPU tier shows with
the path model that each case is what its name says, and that the scheme itself reproduces the reference).  Every rank and
every context's final table must equal tests/pyref's SymRank; the guard must have found nothing."""
import numpy as np
import pytest

import _symchains as sc
import _symsplit as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from orz_amd import _native

    if _native.load().orz_device_count() <= 0:
        pytest.fail("GPU test selected but liborz_hip.so found no HIP device (no CPU fallback exists)")
    import orz_amd

    return orz_amd


NAMES = ["lengths", "scaling", "failed speculation", "repeated symbols", "displaced entries tracked", "ranks 0 1 388", "one hot context",
         "all contexts 40 items"]


@pytest.fixture(scope="module")
def cases():
    out = sp.launches()
    assert len(out) == len(NAMES)
    return out


def _same(name, ranks, tables, ref_ranks, ref_tables):
    bad = np.nonzero(ranks != ref_ranks)[0]
    assert bad.size == 0, "%s: %d ranks differ, first at item %d: %d vs reference %d" % (
        name, bad.size, bad[0], ranks[bad[0]], ref_ranks[bad[0]])
    badc = np.nonzero((tables != ref_tables).any(axis=1))[0]
    assert badc.size == 0, "%s: tables of %d contexts differ, first context %d (cnt/sum %s vs %s)" % (
        name, badc.size, badc[0], tables[badc[0], -4:].tolist(), ref_tables[badc[0], -4:].tolist())


@pytest.mark.parametrize("which", range(len(NAMES)), ids=NAMES)
def test_kernel_equals_the_reference(gpu, cases, which):
    L = cases[which]
    gsym, rstart = L.arrays()
    ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
    ranks, tables, flags, _ = gpu.symrank_chains(L.tables, gsym, rstart)
    _same(L.name, ranks, tables, ref_ranks, ref_tables)
    assert flags == (0, 0), (L.name, flags)


def test_one_chain_over_two_launches(gpu):
    """cut at a group boundary, in mid-group, inside a group's first sub-batch and one item short of a group"""
    L, cuts = sp.split_chain()
    gsym, rstart = L.arrays()
    ref_ranks, ref_tables, _ = sc.reference(L.tables, gsym, rstart)
    A, B = sp.halves(L, cuts)
    ga, ra = A.arrays()
    gb, rb = B.arrays()
    ranks_a, ta, fa, _ = gpu.symrank_chains(A.tables, ga, ra)
    ranks_b, tb, fb, _ = gpu.symrank_chains(ta, gb, rb)
    assert fa == (0, 0) and fb == (0, 0)
    for ctx in cuts:
        got = np.concatenate([ranks_a[ra[ctx]:ra[ctx + 1]], ranks_b[rb[ctx]:rb[ctx + 1]]])
        want = ref_ranks[rstart[ctx]:rstart[ctx + 1]]
        assert (got == want).all(), "context %d: first difference at item %d" % (ctx, np.nonzero(got != want)[0][0])
    assert (tb == ref_tables).all()
