"""GPU tier: the step machinery of the fast parse's round loop as the PRODUCT library launches it on the device (orz_fast_step_path,
orz_fast_step_counts, orz_fast_step_horizon: fast_decide / FastDecide, PathUpWave, PathTileDown in LDS and in global memory,
PathMarkWave, the thread-per-item forms, CountWave, FastPrefix alone and inside FlipPrefixWave, FastItemTotal, OrdWave, OrdWave2,
FastHorizon alone and inside RetireHorizonWave), held entry for entry to the serial references of tests/_stepcases.py -- not to the
emulation -- with poison outside the defined ranges.  Every case runs the fused form; the unfused and the thread-per-item form
take turns over the cases (each runs on a third of them, every family and tile among them), CountWave on the marks on a quarter.
One process; every device step runs under a time limit of its own that ends the process.  Whole encodes under ORZ_FAST_FUSED=0
and ORZ_FAST_ORD=table are byte-identical to the default, each setting in a fresh child process."""
import os
import subprocess
import sys

import pytest

import _stepcases as sc

pytestmark = pytest.mark.gpu

CASES = sc.path_cases()


@pytest.fixture(scope="module")
def run():
    from orz_amd import _native

    lib = _native.load()
    if lib.orz_device_count() <= 0:
        pytest.fail("GPU test selected but liborz_hip.so found no HIP device (no CPU fallback exists)")
    return sc.Runner(lib, gpu=True)


def test_the_references_reach_every_listed_class():
    facts = [sc.reference_of(c)[1] for c in CASES + [sc.large_case()]]
    gaps = sc.coverage_gaps(facts)
    assert not gaps, "\n".join(gaps)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_path_stage_equals_the_walk(run, k):
    sc.check_path(run, CASES[k], forms=(sc.FUSED, (sc.UNFUSED, sc.PLAIN, sc.FUSED)[k % 3])[:1 + (k % 3 != 2)], count_too=k % 4 == 0)


def test_path_stage_on_640_chunks_walks_global_memory(run):
    case = sc.large_case()
    assert sc.tile_down_lds(case["n"], case["tile"], case["t_lo"], case["t_hi"]) == 0
    assert (640 + 5) * sc.ENT + 16 > sc.LDS_MAX
    sc.check_path(run, case, forms=(sc.FUSED,), count_too=False)


@pytest.mark.parametrize("s0,s1,ext,cpt,live_end", sc.prefix_cases())
def test_prefix_alone_and_fused(run, s0, s1, ext, cpt, live_end):
    sc.check_prefix(run, s0, s1, ext, cpt, live_end)


def test_ordinals_both_kernels(run):
    seen = [sc.check_ordinals(run, *case) for case in sc.ordinal_cases()]
    assert any(hot == sc.SUB and nctx == 1 for hot, nctx in seen), "no subtile of 4096 item starts in one context"
    assert any(nctx >= 8 for _, nctx in seen)


def test_horizons_alone_and_fused(run):
    sc.check_horizon(run)


def test_refusals(run):
    sc.check_refusals(run)


_CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tools"))
import _stepcases as sc
import orz_amd
with sc.limit(300):
    enc = orz_amd.StreamEncoder(device=0, level=1, mode="fast", tile_bytes=65536)
try:
    for name, data in sorted(sc.encode_inputs().items()):
        with sc.limit(300):
            out = enc.encode(data)
        print(name, len(data), len(out), hashlib.sha256(out).hexdigest())
finally:
    enc.close()
"""


def test_whole_encodes_are_identical_under_the_switches(run):
    """ORZ_FAST_FUSED=0 (every kernel of a step a launch of its own) and ORZ_FAST_ORD=table (OrdWave for OrdWave2) against the
    default: 1 MiB units, tile 65536.  One child after the other; a child that fails ends the test before the next one starts."""
    outs = {}
    for name, env in sc.SWITCHES.items():
        e = dict(os.environ, ORZ_FAST_UNIT=str(1 << 20), **env)
        for k in ("ORZ_FAST_FUSED", "ORZ_FAST_ORD"):
            if k not in env:
                e.pop(k, None)
        p = subprocess.run([sys.executable, "-c", _CHILD, sc.ROOT], env=e, capture_output=True, text=True, timeout=700)
        assert p.returncode == 0, (name, p.stderr[-2000:])
        outs[name] = p.stdout
    assert len(outs["default"].splitlines()) == 2
    assert outs["unfused"] == outs["default"], (outs["unfused"], outs["default"])
    assert outs["ord_table"] == outs["default"], (outs["ord_table"], outs["default"])
