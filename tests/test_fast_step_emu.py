"""CPU tier: the step machinery of the fast parse's round loop -- fast_decide / FastDecide, PathUpWave, PathTileDown, PathMarkWave
(and the thread-per-item forms PathSeg, PathChunk, PathMark), CountWave, FastPrefix alone and inside FlipPrefixWave, FastItemTotal,
OrdWave, OrdWave2, FastHorizon alone and inside RetireHorizonWave -- run ONCE each by the emulation twin of the library's
stand-alone entry points (tests/emu/emu_fast_step.cpp, the same launches as orz_fast_step_*) and held entry for entry to the
serial references of tests/_stepcases.py, which share no code with the kernels.  Arrays go in poisoned: what a kernel must leave
alone has to come back as it went in.  And whole encodes under the two experiment switches that select second forms of the same
work are byte-identical to the default, each setting in a process of its own (the switches are read once per process)."""
import hashlib
import os
import subprocess
import sys

import pytest

import _stepcases as sc

CASES = sc.path_cases()


@pytest.fixture(scope="module")
def run():
    return sc.Runner(sc.emu_lib())


def test_the_references_reach_every_listed_class():
    """asserted on the references alone, before anything runs: exit offsets 0 and 239 in each map, segments with 0 and 64 item
    starts, every short last chunk, a tile tail jumped over, both variants of PathTileDown, the lazy thresholds, ..."""
    facts = [sc.reference_of(c)[1] for c in CASES + [sc.large_case()]]
    gaps = sc.coverage_gaps(facts)
    assert not gaps, "\n".join(gaps)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_path_stage_equals_the_walk(run, case):
    sc.check_path(run, case)


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
import ctypes, hashlib, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, os.path.join(sys.argv[1], "tools"))
import _stepcases as sc
lib = ctypes.CDLL(os.path.join(sys.argv[1], "build", "libemu.so"))
for name, data in sorted(sc.encode_inputs().items()):
    dst, n, st = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(), (ctypes.c_ulonglong * 5)()
    assert lib.emu_encode_fast(data, ctypes.c_size_t(len(data)), 15, 9, 6, 65536, 0, ctypes.byref(dst), ctypes.byref(n), st) == 0
    print(name, len(data), n.value, hashlib.sha256(ctypes.string_at(dst, n.value)).hexdigest())
"""


def test_whole_encodes_are_identical_under_the_switches(emu):
    """ORZ_FAST_FUSED=0 (every kernel of a step a launch of its own: FastDecide + PathUpWave, FastFlip, FastPrefix, FastHorizon,
    FastRetire + FastRetireDone) and ORZ_FAST_ORD=table (OrdWave for OrdWave2) against the default: 1 MiB units, tile 65536"""
    procs = {}
    for name, env in sc.SWITCHES.items():
        e = dict(os.environ, ORZ_FAST_UNIT=str(1 << 20), **env)
        for k in ("ORZ_FAST_FUSED", "ORZ_FAST_ORD"):
            if k not in env:
                e.pop(k, None)
        procs[name] = subprocess.Popen([sys.executable, "-c", _CHILD, sc.ROOT], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    outs = {}
    for name, p in procs.items():
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, (name, err[-2000:])
        outs[name] = out
    assert len(outs["default"].splitlines()) == 2
    assert outs["unfused"] == outs["default"], (outs["unfused"], outs["default"])
    assert outs["ord_table"] == outs["default"], (outs["ord_table"], outs["default"])
