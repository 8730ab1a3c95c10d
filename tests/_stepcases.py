"""Shared by the two tiers of the fast parse's step tests (test_fast_step_emu.py, test_gpu_fast_step.py): the step machinery of
the round loop (orz_fast.h: decisions, path maps, entries, marks, counts, prefixes, ordinals, ring horizons) restated in numpy and
plain Python FROM ITS DEFINITIONS -- walks, sums and linear scans, no code shared with the kernels --, the cases, the coverage the
cases must reach, and one face for the stand-alone entry points of the library (orz_fast_step_*) and of the emulation twin
(tests/emu/emu_fast_step.cpp).  Positions are block offsets i here: window offset = KPRE + i."""
import contextlib
import ctypes
import faulthandler
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPRE = ((1 << 25) - 1) // 2
SUB, SEG, ENT = 4096, 64, 240
MINLEN, MAXLEN = 4, 240
TY_WORD, TY_LIT, TY_MATCH = 0, 1, 2
KHISTSUB = (KPRE + 1) // SUB
RING_LIMITS = (4094 - 4, 510)     # kRing - kRingMargin, and the offsets that cost fewer than 8 bits
P8, P32, P64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
EINVAL = -22
FUSED, UNFUSED, PLAIN = 0, 1, 2
LDS_MAX = 144 * 1024              # PathTileDown::kLdsMax


class Sizes:
    """entries of the arrays of a call (include/orz_hip.h)"""

    def __init__(self, n, tile):
        self.nsub = (n + SUB - 1) // SUB
        self.ntile = (n + tile - 1) // tile if tile else 0
        self.pos = n + SUB + 512
        self.x1 = (self.nsub + 2) * ENT
        self.x2 = (self.ntile + 2) * ENT
        self.centry = self.nsub + 2
        self.tentry = self.ntile + 2
        self.sbits = n // 64 + 16
        self.cm = (self.nsub + 2) * 256
        self.ev = n + 8 + 512


def tile_down_lds(n, tile, t_lo, t_hi):
    """what PathTileDown needs in LDS for the chunk and tile maps of the range, 0 = more than it may have (the walk in global memory)"""
    hi = min(n, (t_hi + 1) * tile)
    nch = (hi - t_lo * tile + SUB - 1) // SUB
    need = (nch + (t_hi - t_lo + 1)) * ENT + 16
    return need if need <= LDS_MAX else 0


# ------------------------------------------------------------------------------------------------ the two libraries
def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_fast_step.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_fast_step.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    return ctypes.CDLL(so)


@contextlib.contextmanager
def limit(seconds):
    """a step that is still running after `seconds` ends the whole process (a hung device call cannot be interrupted from Python)"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class Runner:
    """the three entry points of the emulation twin (lib = emu_lib()) or of the product library (lib = orz_amd._native.load(),
    gpu=True): numpy arrays in, (rc, arrays) out"""

    def __init__(self, lib, gpu=False):
        self.lib, self.gpu = lib, gpu
        self.err = ctypes.create_string_buffer(256)

    def _call(self, name, args):
        u32 = ctypes.c_uint32
        args = [u32(a) if isinstance(a, (int, np.integer)) and not isinstance(a, bool) else a for a in args]
        if self.gpu:
            with limit(120):                      # (every device step under a time limit of its own)
                return getattr(self.lib, "orz_" + name)(0, *args)
        return getattr(self.lib, "emu_" + name)(*args, self.err, ctypes.c_size_t(256))

    def path(self, case, form, poison=True, ev=None, tile=None, entry=None):
        """the path stage on a case: rc, {name: array}"""
        n, tile = case["n"], case["tile"] if tile is None else tile
        z = Sizes(n, tile if tile else SUB)
        out = {k: np.full(z.pos, P8, np.uint8) for k in ("ty", "nl", "x0", "pt")}
        out["x1"] = np.full(z.x1, P8, np.uint8)
        out["x2"] = np.full(z.x2, P8, np.uint8)
        out["centry"] = np.full(z.centry, P32, np.uint32)
        out["tentry"] = np.full(z.tentry, P32, np.uint32)
        out["sbits"] = np.full(z.sbits, P64, np.uint64)
        out["cm"] = np.full(z.cm, P32, np.uint32)
        lds = ctypes.c_uint64(1)
        ev = case["ev"] if ev is None else ev
        entry = KPRE + case["entry"] if entry is None else entry
        args = [ctypes.c_uint(form), n, tile, case["t_lo"], case["t_hi"], entry, _p(case["wbytes"]), _p(ev)]
        args += [_p(out[k]) for k in ("ty", "nl", "x0", "x1", "x2", "centry", "tentry", "sbits", "pt", "cm")] + [ctypes.byref(lds)]
        rc = self._call("fast_step_path", args)
        out["lds"] = lds.value
        return rc, out

    def counts(self, n, wbytes, sbits, count, s0, s1, ext, cpt, live_end, rows, cm, cp0):
        """cm: [rows][256] or None (poison: CountWave writes it); cp0: row s0 of cp"""
        cm = np.full(rows * 256, P32, np.uint32) if cm is None else np.ascontiguousarray(cm, np.uint32).reshape(-1).copy()
        cp = np.full((rows + 1) * 256, P32, np.uint32)
        cp[s0 * 256:(s0 + 1) * 256] = cp0
        cp2 = cp.copy()
        o1, o2 = np.full(n, P32, np.uint32), np.full(n, P32, np.uint32)
        acc = np.zeros(2, np.uint32)
        rc = self._call("fast_step_counts", [n, _p(wbytes), _p(sbits), ctypes.c_int(count), s0, s1, ext, cpt, live_end, rows, _p(cm), _p(cp),
                                             _p(cp2), _p(o1), _p(o2), _p(acc)])
        return rc, {"cm": cm.reshape(rows, 256), "cp": cp.reshape(rows + 1, 256), "cp2": cp2.reshape(rows + 1, 256), "ord": o1, "ord2": o2,
                    "acc": int(acc[0]), "hotacc": int(acc[1])}

    def horizon(self, cp, hpre, s0, s1, hz0):
        cp = np.ascontiguousarray(cp, np.uint32)
        hpre = np.ascontiguousarray(hpre, np.uint32)
        hz, hz2 = hz0.copy(), hz0.copy()
        rc = self._call("fast_step_horizon", [_p(cp), cp.shape[0], _p(hpre), s0, s1, _p(hz), _p(hz2)])
        return rc, hz, hz2


# ------------------------------------------------------------------------------------------------ decisions
def pack_ev(n, L, lz1, lz2, lwm, ro):
    """ev as FastEval leaves it: best length | lazy-1 answer << 8 | lazy-2 answer << 16 | last word matched << 24 | robitlen < 8 << 25;
    behind the block 0xFFFFFFFF (nothing there may count)"""
    ev = np.full(Sizes(n, SUB).ev, 0xFFFFFFFF, np.uint32)
    ev[:n] = (np.asarray(L, np.uint32) | (np.asarray(lz1, np.uint32) << 8) | (np.asarray(lz2, np.uint32) << 16)
              | (np.asarray(lwm, np.uint32) << 24) | (np.asarray(ro, np.uint32) << 25))
    return ev


def decide(ev, n):
    """LZEncoder::encode's choice at every position (reference src/lz.rs:139-234) on the snapshot's answers, with the end clip
    (src/matcher.rs:183: an item ends before the block end -- a longer match is cut to that, and is none below MINLEN).
    Returns (type, advance, lazy id, l1, l2) per position."""
    e = ev[:n].astype(np.int64)
    i = np.arange(n)
    m_len = e & 0xff
    m_len = np.where(i + m_len >= n, n - 1 - i, m_len)          # pos + match_len < buf.len()
    m_len = np.where(m_len < MINLEN, 0, m_len)
    last_word_matched = (e >> 24) & 1
    short_robits = (e >> 25) & 1                                 # robitlen < 8
    ans1 = np.zeros(n, np.int64)                                 # has_lazy_match(spos, ...): what spos + 1 offers at lazy depth 1
    ans1[:-1] = (e[1:] >> 8) & 0xff
    ans2 = np.zeros(n, np.int64)                                 # has_lazy_match(spos + 1, ...): what spos + 2 offers at lazy depth 2
    if n > 2:
        ans2[:-2] = (e[2:] >> 16) & 0xff
    lazy_len1 = m_len + 1 + short_robits
    lazy_len2 = lazy_len1 - last_word_matched
    looks = (m_len > 0) & (m_len < MAXLEN // 2)
    lazy_id = np.zeros(n, np.int64)
    lazy_id[looks & (ans1 >= lazy_len1)] = 1
    lazy_id[looks & (lazy_id == 0) & (ans2 >= lazy_len2)] = 2
    is_match = (m_len > 0) & (lazy_id == 0)
    is_word = ~is_match & (i + 1 < n) & (lazy_id != 1) & (last_word_matched == 1)
    ty = np.where(is_match, TY_MATCH, np.where(is_word, TY_WORD, TY_LIT))
    adv = np.where(is_match, m_len, np.where(is_word, 2, 1))
    return ty, adv, lazy_id, np.where(looks, lazy_len1, 0), np.where(looks, lazy_len2, 0), ans1, ans2


def ctx_at(wbytes, i):
    """hash1 of the position before item start i (wbytes[0] is the byte two before the block)"""
    b1 = wbytes[np.asarray(i) + 1].astype(np.int64)
    b2 = wbytes[np.asarray(i)].astype(np.int64)
    alnum = ((b2 >= 48) & (b2 <= 57)) | ((b2 >= 65) & (b2 <= 90)) | ((b2 >= 97) & (b2 <= 122))
    return (b1 & 0x7f) | (alnum.astype(np.int64) << 7)


# ------------------------------------------------------------------------------------------------ the path
def walk_exits(adv, starts, ends):
    """where a walk x += adv[x] from each start first reaches or passes its end, as an offset past the end (a start at or beyond
    the end has left already)"""
    x = np.asarray(starts, np.int64).copy()
    ends = np.asarray(ends, np.int64)
    idx = np.nonzero(x < ends)[0]
    while idx.size:
        x[idx] += adv[x[idx]]
        idx = idx[x[idx] < ends[idx]]
    return x - ends


def path_reference(case):
    """every output of the path stage: {name: (expected array with poison where nothing is defined)} plus the facts the coverage
    test reads"""
    n, T, t_lo, t_hi = case["n"], case["tile"], case["t_lo"], case["t_hi"]
    z = Sizes(n, T)
    ty, adv, lazy_id, l1, l2, a1, a2 = decide(case["ev"], n)
    lo, hi = t_lo * T, min(n, (t_hi + 1) * T)
    want = {k: np.full(z.pos, P8, np.uint8) for k in ("ty", "nl", "x0", "pt")}
    want["ty"][lo:hi] = ty[lo:hi]
    want["nl"][lo:hi] = adv[lo:hi]
    pos = np.arange(lo, hi)
    seg_end = np.minimum(n, (pos // SEG + 1) * SEG)
    want["x0"][lo:hi] = walk_exits(adv, pos, seg_end)
    c0, c1 = lo // SUB, (hi + SUB - 1) // SUB                                    # chunks of the range
    want["x1"] = np.full(z.x1, P8, np.uint8)
    cc = np.repeat(np.arange(c0, c1), ENT)
    ee = np.tile(np.arange(ENT), c1 - c0)
    x1 = walk_exits(adv, cc * SUB + ee, np.minimum(n, (cc + 1) * SUB))
    want["x1"][c0 * ENT:c1 * ENT] = x1
    want["x2"] = np.full(z.x2, P8, np.uint8)
    tt = np.repeat(np.arange(t_lo, t_hi + 1), ENT)
    ee = np.tile(np.arange(ENT), t_hi + 1 - t_lo)
    x2 = walk_exits(adv, tt * T + ee, np.minimum(n, (tt + 1) * T))
    want["x2"][t_lo * ENT:(t_hi + 1) * ENT] = x2
    # the path: x = entry; while x < hi: x += adv[x]
    path, x = [], case["entry"]
    adv_l = adv.tolist()
    while x < hi:
        path.append(x)
        x += adv_l[x]
    exit_at = x
    stops = np.array(path + [exit_at], np.int64)                                 # ascending
    first_at = lambda start: int(stops[np.searchsorted(stops, start)])
    want["centry"] = np.full(z.centry, P32, np.uint32)
    for c in range(c0, c1):
        want["centry"][c] = KPRE + first_at(c * SUB)
    want["tentry"] = np.full(z.tentry, P32, np.uint32)
    want["tentry"][t_lo] = KPRE + case["entry"]                                  # (given)
    for t in range(t_lo + 1, t_hi + 1):
        want["tentry"][t] = KPRE + first_at(t * T)
    want["tentry"][t_hi + 1] = KPRE + exit_at                                    # the exit of the range
    path = np.array(path, np.int64)
    bits = np.zeros(z.sbits * 64, np.uint8)
    bits[path] = 1
    words = np.packbits(bits.reshape(-1, 64)[:, ::-1], axis=1).view(">u8").reshape(-1).astype(np.uint64)
    want["sbits"] = np.full(z.sbits, P64, np.uint64)
    want["sbits"][lo // 64:(hi + 63) // 64] = words[lo // 64:(hi + 63) // 64]
    want["pt"][path + adv[path]] = ty[path]
    want["cm"] = np.full(z.cm, P32, np.uint32)
    cm = np.bincount((path // SUB) * 256 + ctx_at(case["wbytes"], path), minlength=z.cm) if path.size else np.zeros(z.cm, np.int64)
    want["cm"][c0 * 256:c1 * 256] = cm[c0 * 256:c1 * 256]
    starts_per_seg = np.bincount(path // SEG, minlength=(hi + SEG - 1) // SEG)[lo // SEG:] if path.size else np.zeros(1, np.int64)
    facts = {
        "x0": set(want["x0"][lo:hi].tolist()), "x1": set(x1.tolist()), "x2": set(x2.tolist()),
        "seg_starts": set(starts_per_seg.tolist()),
        "last_chunk": n - (c1 - 1) * SUB if hi == n else SUB,
        "entry_off": case["entry"] - lo, "entry_beyond": case["entry"] >= hi,
        "lds": tile_down_lds(n, T, t_lo, t_hi) != 0,
        "tail_jumped": hi == n and n % T not in (0, 1) and t_hi > t_lo and first_at(t_hi * T) == n - 1,
        "ev_past_end": bool(np.all(case["ev"][n:] == 0xFFFFFFFF)),
        "lazy": set(), "ctxs": int(np.unique(ctx_at(case["wbytes"], path)).size) if path.size else 0, "tiles": t_hi - t_lo + 1, "t_lo": t_lo,
    }
    r = slice(lo, hi)
    look = l1[r] > 0
    for name, hit in (("l1_exact", look & (a1[r] == l1[r])), ("l1_below", look & (a1[r] == l1[r] - 1) & (lazy_id[r] != 1)),
                      ("l2_exact", look & (lazy_id[r] == 2) & (a2[r] == l2[r])), ("l2_below", look & (lazy_id[r] == 0) & (a2[r] == l2[r] - 1)),
                      ("l2_differs_from_l1", look & (l1[r] != l2[r]) & (lazy_id[r] == 0) & (a2[r] == l2[r] - 1))):
        if hit.any():
            facts["lazy"].add(name)
    e = case["ev"][:n].astype(np.int64)
    Lraw = (e & 0xff)[r]
    if ((Lraw == 119) & (lazy_id[r] == 1)).any(): facts["lazy"].add("look119")
    if ((Lraw == 120) & (a1[r] >= 122) & (ty[r] == TY_MATCH)).any(): facts["lazy"].add("look120")
    if hi == n:
        i = np.arange(lo, hi)
        lw = ((e >> 24) & 1)[r]
        if n >= 2 and lo <= n - 2 and lw[n - 2 - lo] and ty[n - 2] == TY_WORD: facts["lazy"].add("word_at_len-2")
        if lw[n - 1 - lo] and ty[n - 1] == TY_LIT: facts["lazy"].add("word_at_len-1")
        if ((Lraw >= MINLEN) & (i + Lraw >= n) & (n - 1 - i == 3) & (ty[r] != TY_MATCH)).any(): facts["lazy"].add("clip3")
        if ((Lraw > MINLEN) & (i + Lraw >= n) & (n - 1 - i == 4) & (ty[r] == TY_MATCH) & (adv[r] == 4)).any(): facts["lazy"].add("clip4")
    return want, facts


def x0_tail_mask(case):
    """PathUpWave stores x0 as whole 8-byte words: behind a block end that is no multiple of 8 the rest of the last word is written
    (from LDS nobody filled; no kernel reads x0 there).  Those entries are not held to anything -- in the wave forms only."""
    n = case["n"]
    hi = min(n, (case["t_hi"] + 1) * case["tile"])
    return slice(n, (n + 7) // 8 * 8) if hi == n else slice(0, 0)


# ------------------------------------------------------------------------------------------------ path cases
def fam_lit(rng, n):
    z = np.zeros(n, np.int64)
    return z, z, z, z, z


def fam_m240(rng, n):
    z = np.zeros(n, np.int64)
    return z + 240, z, z, z, z


def fam_word(rng, n):
    z = np.zeros(n, np.int64)
    return z, z, z, z + 1, z


def fam_mix(rng, n, p_lit=0.35):
    """literals, words, short and long matches, lazy answers of every size"""
    kind = rng.random(n)
    L = np.where(kind < p_lit, 0, np.where(kind < 0.9, rng.integers(4, 40, n), rng.integers(40, 241, n)))
    pick = lambda: np.where(rng.random(n) < 0.5, 0, np.where(rng.random(n) < 0.8, rng.integers(4, 40, n), rng.integers(4, 241, n)))
    return L, pick(), pick(), (rng.random(n) < 0.3).astype(np.int64), (rng.random(n) < 0.5).astype(np.int64)


def fam_dense(rng, n):
    return fam_mix(rng, n, p_lit=0.03)


def fam_lazy(rng, n):
    """the lazy rules at their thresholds: the answers of p + 1 / p + 2 sit exactly at l1 / l2 of p, or one below"""
    L = np.where(rng.random(n) < 0.3, 0, rng.integers(5, 30, n))
    lwm = (rng.random(n) < 0.5).astype(np.int64)
    ro = (rng.random(n) < 0.5).astype(np.int64)
    l1 = L + 1 + ro
    l2 = l1 - lwm
    lz1, lz2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    lz1[1:] = np.where(L[:-1] > 0, l1[:-1] - rng.integers(0, 2, n - 1), 0) if n > 1 else 0
    if n > 2:
        lz2[2:] = np.where(L[:-2] > 0, l2[:-2] - rng.integers(0, 2, n - 2), 0)
    # (mostly one below at lazy 1, so that lazy 2 gets its turn)
    if n > 1:
        lz1[1:] = np.where(rng.random(n - 1) < 0.6, np.where(L[:-1] > 0, l1[:-1] - 1, 0), lz1[1:])
    return L, lz1, lz2, lwm, ro


def fam_ends(which):
    """literals with the block end's special cases planted: `look` at 119 / 120, a WORD candidate at len - 2 and len - 1, a match
    the end clip leaves 4 (a) or 3 (b) of"""
    def make(rng, n):
        L, lz1, lz2, lwm, ro = (np.zeros(n, np.int64) for _ in range(5))
        if n >= 300:
            L[10], lz1[11] = 119, 240      # looks, and the lazy match wins
            L[20], lz1[21] = 120, 240      # does not look
        if which == "a":
            if n >= 6:
                L[n - 5] = 10              # clipped to 4: a match up to len - 1
            lwm[n - 1] = 1                 # a WORD candidate at len - 1 is a literal
        else:
            if n >= 5:
                L[n - 4] = 10              # clipped to 3: none
            if n >= 2:
                lwm[n - 2] = 1             # a WORD at len - 2 ends at the block end
        return L, lz1, lz2, lwm, ro
    return make


FAMILIES = {"lit": fam_lit, "m240": fam_m240, "word": fam_word, "mix": fam_mix, "dense": fam_dense, "lazy": fam_lazy,
            "ends_a": fam_ends("a"), "ends_b": fam_ends("b")}
NS = (1, 2, 7, 8, 9, 63, 64, 65, 239, 240, 241, 4095, 4096, 4097, 4096 + 239, 8192 + 1)
TILES = (4096, 8192, 12288)
_ALNUM = np.frombuffer(b" ae,.\x00\xffZ09", np.uint8)


def make_case(name, n, tile, t_lo, t_hi, entry_off, family, seed, const_bytes=False):
    rng = np.random.default_rng(seed)
    fields = FAMILIES[family](rng, n)
    wbytes = np.full(n + 2, ord("a"), np.uint8) if const_bytes else _ALNUM[rng.integers(0, _ALNUM.size, n + 2)] if seed % 2 else \
        rng.integers(0, 256, n + 2, dtype=np.uint8)
    return {"name": name, "n": n, "tile": tile, "t_lo": t_lo, "t_hi": t_hi, "entry": t_lo * tile + entry_off, "ev": pack_ev(n, *fields),
            "wbytes": np.ascontiguousarray(wbytes), "family": family}


def path_cases():
    """the small cases: every n of the issue's list at every family that can matter there, the three tiles with 1 to 4 active
    tiles and t_lo > 0, entries at 0, 239, and beyond a short range"""
    out, seed = [], 100
    fams = sorted(FAMILIES)
    for k, n in enumerate(NS):
        tile = TILES[k % 3] if n > 4096 else 4096
        ntile = (n + tile - 1) // tile
        for j, fam in enumerate(fams):
            seed += 1
            eo = (0, 239, 17)[(k + j) % 3]
            out.append(make_case("n%d_%s_e%d" % (n, fam, eo), n, tile, 0, ntile - 1, eo, fam, seed, const_bytes=(k + j) % 4 == 0))
    for tile in TILES:
        n = 5 * tile + 100
        ranges = [(0, 0), (0, 3), (1, 2), (2, 5), (3, 5), (5, 5), (4, 4)]
        for j, (t_lo, t_hi) in enumerate(ranges):
            for i, fam in enumerate(fams):
                if (i + j) % 2 and fam not in ("m240", "mix"):
                    continue                       # (half of the families per range, alternating)
                seed += 1
                eo = (0, 239, 101, 1)[(i + j) % 4]
                out.append(make_case("T%d_t%d-%d_%s_e%d" % (tile, t_lo, t_hi, fam, eo), n, tile, t_lo, t_hi, eo, fam, seed,
                                     const_bytes=(i + j) % 5 == 0))
    return out


def large_case():
    """640 chunks at a tile of 524288, five tiles active: the maps do not fit PathTileDown's LDS, its walk runs in global memory"""
    tile = 524288
    return make_case("large_640_chunks", 5 * tile, tile, 0, 4, 239, "dense", 7)


def coverage_gaps(facts_list):
    """the classes of the issue that the references of the path cases do not reach (empty = all are there)"""
    gaps = []
    have = lambda f: any(f(x) for x in facts_list)
    for m in ("x0", "x1", "x2"):
        for off in (0, 239):
            if not have(lambda x: off in x[m]):
                gaps.append("no exit offset %d in %s" % (off, m))
    for k in (0, 64):
        if not have(lambda x: k in x["seg_starts"]):
            gaps.append("no segment with %d item starts" % k)
    for ln in (1, 7, 9) + tuple(n % SUB for n in NS if n % SUB):
        if not have(lambda x: x["last_chunk"] == ln):
            gaps.append("no short last chunk of %d positions" % ln)
    for eo in (0, 239):
        if not have(lambda x: x["entry_off"] == eo):
            gaps.append("no entry offset %d" % eo)
    if not have(lambda x: x["entry_beyond"]):
        gaps.append("no entry beyond a short range")
    if not have(lambda x: x["tail_jumped"]):
        gaps.append("no short last tile whose positions an item jumps over")
    if not have(lambda x: x["lds"]) or not have(lambda x: not x["lds"]):
        gaps.append("not both variants of PathTileDown")
    if not all(x["ev_past_end"] for x in facts_list):
        gaps.append("ev is not 0xFFFFFFFF past the block end everywhere")
    for k in range(1, 5):
        if not have(lambda x: x["tiles"] == k):
            gaps.append("no range of %d tiles" % k)
    if not have(lambda x: x["t_lo"] > 0):
        gaps.append("no range with t_lo > 0")
    if not have(lambda x: x["ctxs"] == 1) or not have(lambda x: x["ctxs"] > 8):
        gaps.append("not both one context and many")
    for name in ("l1_exact", "l1_below", "l2_exact", "l2_below", "l2_differs_from_l1", "look119", "look120", "word_at_len-2", "word_at_len-1",
                 "clip3", "clip4"):
        if not have(lambda x: name in x["lazy"]):
            gaps.append("no decision of the class %s" % name)
    return gaps


# ------------------------------------------------------------------------------------------------ prefix, ordinals
def prefix_reference(cm, cp_s0, s0, s1, ext, cpt, live_end, rows):
    """cp[s + 1] = cp[s0] + the sum over u in [s0, s] of: the subtile's own count below live_end; behind it the count of the same
    place in the newest tile (cpt subtiles) below live_end, or nothing where there is no such subtile.  Rows outside (s0, s1 + ext]:
    poison."""
    cm = np.asarray(cm, np.int64).reshape(-1, 256)
    want = np.full((rows + 1, 256), P32, np.int64)
    want[s0] = cp_s0
    run = np.asarray(cp_s0, np.int64).copy()
    for u in range(s0, s1 + ext):
        if u < live_end:
            run = run + cm[u]
        else:
            place = live_end - cpt + (u - live_end) % cpt
            if place >= 0:
                run = run + cm[place]
        want[u + 1] = run & 0xFFFFFFFF
    return want.astype(np.uint32)


def prefix_cases():
    out = []
    for total in (1, 63, 64, 65, 129):
        for cpt in (1, 3, 64):
            for s0 in (0, 3):
                ext = min(cpt + 1, total - 1)
                s1 = s0 + total - ext
                for live_end in sorted({s0, (s0 + s1) // 2, s1}):
                    out.append((s0, s1, ext, cpt, live_end))
    return out


def bits_to_words(bits):
    bits = np.asarray(bits, np.uint8)
    pad = (-bits.size) % 64
    bits = np.concatenate([bits, np.zeros(pad, np.uint8)])
    return np.packbits(bits.reshape(-1, 64)[:, ::-1], axis=1).view(">u8").reshape(-1).astype(np.uint64)


def ordinal_reference(n, wbytes, sbits, cp):
    """ORD of every set bit below n: cp[subtile][ctx] + the earlier item starts of that subtile with the same ctx; poison elsewhere"""
    want = np.full(n, P32, np.uint32)
    seen = {}
    for i in range(n):
        if (int(sbits[i // 64]) >> (i % 64)) & 1:
            key = (i // SUB, int(ctx_at(wbytes, i)))
            want[i] = (int(cp[key[0]][key[1]]) + seen.get(key, 0)) & 0xFFFFFFFF
            seen[key] = seen.get(key, 0) + 1
    return want


def ordinal_cases():
    """(name, n, wbytes, sbits with stale bits set behind n)"""
    out = []
    rng = np.random.default_rng(5)
    one_bit = np.frombuffer(b"\x20\x21\x22\x24\x28\x30\x60\x00a!", np.uint8)     # contexts that differ in exactly one bit
    for name, n, dens, const in (("one_ctx_all_starts", 2 * SUB, 1.0, True), ("n%64=1", SUB + 1, 0.6, False), ("n%64=63", 2 * SUB + 63, 0.4, False),
                                 ("n%64=0_sparse", SUB + 64, 0.05, False), ("tiny", 1, 1.0, False)):
        z = Sizes(n, SUB)
        bits = (rng.random(z.sbits * 64) < dens).astype(np.uint8)
        bits[n:] = 1                                                             # stale bits behind the block
        wb = np.full(n + 2, ord("a"), np.uint8) if const else one_bit[rng.integers(0, one_bit.size, n + 2)]
        out.append((name, n, np.ascontiguousarray(wb), bits_to_words(bits)))
    return out


# ------------------------------------------------------------------------------------------------ horizons
def horizon_reference(cp, hpre, s, c, limit):
    """The oldest window offset from which at most `limit` item starts of the context lie before the middle of subtile s's own
    (orz_fast.h, above FastHorizon), by linear scans: (horizon, facts)"""
    col = cp[:s + 2, c].astype(np.int64).tolist()
    end = col[s] + (col[s + 1] - col[s]) // 2
    base = col[0]
    facts = set()
    if end - base == limit: facts.add("eq_limit")
    if end - base == limit + 1: facts.add("eq_limit+1")
    if end - base > limit:
        lo = next(k for k in range(s + 2) if col[k] >= end or end - col[k] <= limit)
        if col[lo] < end and end - col[lo] == limit: facts.add("inner_eq")
        h = KPRE + lo * SUB
        if lo:
            room = limit - (0 if col[lo] >= end else end - col[lo])
            m = col[lo] - col[lo - 1]
            if m:
                h -= min(room, m) * SUB // m
        if lo <= s and col[lo + 1] == col[lo]: facts.add("empty_boundary")       # the subtile at the boundary holds no item start
        if col[s + 1] == col[s]: facts.add("empty_self")
        return h, facts
    facts.add("history")
    hc = hpre[:, c].astype(np.int64)
    room, tot = limit - (end - base), int(hc[KHISTSUB])
    lo = int(np.nonzero(tot - hc <= room)[0][0])                                 # the smallest unified subtile from which the rest fits
    hc = hc[:lo + 1].tolist()
    if lo == 0:
        facts.add("whole_history")
        return 1, facts
    if lo == 1: facts.add("first_history_subtile")
    h = lo * SUB - 1
    left = room - (tot - hc[lo])
    m = hc[lo] - hc[lo - 1]
    if m:
        h -= min(left, m) * SUB // m
    if h <= 1:
        facts.add("clamp")
    return max(h, 1), facts


def horizon_case():
    """ONE call: every context column is a scenario of its own.  Returns cp [rows][256], hpre [KHISTSUB + 1][256], s0, s1."""
    rng = np.random.default_rng(11)
    s0, s1 = 2, 44
    rows = s1 + 2
    cm = rng.integers(0, 300, (rows - 1, 256))                                   # item starts per (subtile, ctx)
    cm[:, 128:192] = rng.integers(0, 40, (rows - 1, 64))                         # quiet contexts: their horizons lie in the history
    hcm = np.zeros((KHISTSUB, 256), np.int64)
    hcm[-64:] = rng.integers(0, 200, (64, 256))                                  # the history's newest subtiles
    hcm[:, 200:256] = 0
    hcm[:3, 200:256] = rng.integers(1, 50, (3, 56))                              # all of it in the first subtiles
    base = rng.integers(0, 1 << 20, 256)
    col = 0
    for limit in RING_LIMITS:
        # end - base == limit at subtile 30 (history branch, room 0) / limit + 1 (new region)
        for extra in (0, 1):
            cm[:, col] = 0
            cm[20:30, col] = limit // 10 - 10
            cm[30, col] = 2 * (limit - 10 * (limit // 10 - 10)) + 2 * extra
            col += 1
        # the same, with item starts at subtile 5 in front: end - cp[6 .. 20] == limit inside the new region
        cm[:, col] = 0
        cm[5, col] = 50
        cm[20:30, col] = limit // 10 - 10
        cm[30, col] = 2 * (limit - 10 * (limit // 10 - 10))
        col += 1
        # an empty subtile at the boundary of the new-region search
        cm[:, col] = 0
        cm[3, col] = limit + 5
        cm[10, col] = 7
        col += 1
    # history: everything inside the first history subtile -- 4091 and 511 item starts there leave the interpolation at h = 1, where
    # the clamp stands (left < m always, so with both limits below 4096 no horizon can come out BELOW 1: equality is its edge)
    for m in (4091, 511, 8192):
        hcm[:, col] = 0; hcm[0, col] = m; cm[:, col] = 0; col += 1
    hcm[:, col] = 0; hcm[0, col] = 100; cm[:, col] = 0; col += 1                # the whole history fits
    hcm[:, col] = 0; hcm[7, col] = 100; hcm[9, col] = 5000; cm[:, col] = 0; col += 1   # an empty history subtile below the boundary
    cp = np.zeros((rows, 256), np.int64)
    cp[0] = base
    cp[1:] = base + np.cumsum(cm, axis=0)
    hpre = np.zeros((KHISTSUB + 1, 256), np.int64)
    hpre[1:] = np.cumsum(hcm, axis=0)
    return (cp & 0xFFFFFFFF).astype(np.uint32), hpre.astype(np.uint32), s0, s1


def horizon_gaps(facts_by_limit):
    gaps = []
    for limit, facts in facts_by_limit.items():
        for f in ("eq_limit", "eq_limit+1", "inner_eq", "empty_boundary", "empty_self", "history", "whole_history", "first_history_subtile"):
            if f not in facts:
                gaps.append("no horizon of the class %s at limit %d" % (f, limit))
    if not any("clamp" in f for f in facts_by_limit.values()):
        gaps.append("no horizon at which the h > 1 clamp stands")
    return gaps


# ------------------------------------------------------------------------------------------------ whole encodes
def encode_inputs():
    import _data

    return {"mixed": _data.mixed(1_000_000, seed=31), "zeros_noise": _data.zeros_noise(300_000)}


SWITCHES = {"default": {}, "unfused": {"ORZ_FAST_FUSED": "0"}, "ord_table": {"ORZ_FAST_ORD": "table"}}


# ------------------------------------------------------------------------------------------------ the checks of both tiers
def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size, "%s: %d entries, expected %d" % (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s differs at %d entries, first at %d: got %d, expected %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


_REFS = {}


def reference_of(case):
    if case["name"] not in _REFS:
        _REFS[case["name"]] = path_reference(case)
    return _REFS[case["name"]]


PATH_ARRAYS = ("ty", "nl", "x0", "x1", "x2", "centry", "tentry", "sbits", "pt", "cm")


def check_path(run, case, forms=(FUSED, UNFUSED, PLAIN), count_too=True):
    """every form of the path stage == the reference, entry for entry, poison included; CountWave on the marks == PathMarkWave's cm"""
    want, _ = reference_of(case)
    for form in forms:
        rc, got = run.path(case, form)
        assert rc == 0, "form %d: rc %d" % (form, rc)
        assert got["lds"] == tile_down_lds(case["n"], case["tile"], case["t_lo"], case["t_hi"])
        for k in PATH_ARRAYS:
            g, w = got[k], want[k]
            if k == "x0" and form != PLAIN:
                g, w = g.copy(), w.copy()
                g[x0_tail_mask(case)] = P8
            same(g, w, "%s, form %d: %s" % (case["name"], form, k))
    if count_too:
        n, z = case["n"], Sizes(case["n"], case["tile"])
        rc, got = run.path(case, FUSED)
        rc2, cnt = run.counts(n, case["wbytes"], got["sbits"], 1, 0, z.nsub, 0, 1, z.nsub, z.nsub, None, np.zeros(256, np.uint32))
        assert rc == 0 and rc2 == 0
        c0, c1 = case["t_lo"] * case["tile"] // SUB, (min(n, (case["t_hi"] + 1) * case["tile"]) + SUB - 1) // SUB
        same(cnt["cm"][c0:c1], got["cm"].reshape(-1, 256)[c0:c1], "%s: CountWave's counts against PathMarkWave's" % case["name"])


def check_prefix(run, s0, s1, ext, cpt, live_end):
    rng = np.random.default_rng(s0 * 1000003 + s1 * 1009 + ext * 31 + cpt * 7 + live_end)
    rows = s1 + ext
    cm = rng.integers(1, 5000, (rows, 256)).astype(np.uint32)
    cp0 = rng.integers(0, 1 << 31, 256).astype(np.uint32)
    n = 64                                                                       # (one subtile of item starts: the ordinals are not the subject)
    wb = np.full(n + 2, 97, np.uint8)
    sbits = np.zeros(Sizes(n, SUB).sbits, np.uint64)
    rc, got = run.counts(n, wb, sbits, 0, s0, s1, ext, cpt, live_end, rows, cm, cp0)
    assert rc == 0
    want = prefix_reference(cm, cp0, s0, s1, ext, cpt, live_end, rows)
    what = "s0 %d s1 %d ext %d cpt %d live_end %d" % (s0, s1, ext, cpt, live_end)
    same(got["cp"], want, "FastPrefix alone, " + what)
    same(got["cp2"], want, "FastPrefix inside FlipPrefixWave, " + what)
    same(got["cm"], cm, "cm (read only), " + what)


def check_ordinals(run, name, n, wbytes, sbits):
    z = Sizes(n, SUB)
    cp0 = np.random.default_rng(n).integers(0, 1 << 20, 256).astype(np.uint32)
    rc, got = run.counts(n, wbytes, sbits, 1, 0, z.nsub, 0, 1, z.nsub, z.nsub, None, cp0)
    assert rc == 0
    live = np.zeros(z.sbits * 64, np.uint8)
    live[:n] = 1
    mine = np.array([(int(sbits[i // 64]) >> (i % 64)) & 1 for i in range(n)], np.int64)
    pos = np.nonzero(mine)[0]
    cm = np.bincount((pos // SUB) * 256 + ctx_at(wbytes, pos), minlength=z.nsub * 256).reshape(z.nsub, 256) if pos.size else np.zeros((z.nsub, 256))
    same(got["cm"], cm, name + ": CountWave")
    cp = prefix_reference(cm, cp0, 0, z.nsub, 0, 1, z.nsub, z.nsub)
    same(got["cp"], cp, name + ": cp")
    want = ordinal_reference(n, wbytes, sbits, cp)
    same(got["ord"], want, name + ": OrdWave")
    same(got["ord2"], want, name + ": OrdWave2")
    per_ctx = cm.sum(axis=0)
    assert got["acc"] == int(per_ctx.sum()) and got["hotacc"] == int(per_ctx.max()), (name, got["acc"], got["hotacc"])
    return int(cm.max()), int(np.count_nonzero(per_ctx))                        # the fullest (subtile, ctx), contexts in use


def check_horizon(run):
    cp, hpre, s0, s1 = horizon_case()
    hz0 = np.random.default_rng(3).integers(0, 1 << 32, (s1 + 1) * 256 * 4, dtype=np.uint64).astype(np.uint32)
    want = hz0.copy().reshape(s1 + 1, 256, 4)
    facts = {}
    for which, limit in enumerate(RING_LIMITS):
        facts[limit] = set()
        for s in range(s0, s1 + 1):
            for c in range(256):
                h, f = horizon_reference(cp, hpre, s, c, limit)
                want[s, c, 2 + which] = want[s, c, which]                        # what the step before saw
                want[s, c, which] = h
                facts[limit] |= f
    gaps = horizon_gaps(facts)
    assert not gaps, "\n".join(gaps)
    rc, hz, hz2 = run.horizon(cp, hpre, s0, s1, hz0)
    assert rc == 0
    same(hz, want, "FastHorizon alone")
    same(hz2, want, "FastHorizon inside RetireHorizonWave")


def check_refusals(run):
    case = make_case("refusals", 5000, 4096, 0, 1, 0, "mix", 1)
    assert run.path(case, FUSED)[0] == 0
    for field_shift in (0, 8, 16):
        for bad in (1, 3, 241, 255):
            ev = case["ev"].copy()
            ev[4999] = (ev[4999] & ~np.uint32(0xff << field_shift)) | np.uint32(bad << field_shift)
            assert run.path(case, FUSED, ev=ev)[0] == EINVAL, (field_shift, bad)
    for tile in (0, 4095, 4097, 6144):
        assert run.path(case, FUSED, tile=tile)[0] == EINVAL, tile
    for entry in (KPRE - 1, KPRE + 240, KPRE + 4096):
        assert run.path(case, FUSED, entry=entry)[0] == EINVAL, entry
    assert run.path(case, 3)[0] == EINVAL                                        # no such form
    assert run.path(dict(case, t_lo=1, t_hi=0), FUSED)[0] == EINVAL
    assert run.path(dict(case, t_hi=2), FUSED)[0] == EINVAL                      # a tile behind the block
    # every refusal left the arrays alone
    rc, got = run.path(case, FUSED, tile=4095)
    for k in PATH_ARRAYS:
        assert np.all(got[k] == (P8 if got[k].dtype == np.uint8 else P32 if got[k].dtype == np.uint32 else P64)), k
