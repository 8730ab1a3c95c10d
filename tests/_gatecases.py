"""Proposals and truth for the tests of the validity gate (orz_amd/csrc/orz_verify.h) through item patches
(orz_stream_set_item_patches; tests/emu: emu_encode_fast_patched).  TEST INFRASTRUCTURE ONLY.

From the clean item trace of an input (the fast parse is deterministic; GPU = emulation) a `Parse` rebuilds what the decoder
will know: each item's stream offset (the base of a unit is the sum of the earlier units' lengths -- _oracle.plan_from_trace
assumes whole 16 MiB blocks), its ring (context) and its ordinal in that ring, who refers to whom.  The families below propose
patches of single items.  For the PARSE-level families (TYPE / LEN / SRC) the truth is the oracle's plan-driven encoder
(oracle/orz_oracle.c: orc_encode_plan_mem, real 4094-slot rings and per-node len_min: no method shared with the gate's sorted
ordinals) on the identically patched plan: what it accepts the gate must pass and the stream must decode, what it rejects the
gate must reject, at that item, with the class the oracle's code maps to (CODE_CLASSES).  The ITEM-level families (SYM, CTX,
AL, ENC, ROB, UNL, ORD, LMV) damage what the decoder computes by itself: always a finding, of the family's class.

Rules of the reference these follow: ring membership and distance src/matcher.rs:62-80, len_min src/matcher.rs:65-71 and
src/lz.rs:459-467, reduced-offset codes src/lz.rs:494-514, WORD predictor src/lz.rs:132-133,203,233."""
import ctypes
import re

import numpy as np

P = (1 << 24) - 1   # window offset of a block's first new byte (SBVEC_PREMATCH_LEN)
RING = 4094         # LZ_MF_BUCKET_ITEM_SIZE: ring distances 0 .. 4093 are live
WORD = 388
LEVEL1 = (15, 9, 6)
FIELDS = {"TYPE": 0, "LEN": 1, "SRC": 2, "SYM": 3, "CTX": 4, "AL": 5, "ENC": 6, "ROB": 7, "UNL": 8, "ORD": 9, "LMV": 10}

# the gate's classes (ver_name, orz_verify.h) and the oracle's codes (oracle/orz_oracle.h)
TILING, AFTER_LIT, CONTEXT, SYMBOL = "hole/overlap in the item sequence", "after_literal", "context", "symbol"
NO_START, OTHER_RING, BYTES, OUTSIDE = "source is no item start", "source in another ring", "source bytes differ", "source outside the ring"
OFFSET_CODE, ORDINAL, LEN_MIN, LEN_CODE = "offset code", "ordinal", "length below len_min", "length code"
UNLIKELY, WORD_PRED = "excluded symbol", "WORD prediction"
ALL_CLASSES = (TILING, AFTER_LIT, CONTEXT, SYMBOL, NO_START, OTHER_RING, BYTES, OUTSIDE, OFFSET_CODE, ORDINAL, LEN_MIN, LEN_CODE, UNLIKELY, WORD_PRED)
ESHORT, EPOS, ELEN, EEND, ESRC, EBYTES, ELENMIN, EWORD = 2, 3, 4, 5, 6, 7, 8, 9
# (ESHORT: the plan has items left when the input is used up -- the last item but one grown over the last: the sequence does not tile)
CODE_CLASSES = {ESRC: (NO_START, OTHER_RING, OUTSIDE), EBYTES: (BYTES,), ELENMIN: (LEN_MIN,), EWORD: (WORD_PRED,),
                EPOS: (TILING, SYMBOL), ELEN: (TILING, SYMBOL), EEND: (TILING, SYMBOL), ESHORT: (TILING, SYMBOL)}

TRACE_DT = np.dtype([("block", "<u4"), ("pos", "<u4"), ("symbol", "<u2"), ("rank", "<u2"), ("ctx", "<u2"), ("robits", "<u2"),
                     ("unlikely", "u1"), ("enc_len", "u1"), ("after_literal", "u1"), ("match_len", "u1"), ("src", "<u4")])
_EMU_DT = np.dtype([("block", "<u4"), ("pos", "<u4"), ("src", "<u4"), ("sym", "<u2"), ("ctx", "<u2"), ("rob", "<u2"), ("pad", "<u2"),
                    ("mlen", "u1"), ("al", "u1"), ("unl", "u1"), ("enc", "u1")])
_PLAN_DT = np.dtype({"names": ["pos", "src", "type", "len"], "formats": ["<u8", "<u8", "u1", "u1"], "offsets": [0, 8, 16, 17], "itemsize": 24})

# reduced-offset bases of roid_encode (src/lz.rs:494-514): roid i covers 2^(i/2) distances
ROID_BASES = []
_b, _i = 0, 0
while _b < RING:
    ROID_BASES.append(_b)
    _b += 1 << (_i >> 1)
    _i += 1


def input_a():
    import _data
    return _data.text(2_500_000, seed=5)


def input_b():
    """Periods of two and three 32-bit words (a letter and three zero bytes) from a small alphabet, 30 to 70 bytes each, a few odd
    bytes between them; 300 KB.  Every pattern has stood somewhere before, so a region often begins with short matches from such
    earlier pieces, and its long match then has more than one item start of its ring inside its own span: sources that OVERLAP
    their item, and a choice between them.  (The fast parse leaves such a choice rarely -- a long match normally follows the one
    item start it can come from --: a handful in this input, none at all in plain runs and periods of bytes.)"""
    rng = np.random.default_rng(7)
    letters = b"abcdefgh"
    out = bytearray()
    while len(out) < 300_000:
        per = int(rng.choice([2, 3]))
        pat = b"".join(bytes([letters[int(v)]]) + b"\0" * 3 for v in rng.integers(0, len(letters), per))
        ln = int(rng.integers(30, 70))
        out += (pat * (ln // len(pat) + 1))[:ln]
        out += bytes(b"xyz "[int(v)] for v in rng.integers(0, 4, int(rng.integers(0, 3))))
    return bytes(out[:300_000])


def input_c():
    return input_a()[:300_000]


# ------------------------------------------------------------------------------------------------ the encoders under test
class EmuGate:
    """emu_encode_fast_patched: (stream, trace, "") or (None, None, message); the emulation keeps ONE encoder from call to call"""

    def __init__(self, emu):
        self.lib = emu.lib
        self.lib.emu_encode_fast_patched.restype = ctypes.c_long

    def encode(self, data, patches=(), exact=False, fresh=False, want_trace=False):
        arr = np.array([(b, p, FIELDS.get(f, f), v) for b, p, f, v in patches], dtype="<u4").reshape(-1, 4)
        dst = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t()
        err = ctypes.create_string_buffer(4096)
        items = np.zeros(len(data) + 1 if want_trace else 1, dtype=_EMU_DT)
        rc = self.lib.emu_encode_fast_patched(bytes(data), ctypes.c_size_t(len(data)), *LEVEL1, 1 if exact else 0, 1 if fresh else 0,
                                              ctypes.c_void_p(arr.ctypes.data if len(arr) else None), ctypes.c_size_t(len(arr)),
                                              ctypes.byref(dst), ctypes.byref(n), ctypes.c_void_p(items.ctypes.data),
                                              ctypes.c_size_t(len(items) if want_trace else 0), err, ctypes.c_size_t(4096))
        if rc == -2:
            raise ValueError(err.value.decode())
        if rc < 0:
            return None, None, err.value.decode()
        out = ctypes.string_at(dst, n.value)
        self.lib.emu_free(dst)
        tr = None
        if want_trace:
            e = items[:rc]
            tr = np.zeros(rc, dtype=TRACE_DT)
            for a, b in (("block", "block"), ("pos", "pos"), ("symbol", "sym"), ("ctx", "ctx"), ("robits", "rob"), ("unlikely", "unl"),
                         ("enc_len", "enc"), ("after_literal", "al"), ("match_len", "mlen"), ("src", "src")):
                tr[a] = e[b]
        return out, tr, ""


class GpuGate:
    """the same through the C ABI: one orz_amd.StreamEncoder for a whole sweep (it allocates about 6 GB)"""

    def __init__(self, mode="fast"):
        import orz_amd
        self.orz = orz_amd
        self.mode = mode
        self.enc = orz_amd.StreamEncoder(device=0, level=1, mode=mode)

    def encode(self, data, patches=(), exact=False, fresh=False, want_trace=False):
        assert exact == (self.mode == "exact")
        enc = self.orz.StreamEncoder(device=0, level=1, mode=self.mode) if fresh else self.enc
        try:
            enc.set_item_patches(list(patches))  # (refusals: OrzError, not caught here)
            enc.set_item_trace(want_trace)
            try:
                out = enc.encode(data)
            except self.orz.OrzError as e:
                return None, None, str(e)
            finally:
                tr = enc.item_trace() if want_trace else None
                enc.set_item_trace(False)
            return out, tr, ""
        finally:
            if fresh:
                enc.close()

    def close(self):
        self.enc.close()


# ------------------------------------------------------------------------------------------------ the decoder's view of a parse
class Parse:
    def __init__(self, data, trace):
        self.data = bytes(data)
        tr = self.tr = trace
        n = self.n = len(tr)
        self.is_match = (tr["after_literal"] & 2) != 0
        self.is_word = tr["symbol"] == WORD
        self.is_lit = ~self.is_match & ~self.is_word
        self.length = np.where(self.is_match, tr["match_len"], np.where(self.is_word, 2, 1)).astype(np.int64)
        self.block = tr["block"].astype(np.int64)
        self.units = [int(u) for u in np.unique(self.block)]
        self.base = {}       # unit -> stream offset of its first new byte: the sum of the earlier units' lengths
        self.unit_items = {}  # unit -> (first item, one past the last)
        at = 0
        for u in self.units:
            idx = np.nonzero(self.block == u)[0]
            assert idx[-1] - idx[0] + 1 == len(idx), "the items of a unit lie together"
            self.base[u] = at
            self.unit_items[u] = (int(idx[0]), int(idx[-1]) + 1)
            at += int(self.length[idx].sum())
        assert at == len(self.data), "the items cover the input"
        basev = np.array([self.base[int(b)] for b in self.units], dtype=np.int64)[np.searchsorted(self.units, self.block)]
        self.basev = basev
        self.so = basev + tr["pos"].astype(np.int64) - P   # stream offset of each item
        assert self.so[0] == 0 and (self.so[1:] == self.so[:-1] + self.length[:-1]).all(), "the clean items tile the input"
        self.ss = np.where(self.is_match, basev + tr["src"].astype(np.int64) - P, -1)   # ... of each match's source
        self.item_at = np.full(len(self.data) + 1, -1, dtype=np.int64)
        self.item_at[self.so] = np.arange(n)
        self.ctx8 = (tr["ctx"] & 255).astype(np.int64)
        # ordinals: the k-th item of a context since the stream began (the trace carries the contexts, the count is made here)
        order = np.argsort(self.ctx8, kind="stable")
        sc = self.ctx8[order]
        starts = np.searchsorted(sc, np.arange(257))
        self.ord = np.empty(n, dtype=np.int64)
        self.ord[order] = np.arange(n) - starts[sc]
        self.ring = [order[starts[c]:starts[c + 1]] for c in range(256)]   # items of each context, oldest first
        self.srci = np.where(self.is_match, self.item_at[np.maximum(self.ss, 0)], -1)
        assert (self.srci[self.is_match] >= 0).all(), "every clean source is an item start"
        self.ro = np.where(self.is_match, self.ord - 1 - self.ord[np.maximum(self.srci, 0)], -1)
        assert (self.ro[self.is_match] >= 0).all() and (self.ro[self.is_match] <= RING - 1).all()
        assert (self.ctx8[self.srci[self.is_match]] == self.ctx8[self.is_match]).all()
        # first four bytes of every item as a key (equal bytes start with an equal key)
        pad = np.frombuffer(self.data + b"\0" * 8, dtype=np.uint8)
        s = self.so
        self.key4 = (pad[s].astype(np.int64) | (pad[s + 1].astype(np.int64) << 8) | (pad[s + 2].astype(np.int64) << 16) | (pad[s + 3].astype(np.int64) << 24))
        # who refers to each item (in stream order): the node's len_min at any time follows
        self.refs = {}
        for i in np.nonzero(self.is_match)[0]:
            self.refs.setdefault(int(self.srci[i]), []).append(int(i))
        # items with the same context and key, oldest first / the same key whatever the context
        g = np.lexsort((np.arange(n), self.key4, self.ctx8))
        self._grp, self._grp_at = g, np.empty(n, dtype=np.int64)
        self._grp_at[g] = np.arange(n)
        newgrp = np.ones(n, dtype=bool)
        newgrp[1:] = (self.ctx8[g][1:] != self.ctx8[g][:-1]) | (self.key4[g][1:] != self.key4[g][:-1])
        self._grp_start = np.maximum.accumulate(np.where(newgrp, np.arange(n), 0))
        h = np.lexsort((np.arange(n), self.key4))
        self._any, self._any_at = h, np.empty(n, dtype=np.int64)
        self._any_at[h] = np.arange(n)

    # -- helpers
    def win(self, i, stream_off):
        """window offset, in item i's unit, of a stream offset"""
        return int(stream_off - self.basev[i] + P)

    def where(self, i):
        return int(self.tr["block"][i]), int(self.tr["pos"][i])

    def lcp(self, a, b, cap):
        """common prefix of the input at stream offsets a < b, up to cap (an overlapping source is compared byte by byte, as the
        decoder copies)"""
        d = self.data
        k = 0
        end = len(d)
        while k < cap and b + k < end and d[a + k] == d[b + k]:
            k += 1
        return k

    def equal(self, j, i, L):
        a, b = int(self.so[j]), int(self.so[i])
        return b + L <= len(self.data) and self.data[a:a + L] == self.data[b:b + L] if a + L <= b else self.lcp(a, b, L) == L

    def len_min_at(self, j, i):
        """len_min of node j when item i refers to it (src/matcher.rs:65-71)"""
        v = 0
        for r in self.refs.get(int(j), ()):
            if r >= i:
                break
            v = max(v, min(int(self.length[r]) + 1, 127))
        return v

    def group_before(self, i):
        """earlier items of i's context that start with the same four bytes, oldest first"""
        at = int(self._grp_at[i])
        return self._grp[int(self._grp_start[at]):at]

    def same_ring_before(self, i, limit=400):
        """... nearest first: (item, ring distance)"""
        g = self.group_before(i)
        for j in g[::-1][:limit]:
            yield int(j), int(self.ord[i] - 1 - self.ord[j])

    def same_ring_from_oldest(self, i, limit=400):
        """... that are still in the ring, oldest first"""
        g = self.group_before(i)
        k = int(np.searchsorted(self.ord[g], self.ord[i] - 1 - (RING - 1)))
        for j in g[k:k + limit]:
            yield int(j), int(self.ord[i] - 1 - self.ord[j])

    def same_ring_earlier_unit(self, i, limit=400):
        """... of an earlier unit and still in the ring, nearest first"""
        g = self.group_before(i)
        k = int(np.searchsorted(g, self.unit_items[int(self.block[i])][0]))
        for j in g[:k][::-1][:limit]:
            ro = int(self.ord[i] - 1 - self.ord[j])
            if ro > RING - 1:
                return
            yield int(j), ro

    def at_distance(self, i, ro):
        """the item at ring distance ro of item i, or -1"""
        r = int(self.ord[i]) - 1 - ro
        return int(self.ring[self.ctx8[i]][r]) if r >= 0 else -1

    # -- plans
    def plan(self, patches=()):
        """the parse in stream offsets (orc_plan_item), TYPE / LEN / SRC patches applied"""
        pl = np.zeros(self.n, dtype=_PLAN_DT)
        pl["pos"] = self.so
        pl["type"] = np.where(self.is_match, 2, np.where(self.is_word, 0, 1))
        pl["len"] = np.where(self.is_match, self.tr["match_len"], 0)
        pl["src"] = np.where(self.is_match, self.ss, 0)
        for b, p, f, v in patches:
            i = int(self.item_at[self.base[b] + p - P])
            assert i >= 0 and self.block[i] == b
            if f == "TYPE":
                pl["type"][i] = v
                if v != 2:
                    pl["len"][i] = 0
                    pl["src"][i] = 0
            elif f == "LEN":
                pl["len"][i] = v
            elif f == "SRC":
                pl["src"][i] = self.base[b] + v - P
            else:
                raise AssertionError("the oracle has no say on " + f)
        return pl


def oracle_verdict(oracle, data, plan):
    """(stream, None, None) when the plan-driven encoder accepts the plan, else (None, stream offset, code)"""
    L = oracle.lib()
    L.orc_encode_plan_mem.restype = ctypes.c_int
    dst = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    err = oracle.PlanError()
    plan = np.ascontiguousarray(plan)
    rc = L.orc_encode_plan_mem(bytes(data), ctypes.c_size_t(len(data)), ctypes.c_void_p(plan.ctypes.data), ctypes.c_size_t(len(plan)),
                               ctypes.byref(dst), ctypes.byref(n), None, ctypes.byref(err))
    if rc != 0:
        return None, int(err.pos), int(err.code)
    out = ctypes.string_at(dst, n.value)
    L.orc_free(dst)
    return out, None, None


# ------------------------------------------------------------------------------------------------ families
class Case:
    def __init__(self, family, unit, item, patches, expect=None, level="parse", note=""):
        self.family, self.unit, self.item, self.patches, self.expect, self.level, self.note = family, unit, item, patches, expect, level, note

    def __repr__(self):
        return "%s unit %d item %d %r %s" % (self.family, self.unit, self.item, self.patches, self.note)


def _src_patch(ps, i, j):
    b, p = ps.where(i)
    return [(b, p, "SRC", ps.win(i, ps.so[j]))]


def _legal_alternatives(ps, i):
    L = int(ps.length[i])
    for j, ro in ps.same_ring_before(i):
        if ro > RING - 1:
            return
        if j != ps.srci[i] and ps.equal(j, i, L):
            yield j, ro


def p_src_nearest(ps, i):
    if not ps.is_match[i]:
        return None
    for j, ro in _legal_alternatives(ps, i):
        return _src_patch(ps, i, j), "ring distance %d" % ro
    return None


def p_src_farthest(ps, i):
    if not ps.is_match[i]:
        return None
    L = int(ps.length[i])
    for j, ro in ps.same_ring_from_oldest(i):
        if j != ps.srci[i] and ps.equal(j, i, L):
            return _src_patch(ps, i, j), "ring distance %d" % ro
    return None


def _p_src_at(ro, legal=True):
    def probe(ps, i):
        if not ps.is_match[i]:
            return None
        j = ps.at_distance(i, ro)
        if j < 0 or j == ps.srci[i] or ps.key4[j] != ps.key4[i] or not ps.equal(j, i, int(ps.length[i])):
            return None
        return _src_patch(ps, i, j), "ring distance %d" % ro
    return probe


def p_src_oldest(ps, i):
    """the oldest node still in the ring: distance 4093, or the context's first item while the ring has not yet turned"""
    if not ps.is_match[i]:
        return None
    ro = min(int(ps.ord[i]) - 1, RING - 1)
    return _p_src_at(ro)(ps, i) if ro >= 0 else None


def p_src_earlier_unit(ps, i):
    if not ps.is_match[i]:
        return None
    L = int(ps.length[i])
    for j, ro in ps.same_ring_earlier_unit(i):
        if j != ps.srci[i] and ps.equal(j, i, L):
            return _src_patch(ps, i, j), "ring distance %d, source in unit %d" % (ro, ps.block[j])
    return None


def p_src_overlap(ps, i):
    if not ps.is_match[i]:
        return None
    L = int(ps.length[i])
    for j, ro in _legal_alternatives(ps, i):
        if ps.so[i] - ps.so[j] < L:
            return _src_patch(ps, i, j), "ring distance %d, %d bytes back" % (ro, ps.so[i] - ps.so[j])
    return None


def p_other_ring(ps, i):
    if not ps.is_match[i]:
        return None
    at = int(ps._any_at[i])
    for s in range(at - 1, max(-1, at - 200), -1):
        j = int(ps._any[s])
        if ps.key4[j] != ps.key4[i]:
            break
        if ps.ctx8[j] != ps.ctx8[i] and ps.block[j] == ps.block[i] and ps.equal(j, i, int(ps.length[i])):
            return _src_patch(ps, i, j), "context %d for %d" % (ps.ctx8[j], ps.ctx8[i])
    return None


def p_no_item_start(ps, i):
    if not ps.is_match[i]:
        return None
    b, p = ps.where(i)
    for q in (int(ps.ss[i]) + 1, int(ps.ss[i]) - 1):
        if 0 < q < ps.so[i] and ps.item_at[q] < 0 and ps.win(i, q) >= 1:
            return [(b, p, "SRC", ps.win(i, q))], "one byte off the source"
    return None


def p_bytes_short(ps, i):
    L = int(ps.length[i])
    if not ps.is_match[i] or L < 5:
        return None
    for j, ro in ps.same_ring_before(i):
        if ro > RING - 1:
            break
        if ps.lcp(int(ps.so[j]), int(ps.so[i]), L) == L - 1:
            return _src_patch(ps, i, j), "ring distance %d, equal for %d of %d" % (ro, L - 1, L)
    return None


def p_len_min_above(ps, i):
    L = int(ps.length[i])
    if not ps.is_match[i]:
        return None
    for j, ro in _legal_alternatives(ps, i):
        if ps.len_min_at(j, i) == L + 1:
            return _src_patch(ps, i, j), "ring distance %d, len_min %d" % (ro, L + 1)
    return None


def p_len_plus(ps, i):
    if not ps.is_match[i] or ps.length[i] >= 240:
        return None
    b, p = ps.where(i)
    return [(b, p, "LEN", int(ps.length[i]) + 1)], ""


def p_len_minus(ps, i):
    if not ps.is_match[i]:
        return None
    b, p = ps.where(i)
    return [(b, p, "LEN", int(ps.length[i]) - 1)], ""


def p_len_below_four(ps, i):
    if not ps.is_match[i] or ps.length[i] != 4:
        return None
    b, p = ps.where(i)
    return [(b, p, "LEN", 3)], "a match of three bytes"


def p_match_to_literal(ps, i):
    if not ps.is_match[i]:
        return None
    b, p = ps.where(i)
    return [(b, p, "TYPE", 1)], ""


def p_literals_to_word(ps, i):
    if not (ps.is_lit[i] and i + 1 < ps.n and ps.is_lit[i + 1] and ps.block[i + 1] == ps.block[i]):
        return None
    if ps.tr["unlikely"][i] == ps.data[int(ps.so[i])]:   # (words[hash2][0] is the item's first byte: the table may well predict the pair)
        return None
    b, p = ps.where(i)
    return [(b, p, "TYPE", 0)], ""


def _item(field, value, ok=lambda ps, i: True):
    def probe(ps, i):
        if not ok(ps, i):
            return None
        b, p = ps.where(i)
        return [(b, p, field, int(value(ps, i)))], ""
    return probe


def _lmv_ok(ps, i):
    if not ps.is_match[i]:
        return False
    j = int(ps.srci[i])
    e = max(int(ps.tr["match_len"][j]), 4)
    return ps.len_min_at(j, i) >= 5 and int(ps.length[i]) != e   # (a length equal to the expected one is coded 0 whatever len_min is)


# name -> (probe, level, the class a rejected case must show or None = the oracle alone decides, inputs)
FAMILIES = {
    "src_nearest": (p_src_nearest, "parse", None),
    "src_farthest": (p_src_farthest, "parse", None),
    "src_4093": (_p_src_at(RING - 1), "parse", None),
    "src_oldest": (p_src_oldest, "parse", None),
    "src_earlier_unit": (p_src_earlier_unit, "parse", None),
    "src_overlap": (p_src_overlap, "parse", None),
    "src_4094": (_p_src_at(RING), "parse", OUTSIDE),
    "src_other_ring": (p_other_ring, "parse", OTHER_RING),
    "src_no_item_start": (p_no_item_start, "parse", NO_START),
    "src_bytes_short": (p_bytes_short, "parse", BYTES),
    "src_len_min_above": (p_len_min_above, "parse", LEN_MIN),
    "len_plus": (p_len_plus, "parse", TILING),
    "len_minus": (p_len_minus, "parse", TILING),
    "len_below_four": (p_len_below_four, "parse", SYMBOL),
    "match_to_literal": (p_match_to_literal, "parse", TILING),
    "literals_to_word": (p_literals_to_word, "parse", WORD_PRED),
    "al": (_item("AL", lambda ps, i: (ps.tr["after_literal"][i] & 1) ^ 1), "item", AFTER_LIT),
    "ctx": (_item("CTX", lambda ps, i: ps.tr["ctx"][i] ^ 1), "item", CONTEXT),
    "sym": (_item("SYM", lambda ps, i: ps.tr["symbol"][i] ^ 1, lambda ps, i: bool(ps.is_lit[i])), "item", SYMBOL),
    "sym_match_of_a_literal": (_item("SYM", lambda ps, i: 256 + (ps.tr["symbol"][i] & 127), lambda ps, i: bool(ps.is_lit[i])), "item", SYMBOL),
    # the match flag against the symbol alone: a match coded with the literal symbol of its first byte
    "sym_literal_of_a_match": (_item("SYM", lambda ps, i: ps.data[int(ps.so[i])], lambda ps, i: bool(ps.is_match[i])), "item", SYMBOL),
    # the symbol's offset code alone: the neighbouring code, same length id, offset bits untouched
    "sym_other_offset": (_item("SYM", lambda ps, i: int(ps.tr["symbol"][i]) + (6 if int(ps.tr["symbol"][i]) + 6 < WORD else -6), lambda ps, i: bool(ps.is_match[i])), "item", OFFSET_CODE),
    "rob": (_item("ROB", lambda ps, i: ps.tr["robits"][i] ^ 1, lambda ps, i: bool(ps.is_match[i]) and (ps.tr["robits"][i] >> 12) >= 1), "item", OFFSET_CODE),
    "enc": (_item("ENC", lambda ps, i: ps.tr["enc_len"][i] + 1, lambda ps, i: bool(ps.is_match[i]) and ps.tr["enc_len"][i] + 1 < 240), "item", (LEN_CODE, OFFSET_CODE)),
    "unl": (_item("UNL", lambda ps, i: ps.tr["unlikely"][i] ^ 1), "item", UNLIKELY),
    "ord": (_item("ORD", lambda ps, i: ps.ord[i] + 1), "item", ORDINAL),
    "lmv": (_item("LMV", lambda ps, i: ps.len_min_at(ps.srci[i], i) - 1, _lmv_ok), "item", LEN_CODE),
}
for _k, _base in enumerate(ROID_BASES):   # both sides of every reduced-offset base: the last distance of a code and the first of the next
    if _base >= 1:
        FAMILIES["src_roid_%d_below" % _base] = (_p_src_at(_base - 1), "parse", None)
        FAMILIES["src_roid_%d_at" % _base] = (_p_src_at(_base), "parse", None)
ROID_FAMILIES = sorted((f for f in FAMILIES if f.startswith("src_roid_")), key=lambda f: (int(f.split("_")[2]), f))
LEGAL_SRC_FAMILIES = ["src_nearest", "src_farthest", "src_4093", "src_oldest", "src_earlier_unit"]
ILLEGAL_SRC_FAMILIES = ["src_4094", "src_other_ring", "src_no_item_start", "src_bytes_short", "src_len_min_above"]
SHAPE_FAMILIES = ["len_plus", "len_minus", "len_below_four", "match_to_literal", "literals_to_word"]
ITEM_FAMILIES = ["al", "ctx", "sym", "sym_match_of_a_literal", "sym_literal_of_a_match", "sym_other_offset", "rob", "enc", "unl", "ord", "lmv"]


def targets(ps, unit, family, nrandom=3, seed=11, edges=True, reach=6000):
    """Cases of one family in one unit: the first and the last eligible item of the unit, items 0 and n - 1 and the items number
    63, 64, 255, 256, 4095, 4096 of the unit where the family applies to them, and a few seeded random ones."""
    probe, level, expect = FAMILIES[family]
    lo, hi = ps.unit_items[unit]
    found = {}

    def take(i, note):
        if i is not None and lo <= i < hi and i not in found:
            r = probe(ps, i)
            if r is not None:
                found[i] = Case(family, unit, i, r[0], expect, level, (note + " " + r[1]).strip())
                return True
        return False

    def scan(start, step, note):
        i = start
        for _ in range(reach):
            if not (lo <= i < hi):
                return
            if i in found or take(i, note):
                return
            i += step

    scan(lo, 1, "first eligible")
    scan(hi - 1, -1, "last eligible")
    if edges:
        take(lo, "item 0")
        take(hi - 1, "item n-1")
        for k in (63, 64, 255, 256, 4095, 4096):
            take(lo + k, "item %d" % k)
    rng = np.random.default_rng(seed + 1000 * unit + sum(map(ord, family)))
    for r in range(nrandom):
        scan(int(rng.integers(lo, hi)), 1, "random")
    return [found[i] for i in sorted(found)]


def accepted_src_case(ps, oracle, unit=0, tries=40):
    """the first match of the unit with another equal node in its ring that nothing refers to, moved there -- if the oracle accepts"""
    lo, hi = ps.unit_items[unit]
    for i in range(lo, hi):
        if not ps.is_match[i]:
            continue
        for j, ro in _legal_alternatives(ps, i):
            if j in ps.refs:
                continue
            case = Case("src_unreferenced", unit, i, _src_patch(ps, i, j), None, "parse", "ring distance %d" % ro)
            if oracle_verdict(oracle, ps.data, ps.plan(case.patches))[0] is not None:
                return case
            tries -= 1
            break
        if tries <= 0:
            break
    return None


# ------------------------------------------------------------------------------------------------ judging
_GATE = re.compile(r"validity gate, block (\d+): the items do not decode:(.*) first at window offset (\d+) --")


def parse_gate_message(msg):
    """-> (block, {class: count}, first window offset) of a gate finding, or None"""
    m = _GATE.search(msg)
    if not m:
        return None
    counts = {}
    for part in m.group(2).split(";"):
        part = part.strip()
        if part:
            k, name = part.split(" x ", 1)
            counts[name] = int(k)
    return int(m.group(1)), counts, int(m.group(3))


def judge(ps, oracle, case, out, msg):
    """The one rule of these tests: `out` / `msg` is what the encoder under test made of case.patches.  Returns the gate's classes
    that fired (empty: accepted)."""
    b, p = ps.where(case.item)
    verdict = None
    if case.level == "parse":
        verdict = oracle_verdict(oracle, ps.data, ps.plan(case.patches))
    if verdict is not None and verdict[0] is not None:
        assert case.expect is None, "%r: built to be illegal, but the oracle accepts it" % (case,)
        assert out is not None, "%r: the oracle accepts the patched plan, the gate refuses it: %s" % (case, msg)
        back, used = oracle.decode(out)
        assert back == ps.data and used == len(out), "%r: the gate passed a stream that does not decode" % (case,)
        return ()
    assert out is None, "%r: the damaged items went through the gate (%d bytes)%s" % (
        case, len(out), "" if verdict is None else "; the oracle rejects the plan at %d with code %d" % verdict[1:])
    g = parse_gate_message(msg)
    assert g is not None, "%r: the encode failed, but not at the gate: %s" % (case, msg)
    blk, counts, first = g
    assert blk == b, "%r: finding in block %d: %s" % (case, blk, msg)
    assert first == p, "%r: the first finding is at window offset %d, the patched item at %d: %s" % (case, first, p, msg)
    if case.expect is not None:
        want = case.expect if isinstance(case.expect, tuple) else (case.expect,)
        assert any(counts.get(c, 0) >= 1 for c in want), "%r: no finding of class %r: %s" % (case, want, msg)
    if verdict is not None:
        _, pos, code = verdict
        s = int(ps.so[case.item])
        plen = {"TYPE": 2 if case.patches[0][3] == 0 else 1, "LEN": case.patches[0][3]}.get(case.patches[0][2], int(ps.length[case.item]))
        assert s <= pos <= s + plen, "%r: the oracle rejects at stream offset %d, the patched item is [%d, %d]" % (case, pos, s, s + plen)
        assert code in CODE_CLASSES, "%r: oracle code %d" % (case, code)
        assert any(counts.get(c, 0) >= 1 for c in CODE_CLASSES[code]), "%r: the oracle says code %d, the gate has none of %r: %s" % (
            case, code, CODE_CLASSES[code], msg)
    return tuple(c for c in counts if counts[c])


# ------------------------------------------------------------------------------------------------ many legal patches at once
def legal_set(ps, oracle, per_unit=160, seed=3, overlap=False):
    """SRC patches the oracle accepts ALL AT ONCE: per unit, every match with an equal-bytes node at ring distance exactly 4093,
    matches with a source in an earlier unit, and nearest alternatives (overlapping ones first when asked); a node is used once
    and only if nothing else refers to it (patches interact through len_min); what the oracle still rejects is thinned out.
    -> [(item, source item, ring distance)]"""
    rng = np.random.default_rng(seed)
    chosen, used = [], set()

    def add(i, j, ro, quota, lone=True):
        if i in taken or j in used or (lone and j in ps.refs) or quota[0] <= 0:
            return
        taken.add(i)
        used.add(j)
        chosen.append((i, j, ro))
        quota[0] -= 1

    taken = set()
    for u in ps.units:
        lo, hi = ps.unit_items[u]
        m = np.nonzero(ps.is_match[lo:hi])[0] + lo
        q = [per_unit // 4]
        for i in m[ps.ord[m] >= RING]:     # (a ring that has turned: a node at distance 4093 exists)
            j = ps.at_distance(int(i), RING - 1)
            if ps.key4[j] == ps.key4[i] and j != ps.srci[i] and ps.equal(j, int(i), int(ps.length[i])):
                add(int(i), j, RING - 1, q)
                if q[0] <= 0:
                    break
        pick = rng.permutation(m)
        q = [per_unit // 4]
        if u != ps.units[0]:
            for i in pick[:6000]:
                for j, ro in ps.same_ring_earlier_unit(int(i)):
                    if j != ps.srci[i] and ps.equal(j, int(i), int(ps.length[i])):
                        add(int(i), j, ro, q)
                        break
                if q[0] <= 0:
                    break
        q = [per_unit - sum(1 for i, _, _ in chosen if ps.block[i] == u)]
        for want_overlap in ((True, False) if overlap else (False,)):
            for i in (pick if want_overlap else pick[:8000]):
                for j, ro in _legal_alternatives(ps, int(i)):
                    if not want_overlap or ps.so[i] - ps.so[j] < ps.length[i]:
                        add(int(i), j, ro, q, lone=not want_overlap)   # (an overlapping node is the source of the item before: thinned if need be)
                        break
                if q[0] <= 0:
                    break
    for _ in range(200):   # thin: the oracle names the offset it stops at -- drop the patch of that item, or the patches whose node it refers to
        patches = [p for i, j, _ in chosen for p in _src_patch(ps, i, j)]
        out, pos, code = oracle_verdict(oracle, ps.data, ps.plan(patches))
        if out is not None:
            return chosen, patches, out
        i = int(ps.item_at[pos])
        drop = [c for c in chosen if c[0] == i] or [c for c in chosen if c[1] == ps.srci[i]]
        assert drop, "the oracle rejects the patched plan at %d (code %d) for no patch's sake" % (pos, code)
        chosen = [c for c in chosen if c not in drop]
    raise AssertionError("no legal set after 200 rounds of thinning")


def legal_floors(ps, chosen, overlap=False):
    """what the set must still hold per unit: (patches >= 100, at distance 4093 >= 5, source in an earlier unit >= 5 -- the first
    unit has none before it), and, where overlapping sources were asked for, >= 5 of them in all"""
    for u in ps.units:
        mine = [c for c in chosen if ps.block[c[0]] == u]
        n4093 = sum(1 for c in mine if c[2] == RING - 1)
        nearlier = sum(1 for c in mine if ps.block[c[1]] < u)
        assert len(mine) >= 100, "unit %d: %d legal patches" % (u, len(mine))
        if not overlap:
            assert n4093 >= 5, "unit %d: %d patches at ring distance 4093" % (u, n4093)
        if u != ps.units[0]:
            assert nearlier >= 5, "unit %d: %d patches with a source in an earlier unit" % (u, nearlier)
    if overlap:
        nover = sum(1 for i, j, _ in chosen if ps.so[i] - ps.so[j] < ps.length[i])
        assert nover >= 5, "%d patches with an overlapping source" % nover
