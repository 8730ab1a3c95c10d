"""A serial replay of the fast parse's repair passes (orz_amd/csrc/orz_fast.h: RepairListWave, FastSource, FastRecut,
FastFlipSparse, FastWordCheckL, FastWordApplyL, FastCokGrow, FastPassEnd and their grid forms), and the cases it is run on.

A pass is a deterministic function of the state it starts from, and the replay restates it in plain numpy / Python without the
kernels' shortcuts: no lists, no `rdirty` / `edge` / `cok` / `kdirty` skips, no summary walks -- every match is given its source
in full in every pass, and every WORD item on the path is judged against words[] as a decoder would hold it on reaching it.  It
shares no code with the kernels and reads no table captured from the library: the candidate runs (position order, history
included) come from _fasttables.reference, the history item starts and words[] at the block start from the item trace of the
units before the block.  Its input is the decision field the probe recorded BEFORE the first pass (or the field a test injects).

Positions are block offsets i here (window offset = KPRE + i).  ty: 0 WORD, 1 literal, 2 match.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

import _fasttables as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KPRE = ft.KPRE
WORD, LIT, MATCH = 0, 1, 2
MINLEN, MAXLEN = 4, 240
KRING = 4094                # LZ_MF_BUCKET_ITEM_SIZE
EDGE = 1024                 # FastSource::kEdgeMargin
SUB = 4096
FAR = 16384                 # slots of the run beyond the tabulated ones that the source search looks at
CTL_FIELDS = ("chg", "done", "total", "passes", "nmem", "acc", "lt", "lastflips", "nent", "ncut", "nfix", "nwx", "hot", "hotacc")


def src_cap(depth):
    """item starts examined beyond the tabulated predecessors (the encoder's default: it follows the level's depth)"""
    return 4 * depth + 4


DEPTH = {0: 5, 1: 15, 2: 45}    # match-finder depth of the levels (include/orz_hip.h: orz_lzcfg_from_level)


class Block:
    """what a pass needs besides the state: bytes, candidate runs, history, words[] at the block start"""

    def __init__(self, data, k, trace):
        hpos, wsnap = ft.history_from_trace(data, k, trace)
        R = ft.reference(data, k, hpos, wsnap)
        self.n = n = R["n"]
        self.R = R
        self.win = ft.Window(data, k).win
        self.nhist = R["nhist"]
        self.epos = R["epos"].astype(np.int64)
        self.idx = R["idx"].astype(np.int64)               # slot of new position i
        self.depth = R["depth"].astype(np.int64)           # slots of its run below it
        self.rows = R["rows"]
        self.T = R["text"]
        self.hist_slot = np.nonzero(self.epos < KPRE)[0]
        x = np.arange(KPRE - 4, KPRE + n + 2, dtype=np.int64)
        self._h1 = ft.hash1(self.win, x)                   # hash1(x) for x >= KPRE - 4
        self._h2 = ft.hash2(self.win, x)
        self.ctx_slot = ft.hash1(self.win, self.epos - 1).astype(np.int64)   # context of the position in every slot
        wp = wsnap[0::2].astype(np.int64) | (wsnap[1::2].astype(np.int64) << 8)
        self.words0 = wp

    def h1(self, x):
        return self._h1[x - (KPRE - 4)]

    def h2(self, x):
        return self._h2[x - (KPRE - 4)]

    def byte(self, x):
        return int(self.win[x + ft.PAD])


def path_of(ty, nl, n):
    """item-start flags and previous-item types of the path a field describes, walked from the block's first position; an undecided
    position on the path is the literal it is read as (returned in copies of ty / nl)"""
    ty = np.array(ty[:n], dtype=np.uint8)
    nl = np.array(nl[:n], dtype=np.uint8)
    s = np.zeros(n + 1, dtype=np.uint8)
    pt = np.zeros(n + 1, dtype=np.uint8)
    x = 0
    while x < n:
        if nl[x] == 0:
            ty[x] = LIT
            nl[x] = 1
        s[x] = 1
        t = ty[x]
        x += int(nl[x])
        pt[x] = t
    assert x == n
    return ty, nl, s, pt


class State:
    def __init__(self, ty, nl, pt, s):
        self.ty = np.array(ty, dtype=np.uint8)
        self.nl = np.array(nl, dtype=np.uint8)
        self.pt = np.array(pt, dtype=np.uint8)
        self.s = np.array(s, dtype=np.uint8)

    def copy(self):
        return State(self.ty, self.nl, self.pt, self.s)


def replay_pass(B, st, src, grown, K=ft.K, far=FAR, cap=64, ring=KRING):
    """one repair pass on a copy of state `st` (ty / nl / pt: n + 1 entries, s: item-start flags) -> (new state, src, report).
    src: window offset of every match's source as the passes before left it (updated in the copy returned); grown: item starts
    gained per context since the first pass began (updated in the copy returned)."""
    n = B.n
    st = st.copy()
    src = src.copy()
    grown = grown.copy()
    ty, nl, pt, s = st.ty, st.nl, st.pt, st.s
    rep = {"ring_stops": 0, "cap_stops": 0, "far_found": 0, "cut_spans": [], "edge": {}, "clamped": 0, "recut_words": 0}
    starts = np.nonzero(s[:n])[0]
    rep["nmem"] = len(starts)
    rep["cok"] = (grown <= EDGE).astype(np.uint32)
    # ---- ordinals: item starts of the context before the position, history included (only differences are used)
    live = np.zeros(len(B.epos), dtype=bool)
    live[B.hist_slot] = True
    live[B.idx[starts]] = True
    ls = np.nonzero(live)[0]
    by_pos = ls[np.argsort(B.epos[ls], kind="stable")]
    c = B.ctx_slot[by_pos]
    o = np.argsort(c, kind="stable")
    cs = c[o]
    first = np.concatenate([[0], np.nonzero(np.diff(cs))[0] + 1])
    rank = np.arange(len(cs)) - np.repeat(first, np.diff(np.concatenate([first, [len(cs)]])))
    ordinal = np.zeros(len(B.epos), dtype=np.int64)
    ordinal[by_pos[o]] = rank
    # ---- lists as the pass found them (reported: the capacities)
    m_at = starts[ty[starts] == MATCH]
    w_at = starts[ty[starts] == WORD]
    rep["mcnt"] = np.bincount(m_at // SUB, minlength=(n + SUB - 1) // SUB)
    rep["wcnt"] = np.bincount(w_at // SUB, minlength=(n + SUB - 1) // SUB)
    rep["m_at"], rep["w_at"] = m_at, w_at
    # ---- sources
    cuts = []
    edge = np.zeros(n, dtype=np.uint8)
    for i in m_at.tolist():
        L = int(nl[i])
        j = int(B.idx[i])
        d = int(B.depth[i])
        op = int(ordinal[j])
        r = min(K, d)
        best = bsrc = 0
        found = -1
        stop = False
        row = B.rows[i]
        for k in range(r):
            q = j - 1 - k
            if not live[q]:
                continue
            l = int(row[k])
            if l >= MINLEN and (l >= L or l > best):
                if op - 1 - int(ordinal[q]) > ring - 1:
                    stop = True
                    rep["ring_stops"] += 1
                    break
                if l >= L:
                    found = q
                    break
                best, bsrc = l, q
        if found < 0 and not stop and d > K and far:
            rs = j - d
            top = j - K
            lo2 = top - far if top - rs > far else rs
            cand = np.nonzero(live[lo2:top])[0][::-1] + lo2
            left = cap
            for q in cand.tolist():
                l = int(B.T.lcp([KPRE + i], [B.epos[q]])[0])
                if l >= MINLEN and (l >= L or l > best):
                    if op - 1 - int(ordinal[q]) > ring - 1:
                        stop = True
                        rep["ring_stops"] += 1
                        break
                    if l >= L:
                        found = q
                        rep["far_found"] += 1
                        break
                    best, bsrc = l, q
                left -= 1
                if left == 0:
                    rep["cap_stops"] += 1
                    break
        if found >= 0:
            src[i] = B.epos[found]
            edge[i] = op - 1 - int(ordinal[found]) > ring - 1 - EDGE
            rep["edge"][i] = int(edge[i])
            continue
        cuts.append((i, i + L))
        if best >= MINLEN:
            nl[i] = best
            src[i] = B.epos[bsrc]
            edge[i] = op - 1 - int(ordinal[bsrc]) > ring - 1 - EDGE
            rep["edge"][i] = int(edge[i])
        else:
            ty[i] = LIT
            nl[i] = 1
    # ---- recut: the rest of a cut item's old span, from the field's decisions
    for i, end in cuts:
        x = i + int(nl[i])
        pt[x] = ty[i]
        rep["cut_spans"].append((i, x, end))
        while x < end:
            t, L = int(ty[x]), int(nl[x])
            if L == 0:
                t, L = LIT, 1
            if x + L > end:
                if t == MATCH and end - x >= MINLEN:
                    L = end - x
                    rep["clamped"] += 1
                else:
                    t, L = LIT, 1
            ty[x] = t
            nl[x] = L
            s[x] = 1
            grown[B.h1(KPRE + x - 1)] += 1
            if t == WORD:
                rep["recut_words"] += 1
            x += L
            pt[x] = t
    # ---- WORD check: every WORD item of the path as it stands now, against words[] as a decoder holds it on reaching the item
    words = B.words0.copy()
    fixes = []
    for y in np.nonzero(s[:n])[0].tolist():
        if y >= 1 and pt[y] != WORD:
            words[B.h2(KPRE + y - 3)] = B.byte(KPRE + y - 2) | (B.byte(KPRE + y - 1) << 8)
        if ty[y] == WORD and words[B.h2(KPRE + y - 1)] != (B.byte(KPRE + y) | (B.byte(KPRE + y + 1) << 8)):
            fixes.append(y)
    for y in fixes:
        ty[y] = LIT
        nl[y] = 1
        ty[y + 1] = LIT
        nl[y + 1] = 1
        s[y + 1] = 1
        pt[y + 1] = LIT
        pt[y + 2] = LIT
        grown[B.h1(KPRE + y)] += 1
    rep.update(ncut=len(cuts), nfix=len(fixes), chg=len(cuts) + len(fixes), edge_arr=edge, grown=grown.copy(), fixes=fixes)
    return st, src, rep


def replay(B, ty, nl, pt=None, s=None, K=ft.K, far=FAR, cap=64, ring=KRING, max_passes=64):
    """all passes from a decision field: [(state, src, report)] per pass, the last of which repaired nothing.  pt / s: as recorded
    before the first pass (None: derived from the field by walking the path, as an injected field's are)."""
    n = B.n
    if s is None:
        ty, nl, s, pt = path_of(ty, nl, n)
    st = State(np.concatenate([ty[:n], [0]]), np.concatenate([nl[:n], [0]]), pt[:n + 1], s[:n + 1])
    st.ty[n] = ty[n] if len(ty) > n else 0
    st.nl[n] = nl[n] if len(nl) > n else 0
    src = np.zeros(n, dtype=np.int64)
    grown = np.zeros(256, dtype=np.int64)
    out = []
    for _ in range(max_passes):
        st, src, rep = replay_pass(B, st, src, grown, K=K, far=far, cap=cap, ring=ring)
        grown = rep["grown"]
        out.append((st, src, rep))
        if rep["chg"] == 0:
            return out
    raise AssertionError("the replay's passes do not come to an end")


def final_arrays(B, st):
    """S / TY (low two bits and the after-a-literal bit) / ML / W0 of the committed parse, from the final state"""
    n = B.n
    S = st.s[:n].copy()
    at = np.nonzero(S)[0]
    TY = np.zeros(n, dtype=np.uint8)
    TY[at] = st.ty[at] | ((st.pt[at] == LIT).astype(np.uint8) << 2)
    ML = np.zeros(n, dtype=np.uint8)
    m = at[st.ty[at] == MATCH]
    ML[m] = st.nl[m]
    words = B.words0.copy()
    W0 = np.zeros(n, dtype=np.uint8)
    for y in at.tolist():
        if y >= 1 and st.pt[y] != WORD:
            words[B.h2(KPRE + y - 3)] = B.byte(KPRE + y - 2) | (B.byte(KPRE + y - 1) << 8)
        W0[y] = words[B.h2(KPRE + y - 1)] & 0xff
    return S, TY, ML, W0


def compare(probe, B, passes, lt0=None):
    """lines that say where a probe (probe_tables) differs from the replay `passes`; empty = equal.
    lt0: type of the item that ended at the block's start (None: the stream's first block, whose first item is not held to it)"""
    bad = []
    n = B.n

    def eq(name, got, want):
        got = np.asarray(got).astype(np.int64)
        want = np.asarray(want).astype(np.int64)
        if got.shape != want.shape:
            bad.append("%s: %r entries, want %r" % (name, got.shape, want.shape))
            return
        ne = np.nonzero(got != want)[0]
        if len(ne):
            bad.append("%s: %d of %d entries differ, first at %d: got %r want %r" % (name, len(ne), got.size, ne[0], got[ne[0]], want[ne[0]]))

    if len(probe["passes"]) != len(passes):
        bad.append("passes: %d, want %d (repairs per pass: %r, want %r)" % (len(probe["passes"]), len(passes), [p["ctl"]["chg"] for p in probe["passes"]],
                                                                            [r["chg"] for _, _, r in passes]))
    total = 0
    prev_src = prev_nl = None
    high = {}
    for k, (got, (st, src, rep)) in enumerate(zip(probe["passes"], passes)):
        tag = "pass %d " % k
        eq(tag + "sbits", got["sbits"][:n], st.s[:n])
        eq(tag + "ty", got["ty"][:n], st.ty[:n])
        eq(tag + "nl", got["nl"][:n], st.nl[:n])
        eq(tag + "pt", got["pt"], st.pt)
        m = np.nonzero((st.s[:n] == 1) & (st.ty[:n] == MATCH))[0]
        # (a match an item was recut into in this pass gets its source in the next one)
        have = m[src[m] != 0]
        eq(tag + "src", got["src"][have], src[have])
        # the edge flag of every source the replay ASSIGNED: all in the first pass, later where the answer is a new one (the
        # kernels' later passes keep the flag of a source they do not look at again, by design)
        if k == 0:
            fresh = have
        else:
            fresh = have[(prev_src[have] != src[have]) | (prev_nl[have] != st.nl[have])]
        eq(tag + "edge", got["edge"][fresh], rep["edge_arr"][fresh])
        prev_src, prev_nl = src, st.nl.copy()
        c = got["ctl"]
        lists = probe["lists"]      # (the grid form keeps no lists and none of their counters)
        for name, want in (("chg", rep["chg"]), ("ncut", rep["ncut"]), ("nfix", rep["nfix"]), ("nwx", rep["recut_words"]), ("acc", rep["nmem"]),
                           ("total", total), ("passes", k), ("done", 0)):
            if c[name] != want and (lists or name not in ("ncut", "nfix", "nwx")):
                bad.append("%sctl.%s: %d, want %d" % (tag, name, c[name], want))
        total += rep["chg"]
        if lists:
            eq(tag + "cgrow", got["cok"][:256], rep["grown"])
            eq(tag + "cok", got["cok"][256:], rep["cok"])
            if k == 0:      # (later passes list only what they look at again)
                eq(tag + "mcnt", got["mcnt"], rep["mcnt"])
            eq(tag + "wcnt", got["wcnt"], rep["wcnt"])
            # the lists' rows: the entries in position order, and NOTHING written behind them -- the rows were filled with 0xa5
            # before the first pass; behind the most entries a pass has listed so far they, and the row behind the last subtile's,
            # still hold it (a write past a full row lands in the next)
            nsub = len(rep["mcnt"])
            for name, width, at, held in (("mlist", SUB // MINLEN, rep["m_at"], k == 0), ("wlist", SUB // 2, rep["w_at"], True)):
                rows = got[name].reshape(nsub + 1, width).astype(np.int64)
                cnt = np.bincount(at // SUB, minlength=nsub)
                top = high.setdefault(name, np.zeros(nsub + 1, dtype=np.int64))
                if held:
                    want = np.full((nsub + 1, width), -1, dtype=np.int64)
                    for sub in range(nsub):
                        want[sub, :cnt[sub]] = at[at // SUB == sub] % SUB
                    ne = np.nonzero((want >= 0) & (rows != want))
                    if len(ne[0]):
                        bad.append("%s%s: row %d entry %d is %d, want %d" % (tag, name, ne[0][0], ne[1][0], rows[ne[0][0], ne[1][0]], want[ne[0][0], ne[1][0]]))
                    top[:nsub] = np.maximum(top[:nsub], cnt)
                else:           # (later passes list only the matches they look at again: at most those of the first)
                    if (got["mcnt"] > cnt).any():
                        bad.append("%smcnt: more matches listed than the pass found" % tag)
                    top[:nsub] = np.maximum(top[:nsub], got["mcnt"])
                behind = np.arange(width)[None, :] >= top[:, None]
                ne = np.nonzero(behind & (rows != 0xa5a5))
                if len(ne[0]):
                    bad.append("%s%s: row %d entry %d was written (%d) behind the row's %d entries" % (tag, name, ne[0][0], ne[1][0], rows[ne[0][0], ne[1][0]], top[ne[0][0]]))
        if len(bad) > 12:
            return bad
    if bad:
        return bad
    st, src, rep = passes[-1]
    S, TY, ML, W0 = final_arrays(B, st)
    f = probe["final"]
    eq("final S", f["S"], S)
    gTY = f["TY"].copy()
    gTY[S == 0] = 0
    if lt0 is None:
        gTY[0] &= 3
    TY[0] = (TY[0] & 3) | ((lt0 == LIT) << 2 if lt0 is not None else 0)
    eq("final TY", gTY, TY)
    eq("final ML", f["ML"], ML)
    gW0 = f["W0"].copy()
    gW0[S == 0] = 0
    eq("final W0", gW0, W0)
    if probe["lists"] and f["items"] != rep["nmem"]:
        bad.append("final items: %d, want %d" % (f["items"], rep["nmem"]))
    for name, want in (("total", total), ("passes", len(passes)), ("nmem", rep["nmem"]), ("done", 1)):
        if f["ctl"][name] != want:
            bad.append("final ctl.%s: %d, want %d" % (name, f["ctl"][name], want))
    return bad


# ------------------------------------------------------------------------------------------------------------- the emulation twin
class EmuItem(ctypes.Structure):
    _fields_ = [("block", ctypes.c_uint32), ("pos", ctypes.c_uint32), ("src", ctypes.c_uint32), ("sym", ctypes.c_uint16),
                ("rank", ctypes.c_uint16), ("ctx", ctypes.c_uint16), ("mlen", ctypes.c_uint8), ("al", ctypes.c_uint8),
                ("unl", ctypes.c_uint8), ("enc", ctypes.c_uint8)]


ITEM_DT = np.dtype([("block", "<u4"), ("pos", "<u4"), ("src", "<u4"), ("sym", "<u2"), ("rank", "<u2"), ("ctx", "<u2"), ("mlen", "u1"),
                    ("al", "u1"), ("unl", "u1"), ("enc", "u1")], align=True)


@functools.lru_cache(maxsize=None)
def emu_lib():
    so = os.path.join(ROOT, "build", "libemu_repair.so")
    src = os.path.join(ROOT, "tests", "emu", "emu_repair.cpp")
    srcs = [src] + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu_backend.cpp", "simt.h")]
    srcs += [os.path.join(ROOT, "orz_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "orz_amd", "csrc"))]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so + ".tmp", src])
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.emu_repair_table.restype = ctypes.c_long
    return lib


class FieldRefused(ValueError):
    pass


def emu_encode(data, k=None, level=1, tile=0, rounds=0, ty=None, nl=None, lib=None):
    """(stream, probe or None, trace) of one encode on the emulation; k: the encode_block call to probe (None: unarmed)"""
    lib = lib or emu_lib()
    data = bytes(data)
    cfg = {0: (5, 3, 2), 1: (15, 9, 6), 2: (45, 27, 18)}[level]
    dst = ctypes.POINTER(ctypes.c_uint8)()
    dlen = ctypes.c_size_t()
    err = ctypes.create_string_buffer(512)
    cap = len(data) + 16
    items = (EmuItem * cap)()
    nitems = ctypes.c_size_t()
    if ty is not None:
        ty = np.ascontiguousarray(ty, dtype=np.uint8)
        nl = np.ascontiguousarray(nl, dtype=np.uint8)
    rc = lib.emu_repair_encode(data, ctypes.c_size_t(len(data)), cfg[0], cfg[1], cfg[2], int(tile), int(rounds), -1 if k is None else int(k),
                               ctypes.c_void_p(ty.ctypes.data) if ty is not None else None, ctypes.c_void_p(nl.ctypes.data) if nl is not None else None,
                               ctypes.c_size_t(len(ty) if ty is not None else 0), ctypes.byref(dst), ctypes.byref(dlen), items,
                               ctypes.c_size_t(cap), ctypes.byref(nitems), err, ctypes.c_size_t(512))
    if rc == -22:
        raise FieldRefused(err.value.decode())
    assert rc == 0, err.value.decode()
    out = ctypes.string_at(dst, dlen.value)
    lib.emu_free(dst)
    arr = np.frombuffer(items, dtype=ITEM_DT)[:nitems.value]
    trace = {"block": arr["block"].copy(), "pos": arr["pos"].copy(), "word": arr["sym"] == 388, "mlen": np.where(arr["al"] & 2, arr["mlen"], 0)}

    def get(name, dtype):
        size = lib.emu_repair_table(name.encode(), None, ctypes.c_size_t(0))
        if size < 0:
            raise KeyError(name)
        buf = np.empty(size, dtype=np.uint8)
        lib.emu_repair_table(name.encode(), ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(size))
        return buf.view(dtype)

    probe = probe_tables(get) if k is not None else None
    return out, probe, trace


def probe_tables(get):
    """the tables of a repair probe, read through get(name, dtype), as {"n", "K", "depth", "block", "lists", "before": state,
    "passes": [state, ...], "final": {...}}; a state holds ty, nl, pt (n + 1 entries), sbits (a flag per position), and per pass
    src, edge, cok, ctl -- in the lists form also mcnt, wcnt and the rows mlist, wlist"""
    sc = get("scalars", "<u8")
    n = int(sc[0])
    out = {"n": n, "K": int(sc[1]), "depth": int(sc[2]), "block": int(sc[3]), "lists": bool(sc[5])}

    def state(tag):
        st = {k: get("%s.%s" % (tag, k), "u1") for k in ("ty", "nl", "pt")}
        st["sbits"] = np.unpackbits(get(tag + ".sbits", "u1"), bitorder="little")[:n + 1]
        return st

    def ctl(name):
        return {k: int(v) for k, v in zip(CTL_FIELDS, get(name, "<u4"))}

    out["before"] = state("before")
    out["passes"] = []
    for k in range(int(get("passes", "<u4")[0])):
        st = state("p%d" % k)
        for name, dt in (("src", "<u4"), ("edge", "u1"), ("cok", "<u4")) + ((("mcnt", "<u4"), ("wcnt", "<u4"), ("mlist", "<u2"), ("wlist", "<u2")) if out["lists"] else ()):
            st[name] = get("p%d.%s" % (k, name), dt)
        st["ctl"] = ctl("p%d.ctl" % k)
        out["passes"].append(st)
    out["final"] = {k: get("final." + k, "u1") for k in ("S", "TY", "ML", "W0")}
    out["final"]["ctl"] = ctl("final.ctl")
    if out["lists"]:
        out["final"]["items"] = int(get("final.items", "<u4")[0])
    return out


def last_type_before(trace, k):
    """type of the last item of the units before unit k (it ends at the unit's start)"""
    sel = np.nonzero(np.asarray(trace["block"]) < k)[0]
    if not len(sel):
        return None
    i = sel[-1]
    return WORD if trace["word"][i] else MATCH if trace["mlen"][i] else LIT


def gpu_trace(it):
    return {"block": it["block"], "pos": it["pos"], "word": it["symbol"] == 388, "mlen": np.where(it["after_literal"] & 2, it["match_len"], 0)}


# ------------------------------------------------------------------------------------------------------------------ natural cases
NATURAL_SIZES = (4095, 4096, 4097, 3 * 4096 + 17, 65537)
COARSE = dict(tile=1 << 20, rounds=1)      # one round and coarse tiles: hundreds of repairs


@functools.lru_cache(maxsize=None)
def natural_inputs():
    """name -> bytes: text and the "mixed" shape at the sizes around one, three and sixteen subtiles"""
    import _data
    import corpus

    d = {}
    text = corpus.enwik_like(65537)
    mixed = _data.mixed(65537)
    for n in NATURAL_SIZES:
        d["text_%d" % n] = text[:n]
        d["mixed_%d" % n] = mixed[:n]
    d["noise_65537"] = _data.zeros_noise(65537)      # (one round: two thousand WORD items to fix in the first pass)
    return d


# ----------------------------------------------------------------------------------------------------------------- injected cases
# A case is an input of one block (k = 0), a decision field for it and the edges the REPLAY has to reach on it (`reached`: asserted on
# the replay alone, before any kernel runs).  Every field starts from all literals, so every position that is not inside an item
# planted here starts an item: the ordinal distance of two positions of a context is then the count of that context's positions
# between them.
class Case:
    def __init__(self, data, ty, nl):
        self.data = bytes(data)
        self.ty = np.asarray(ty, dtype=np.uint8)
        self.nl = np.asarray(nl, dtype=np.uint8)

    @functools.lru_cache(maxsize=None)
    def block(self):
        none = {"block": np.zeros(0, np.int64), "pos": np.zeros(0, np.int64), "word": np.zeros(0, bool), "mlen": np.zeros(0, np.int64)}
        return Block(self.data, 0, none)

    @functools.lru_cache(maxsize=None)
    def passes(self, level=1):
        return replay(self.block(), self.ty, self.nl, cap=src_cap(DEPTH[level]))


def _literals(n):
    return np.full(n, LIT, dtype=np.uint8), np.ones(n, dtype=np.uint8)


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _plant(d, q, p, length):
    """the bytes [q - 2, q + length) again at p - 2: position p then has q's context, 4-gram and `length` bytes; the byte behind differs"""
    d[p - 2:p + length] = d[q - 2:q + length]
    if p + length < len(d):
        d[p + length] = d[q + length] ^ 0x55


def case_words_cap():
    """every even position of the second subtile a WORD item with a wrong prediction: 2048 list entries, 2048 fixes"""
    n = 3 * SUB + 17
    d = _rand(n, 101)
    ty, nl = _literals(n)
    ty[SUB:2 * SUB:2] = WORD
    nl[SUB:2 * SUB:2] = 2
    c = Case(d, ty, nl)

    def reached(passes):
        r = passes[0][2]
        assert r["wcnt"][1] == SUB // 2 and r["nfix"] == SUB // 2, "the WORD list's capacity was not reached"
        assert r["wcnt"][0] == 0 and r["wcnt"][2] == 0 and r["mcnt"].sum() == 0
    c.reached = reached
    return c


def case_matches_cap():
    """every fourth position of the second subtile a match of four bytes (a copy of the first subtile, a third of them spoiled):
    1024 list entries, the subtiles around it without a match or WORD item"""
    n = 3 * SUB + 17
    d = _rand(n, 102)
    d[SUB:2 * SUB] = d[:SUB]
    d[SUB + 2:2 * SUB:12] ^= 0x3c              # every third match has two bytes in common with its only candidate
    ty, nl = _literals(n)
    ty[SUB:2 * SUB:4] = MATCH
    nl[SUB:2 * SUB:4] = 4
    c = Case(d, ty, nl)

    def reached(passes):
        r = passes[0][2]
        assert r["mcnt"][1] == SUB // 4 and r["mcnt"][0] == 0 and r["mcnt"][2] == 0 and r["wcnt"].sum() == 0, "the match list's capacity was not reached"
        assert 300 < r["ncut"] < 400 and r["nfix"] == 0
    c.reached = reached
    return c


def case_round3():
    """the round-3 shape: a WORD item to be fixed in a wavefront's last lane; the field's decision at the next position is a WORD
    item with a wrong prediction (it is no item: the position lies inside the first), the one after it a match -- which survives"""
    n = SUB + 1
    d = _rand(n, 103)
    at = [64 * 5 + 63, 64 * 31 + 63, SUB - 1 - 64]
    ty, nl = _literals(n)
    for k, i in enumerate(at):
        _plant(d, 100 + 40 * k, i + 2, 9)
        ty[i] = WORD; nl[i] = 2
        ty[i + 1] = WORD; nl[i + 1] = 2
        ty[i + 2] = MATCH; nl[i + 2] = 9
    c = Case(d, ty, nl)

    def reached(passes):
        assert passes[0][2]["fixes"] == at, "the WORD items in the last lanes were not fixed"
        st = passes[-1][0]
        for i in at:
            assert i % 64 == 63 and st.ty[i + 1] == LIT and st.s[i + 2] and st.ty[i + 2] == MATCH and st.nl[i + 2] == 9, "the match did not survive"
    c.reached = reached
    return c


def case_cuts():
    """matches of 240 bytes whose best source offers 4 .. 239; the decisions inside their spans make the recut produce WORD items
    and matches clamped at the old end; one span crosses a subtile boundary, one ends at the block's last byte"""
    n = 3 * SUB + 17
    d = _rand(n, 104)
    ty, nl = _literals(n)
    offers = (4, 5, 17, 239, 236, 237, 238, 100)
    starts = [SUB + 300 * k + 11 for k in range(len(offers))]
    starts[2] = 2 * SUB - 100                      # the rest of its span crosses into the third subtile
    starts[7] = n - 240                            # ... and this one's ends with the block
    for k, (p, l) in enumerate(zip(starts, offers)):
        _plant(d, 64 + 300 * k, p, l)
        ty[p] = MATCH; nl[p] = 240
        x = p + l                                  # inside the span, behind the prefix the source offers:
        ty[x] = WORD; nl[x] = 2                    # a WORD item,
        if p + 240 - (x + 2) >= 1:
            ty[x + 2] = MATCH; nl[x + 2] = min(240, n - (x + 2))   # a match that reaches beyond the old end (clamped, or a literal below 4),
        if k % 2:                                  # and a WORD item that would cross the old end (a literal)
            ty[p + 239] = WORD; nl[p + 239] = 2 if p + 241 <= n else 0
    if nl[n - 1] == 0:
        ty[n - 1] = LIT
    c = Case(d, ty, nl)

    def reached(passes):
        r = passes[0][2]
        spans = {i: (x, end) for i, x, end in r["cut_spans"]}
        assert sorted(spans) == sorted(starts), "not every planted match was cut"
        assert [spans[p][0] - p for p in starts] == list(offers), "the sources do not offer 4 .. 239"
        assert any(x // SUB != (end - 1) // SUB for x, end in spans.values()), "no cut span crosses a subtile boundary"
        assert any(end == n for _, end in spans.values()), "no cut span ends at the block's last byte"
        assert r["clamped"] >= 3 and r["recut_words"] >= 6, "the recut made no clamped matches / WORD items"
        assert len(passes) >= 3, "the clamped matches were not looked at again"
    c.reached = reached
    return c


def _two_contexts(n, seed):
    """'!' or '#' at every even position (the first / second half), a byte of 0x80 .. 0xff at every odd one: the odd positions of a
    half all have ONE context (0x21 / 0x23, not behind a letter or digit), their 4-grams hold two random bytes (sparse runs)"""
    d = np.random.default_rng(seed).integers(128, 256, n, dtype=np.uint8)
    d[(d == 0xa1) | (d == 0xa3)] = 0xa5          # (no even position has one of the two contexts)
    half = (n // 2) & ~1
    d[0:half:2] = 0x21
    d[half::2] = 0x23
    return d, half


def _odd_at_distance(s, q, dist):
    """the odd position p > q with exactly `dist` item starts at odd positions strictly between q and p"""
    odd = np.nonzero(s[q + 2::2])[0] * 2 + q + 2       # item starts at odd positions behind q
    p = int(odd[dist])
    assert p % 2 == 1 and int(s[q + 2:p:2].sum()) == dist
    return p


def case_ring():
    """one context with thousands of item starts (see _two_contexts).  First half: 1500 WORD items between sources and their matches
    are fixed in the first pass, each adding an item start of the context -- it gains more than 1024 (`cok` turns 0), a source that
    was far from the ring's end (no `edge`) is pushed out of the ring.  Second half: the context gains exactly 1024 (`cok` stays 1);
    sources 3069 / 3070 item starts back (the two sides of `edge`) end up 4093 / 4094 back (the two sides of the ring).  First half
    again: matches whose only covering source is 4093 / 4094 item starts back in the first pass already (found / ring stop)."""
    n = 65537
    d, half = _two_contexts(n, 105)
    ty, nl = _literals(n)
    ty0, nl0 = _literals(n)
    # WORD items at even positions: [2000, 5000) in the first half; in the second as many as give exactly 1024 fixes
    ty[2000:5000:2] = WORD; nl[2000:5000:2] = 2
    w2 = half + 2000
    ty[w2:w2 + 2 * 1100:2] = WORD; nl[w2:w2 + 2 * 1100:2] = 2
    # (the second half keeps exactly 1024 WORD items, every one of them wrong: nothing is left there for a later pass to fix)
    for _ in range(20):
        probe = Case(d, ty, nl)
        fixes = set(y for y in replay_pass(probe.block(), *_start(probe), cap=64)[2]["fixes"] if y >= half)
        have = [y for y in range(w2, w2 + 2 * 1100, 2) if ty[y] == WORD]
        drop = [y for y in have if y not in fixes] or have[1024:]
        if not drop:
            break
        ty[drop] = LIT; nl[drop] = 1
    assert len(have) == 1024 and not drop
    _, _, s, _ = path_of(ty, nl, n)
    plan, srcs = {}, {}
    # (no planted match in a run that gains an item start in the first pass -- a run marked dirty is searched again whatever `edge`
    # and `cok` say: the sources are taken from positions whose (context, 4-gram) key no WORD item's second position has)
    sd = np.concatenate([np.zeros(ft.PAD, dtype=np.uint8), d, np.zeros(16, dtype=np.uint8)])
    gains = set(ft.bucket_key(sd, np.nonzero(ty == WORD)[0] + 1).tolist())

    def match(name, q, dist, length=12):
        while int(ft.bucket_key(sd, np.array([q]))[0]) in gains:
            q += 2
        p = _odd_at_distance(s, q, dist)
        _plant(d, q, p, length)
        ty[p] = MATCH; nl[p] = length
        s[p + 1:p + length] = 0                    # (the matches are planted in the order of their positions: each counts those before it)
        plan[name] = p
        srcs[name] = q
    match("grown_out", 1001, 2799)                 # + ~1485 fixes: beyond the ring in the second pass, `edge` never set
    match("found_4093", 1101, KRING - 1)           # (behind the WORD items: the distance counts the path's item starts of the first pass)
    match("stop_4094", 1201, KRING)
    match("edge0_3069", half + 1001, KRING - 1 - EDGE)      # + 1024 = 4093: still a ring member
    match("edge1_3070", half + 1101, KRING - EDGE)          # + 1024 = 4094: not any more
    c = Case(d, ty, nl)
    c.plan = plan

    def reached(passes):
        st0, src0, r0 = passes[0]
        st1, src1, r1 = passes[1]
        B = c.block()
        c1, c2 = 0x21, 0x23
        assert r0["grown"][c1] > EDGE and r1["cok"][c1] == 0, "`cok` did not turn 0 in the first context"
        assert r0["grown"][c2] == EDGE and r1["cok"][c2] == 1, "the second context did not gain exactly the edge margin"
        assert r0["ring_stops"] >= 1 and r1["ring_stops"] >= 2, "the ring did not stop a search in both passes"
        p = plan["found_4093"]                     # (a ring member in the first pass; the context's growth pushes it out in the second)
        assert st0.ty[p] == MATCH and st0.nl[p] == 12 and st1.nl[p] < 12, "found_4093"
        p = plan["edge0_3069"]
        assert passes[-1][0].ty[p] == MATCH and passes[-1][0].nl[p] == 12 and src1[p] == KPRE + srcs["edge0_3069"], "edge0_3069"
        _, _, s0, _ = path_of(c.ty, c.nl, n)
        for k, (st, _, _) in enumerate(passes[:-1]):     # no planted match lies in a run that gained an item start
            new = np.nonzero((st.s[:n] == 1) & (s0[:n] == 0))[0]
            dirty = set(ft.bucket_key(B.win, new + KPRE).tolist())
            for name, p in plan.items():
                if st.ty[p] == MATCH and st.nl[p] == 12:
                    assert int(ft.bucket_key(B.win, np.array([p + KPRE]))[0]) not in dirty, name + ": its run gained an item start"
        assert r0["edge"][plan["found_4093"]] == 1 and r0["edge"][plan["grown_out"]] == 0
        assert r0["edge"][plan["edge0_3069"]] == 0 and r0["edge"][plan["edge1_3070"]] == 1
        assert st0.nl[plan["stop_4094"]] < 12, "stop_4094 was not cut in the first pass"
        for name in ("grown_out", "edge1_3070"):
            p = plan[name]
            assert st0.nl[p] == 12 and st0.ty[p] == MATCH and st1.nl[p] < 12, name + " was not cut in the second pass"
    c.reached = reached
    return c


def _start(case):
    ty, nl, s, pt = path_of(case.ty, case.nl, case.block().n)
    n = case.block().n
    st = State(np.concatenate([ty, [0]]), np.concatenate([nl, [0]]), pt, s)
    return st, np.zeros(n, dtype=np.int64), np.zeros(256, dtype=np.int64)


def case_both_lists():
    """the second subtile holds 512 matches AND 1024 WORD items (a match of four bytes and two WORD items in every eight positions):
    both halves of the packed lane prefix are large at once, 8 + 16 entries a lane"""
    n = 3 * SUB + 17
    d = _rand(n, 106)
    d[SUB:2 * SUB] = d[:SUB]
    d[SUB + 1:2 * SUB:24] ^= 0x3c              # every third match has one byte in common with its only candidate
    ty, nl = _literals(n)
    ty[SUB:2 * SUB:8] = MATCH; nl[SUB:2 * SUB:8] = 4
    for off in (4, 6):
        ty[SUB + off:2 * SUB:8] = WORD; nl[SUB + off:2 * SUB:8] = 2
    c = Case(d, ty, nl)

    def reached(passes):
        r = passes[0][2]
        assert r["mcnt"][1] == SUB // 8 and r["wcnt"][1] == SUB // 4, "the lists do not hold 512 matches and 1024 WORD items"
        assert r["mcnt"][0] == r["mcnt"][2] == r["wcnt"][0] == r["wcnt"][2] == 0
        assert r["ncut"] > 100 and r["nfix"] > 100
    c.reached = reached
    return c


def case_cuts_grow():
    """one context (see _two_contexts) gains more than 1024 item starts through CUTS alone: ten matches of 240 bytes whose source
    offers four, the rest of every span re-parsed into literals (118 of them in the context).  `cok` turns 0; a match behind them
    whose source lay 3000 item starts back (no `edge`) finds it beyond the ring in the second pass."""
    n = 65537
    d, half = _two_contexts(n, 107)
    ty, nl = _literals(n)
    big = [3001 + 400 * k for k in range(10)]
    for k, p in enumerate(big):
        _plant(d, 101 + 20 * k, p, 4)
        ty[p] = MATCH; nl[p] = 240
    _, _, s, _ = path_of(ty, nl, n)
    sd = np.concatenate([np.zeros(ft.PAD, dtype=np.uint8), d, np.zeros(16, dtype=np.uint8)])
    inside = np.concatenate([np.arange(p + 4, p + 240) for p in big])
    gains = set(ft.bucket_key(sd, inside).tolist())
    q = 1001
    while int(ft.bucket_key(sd, np.array([q]))[0]) in gains:
        q += 2
    p = _odd_at_distance(s, q, 3000)
    assert p > big[-1] + 240
    _plant(d, q, p, 12)
    ty[p] = MATCH; nl[p] = 12
    c = Case(d, ty, nl)

    def reached(passes):
        st0, _, r0 = passes[0]
        st1, _, r1 = passes[1]
        assert r0["ncut"] == 10 and r0["nfix"] == 0 and [x - i for i, x, _ in r0["cut_spans"]] == [4] * 10, "not ten cuts down to four bytes"
        assert r0["grown"][0x21] > EDGE and r1["cok"][0x21] == 0, "`cok` did not turn 0 through cuts"
        assert r0["edge"][p] == 0 and st0.nl[p] == 12 and st1.nl[p] < 12 and r1["ring_stops"] >= 1, "the match behind the cuts was not pushed out of the ring"
    c.reached = reached
    return c


@functools.lru_cache(maxsize=None)
def injected():
    return {"words_cap": case_words_cap(), "matches_cap": case_matches_cap(), "both_lists": case_both_lists(), "round3": case_round3(),
            "cuts": case_cuts(), "cuts_grow": case_cuts_grow(), "ring": case_ring()}


# -------------------------------------------------------------------------------------------------------------- form equivalence
# The knobs of the repair stage (ORZ_FAST_REPAIR, ORZ_FAST_FULLPASS, ORZ_FAST_SRCCAP) are read once per process: every form runs in a
# child process of its own, which writes the stream and the probe of the natural many-repair case to a file.
FORM_INPUTS = (("mixed_65537", 2), ("noise_65537", 1))     # (input, rounds): the most cuts over four passes / thousands of WORD fixes
FORMS = {"default": {}, "grid": {"ORZ_FAST_REPAIR": "grid"}, "fullpass": {"ORZ_FAST_FULLPASS": "1"}, "nocap": {"ORZ_FAST_SRCCAP": "0"}}


def flatten(out, probe):
    flat = {"stream": np.frombuffer(out, dtype=np.uint8), "n": probe["n"], "K": probe["K"], "depth": probe["depth"], "npass": len(probe["passes"]),
            "lists": int(probe["lists"])}
    for k, v in probe["before"].items():
        flat["before." + k] = v
    for i, p in enumerate(probe["passes"]):
        for k, v in p.items():
            flat["p%d.%s" % (i, k)] = np.array([v[f] for f in CTL_FIELDS]) if k == "ctl" else v
    for k, v in probe["final"].items():
        flat["final." + k] = np.array([v[f] for f in CTL_FIELDS]) if k == "ctl" else v
    return flat


def unflatten(z):
    def ctl(a):
        return {f: int(x) for f, x in zip(CTL_FIELDS, a)}

    probe = {"n": int(z["n"]), "K": int(z["K"]), "depth": int(z["depth"]), "lists": bool(z["lists"]), "before": {}, "passes": [{} for _ in range(int(z["npass"]))], "final": {}}
    for key in z.files:
        head, _, k = key.partition(".")
        if not k:
            continue
        v = ctl(z[key]) if k == "ctl" else int(z[key]) if k == "items" else z[key]
        if head == "before":
            probe["before"][k] = v
        elif head == "final":
            probe["final"][k] = v
        else:
            probe["passes"][int(head[1:])][k] = v
    return z["stream"].tobytes(), probe


NO_TRACE = {"block": np.zeros(0, np.int64), "pos": np.zeros(0, np.int64), "word": np.zeros(0, bool), "mlen": np.zeros(0, np.int64)}


def forms_agree(forms):
    """default, grid and fullpass of run_form: one stream, one state after every pass, one set of committed arrays, per input"""
    for name, _ in FORM_INPUTS:
        out0, p0 = forms["default"][name]
        assert p0["lists"] and len(p0["passes"]) >= 3 and sum(p["ctl"]["chg"] for p in p0["passes"]) >= 100, name
        for f in ("grid", "fullpass"):
            out, p = forms[f][name]
            assert p["lists"] == (f != "grid")
            assert out == out0, (name, f)
            assert len(p["passes"]) == len(p0["passes"]), (name, f)
            for k, (a, b) in enumerate(zip(p["passes"], p0["passes"])):
                for key in ("ty", "nl", "pt", "sbits"):
                    assert np.array_equal(a[key], b[key]), (name, f, k, key)
                m = np.nonzero((b["sbits"][:p0["n"]] == 1) & (b["ty"][:p0["n"]] == MATCH))[0]
                assert np.array_equal(a["src"][m], b["src"][m]), (name, f, k, "src")
                for key in ("chg", "total", "passes", "acc"):
                    assert a["ctl"][key] == b["ctl"][key], (name, f, k, key)
            for key in ("S", "TY", "ML", "W0"):
                assert np.array_equal(p["final"][key], p0["final"][key]), (name, f, key)
            for key in ("total", "passes", "nmem", "done"):
                assert p["final"]["ctl"][key] == p0["final"]["ctl"][key], (name, f, key)


def run_form(backend, form, timeout=600):
    """{input: (stream, probe)} of FORM_INPUTS under the form's knobs, from a child process (backend: "emu" or "gpu")"""
    import sys
    import tempfile

    env = dict(os.environ)
    for k in ("ORZ_FAST_REPAIR", "ORZ_FAST_FULLPASS", "ORZ_FAST_SRCCAP", "ORZ_FAST_UNIT"):
        env.pop(k, None)
    env.update(FORMS[form])
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([sys.executable, os.path.abspath(__file__), backend, tmp], env=env, check=True, timeout=timeout)
        out = {}
        for name, _ in FORM_INPUTS:
            with np.load(os.path.join(tmp, name + ".npz")) as z:
                out[name] = unflatten(z)
        return out


def _child(backend, tmp):
    if backend == "gpu":
        import faulthandler

        import orz_amd

        faulthandler.dump_traceback_later(300, exit=True)   # (a hung device call ends the child)
    for name, rounds in FORM_INPUTS:
        data = natural_inputs()[name]
        if backend == "emu":
            out, probe, _ = emu_encode(data, 0, level=1, tile=COARSE["tile"], rounds=rounds)
        else:
            enc = orz_amd.StreamEncoder(device=0, level=1)
            try:
                enc.set_mode("fast", COARSE["tile"], rounds)
                enc.arm_repair_probe(0)
                out = enc.encode(data)
                probe = probe_tables(enc.repair_probe)
            finally:
                enc.close()
        np.savez(os.path.join(tmp, name + ".npz"), **flatten(out, probe))


if __name__ == "__main__":
    import sys

    _child(sys.argv[1], sys.argv[2])
