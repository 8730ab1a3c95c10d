"""Brute-force references of the fast parse's static per-block tables, and the inputs they are checked on.

Every table the rounds of a block read (the comments of FastArgs in orz_amd/csrc/orz_fast.h) has a plain
definition in terms of the window's bytes and the set of history item starts.  This module restates those definitions in numpy
and shares no code with the kernels: it gets the input bytes, the number of the captured unit and the item trace of the units
before it, and builds everything else itself.  tests/test_fast_tables.py (emulation) and tests/test_gpu_fast_tables.py (the
product library) compare a captured block with it entry for entry.

Two conventions had to be read out of the encoder (orz_stream.h) because a reference can silently copy a kernel's mistake there:

(a) WHAT LIES BEHIND THE BLOCK'S END.  Prefixes (up to 240 bytes), the slot records (12 bytes), the 4-gram of the last three
    positions and the two bytes of the last word-list slot all read past the end of the new bytes.  encode_stream uploads the
    whole block's bytes (all its units) at window offset kPre before the first unit is encoded, and slide_by moves
    kPre + (bytes of the later units) + 2 bytes down by the unit's size.  So behind a unit's end lie THE NEXT UNITS' BYTES -- not the
    zero sentinel -- and behind the end of the data lies whatever the window held there before: for the last unit of an input
    the stale copy of the input's tail that the slides left in place, then the zeros of a fresh encoder.  `Window` below replays
    exactly these copies on a zero buffer; nothing else about the encoder is assumed.
(b) THE KEYS OF THE LAST THREE HISTORY POSITIONS (window offsets kPre-3 .. kPre-1).  BuildKeys takes them from `tailkey`, which
    TailKeys fills from the window BEFORE the slide (positions end-3 .. end-1 of the unit just encoded): the reference files an
    item under the 4-gram it saw when it inserted it.  Between the units of one block the bytes behind the unit's end are the same
    before and after the slide (see (a)), so the two readings agree there; they differ only across a 16 MiB block boundary, where
    the 4-gram ran into the sentinel.  The reference here computes those three keys from the window as it was before the slide in
    every case.  The input `far` of the GPU tier (17 MiB: its captured unit is the first of the second block) is where the two
    readings differ.

Units: ORZ_FAST_UNIT = 1 MiB (the minimum); a rest shorter than an eighth of a unit joins the unit before it
(encode_block_units).  The inputs of the CPU tier are shorter than one 16 MiB block.
"""
import functools

import numpy as np

KPRE = (1 << 25) // 2 - 1          # SBVEC_PREMATCH_LEN: window offset of a block's first new byte
UNIT = 1 << 20
KHASH = 4627
NKEYS = 256 * KHASH
MAXLEN = 240
K = 32                             # run predecessors tabulated per position (kFastK)
KSUB = 4096
KHISTSUB = (KPRE + 1) // KSUB
PAD = 64                           # bytes kept in front of window offset 0 (the encoder keeps 480 zeros there, two of them matter)
DIST_SAMPLES = (0, 1, 3, 7, 15, 31, 47, 63)   # the predecessors whose distance is coded (0 = the newest)


# ---------------------------------------------------------------------------------------------------------------- the window
BLOCK = 1 << 24                    # new bytes of a full block


def unit_sizes(total, unit=UNIT):
    """sizes of the encode_block calls of an input, in order (every 16 MiB block is cut into units by itself)"""
    out = []
    for b0 in range(0, total, BLOCK):
        take, done = min(BLOCK, total - b0), 0
        while done < take:
            n = min(unit, take - done)
            if take - done - n < unit // 8:
                n = take - done
            out.append(n)
            done += n
    return out


class Window:
    """the window of encode_block call k of `data` as the encoder holds it; win[x + PAD] is the byte at window offset x"""

    def __init__(self, data, k):
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        total = len(data)
        assert total > 0
        sizes = unit_sizes(total)
        buf = np.zeros(PAD + KPRE + min(total, BLOCK) + 1024, dtype=np.uint8)
        take = min(BLOCK, total)
        buf[PAD + KPRE:PAD + KPRE + take] = data[:take]   # a whole block is uploaded before its first unit
        done = 0           # bytes of the stream encoded so far
        in_block = 0       # ... of the current block
        self.tailkeys = None
        for j in range(k):
            sh = sizes[j]
            extra = take - in_block - sh                   # bytes of the block's later units: they move along
            # keys of the unit's last three positions, from the window before it slides (convention (b))
            end = KPRE + sh
            self.tailkeys = bucket_key(buf, np.arange(end - 3, end))
            span = KPRE + extra + 2
            buf[PAD - 2:PAD - 2 + span] = buf[PAD - 2 + sh:PAD - 2 + sh + span].copy()
            done += sh
            in_block += sh
            if extra == 0:                                 # the block is done: the next one is uploaded over what lies there
                take = min(BLOCK, total - done)
                buf[PAD + KPRE:PAD + KPRE + take] = data[done:done + take]
                in_block = 0
        self.win = buf
        self.off = done            # stream offset of the unit's first byte
        self.n = sizes[k]
        self.sizes = sizes
        self.k = k


# ------------------------------------------------------------------------------------------------- the format's hash functions
def is_alnum(b):
    b = b.astype(np.int32)
    return ((b >= 48) & (b <= 57)) | ((b >= 65) & (b <= 90)) | ((b >= 97) & (b <= 122))


def hash1(win, x):
    """ctx of an item starting at x + 1: low seven bits of the byte at x, and whether the byte before it is a letter or digit"""
    x = np.asarray(x, dtype=np.int64)
    return (win[x + PAD] & 0x7f).astype(np.uint32) | (is_alnum(win[x - 1 + PAD]).astype(np.uint32) << 7)


def hash2(win, x):
    x = np.asarray(x, dtype=np.int64)
    return (win[x + PAD] & 0x7f).astype(np.uint32) | (hash1(win, x - 1) << 7)


def hash_dword(win, x):
    x = np.asarray(x, dtype=np.int64)
    b = [win[x + i + PAD].astype(np.uint64) for i in range(4)]
    m = np.uint64(0xffffffff)
    h = (((b[0] * np.uint64(131313131)) & m) ^ np.uint64(797)) + (((b[1] * np.uint64(1313131)) & m) ^ np.uint64(79797)) \
        + (((b[2] * np.uint64(13131)) & m) ^ np.uint64(7979797)) + (((b[3] * np.uint64(131)) & m) ^ np.uint64(797979797))
    return (h & m).astype(np.uint64)


def bucket_key(win, x):
    x = np.asarray(x, dtype=np.int64)
    return (hash1(win, x - 1).astype(np.uint64) * np.uint64(KHASH) + hash_dword(win, x) % np.uint64(KHASH)).astype(np.uint32)


# --------------------------------------------------------------------------------------------------------- distance codes
def _code_values():
    """the distance each code stands for: exact below 16, then eight steps per octave"""
    v = list(range(16))
    c = 16
    while v[-1] < (1 << 26):
        v.append((8 + (c - 16) % 8) << ((c - 16) // 8 + 1))
        c += 1
    return np.array(v, dtype=np.int64)


CODE_VALUES = _code_values()


def dist_code_up(d):
    """the smallest code whose distance is not below d"""
    return np.searchsorted(CODE_VALUES, np.asarray(d, dtype=np.int64), side="left").astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------ common prefixes
class Text:
    """bytes of the window region a block uses, readable eight at a time"""

    def __init__(self, win, lo, hi):
        self.lo = lo
        seg = win[lo + PAD:hi + PAD + 8].astype(np.uint64)
        m = len(seg) - 8
        w = np.zeros(m, dtype=np.uint64)
        for i in range(8):
            w |= seg[i:i + m] << np.uint64(8 * i)
        self.w8 = w

    def lcp(self, p, q, cap=MAXLEN):
        """common prefix of the texts at p[i] and q[i], capped"""
        p = np.asarray(p, dtype=np.int64) - self.lo
        q = np.asarray(q, dtype=np.int64) - self.lo
        res = np.full(len(p), cap, dtype=np.int64)
        act = np.arange(len(p))
        for off in range(0, cap, 8):
            if not len(act):
                break
            x = self.w8[p[act] + off] ^ self.w8[q[act] + off]
            ne = x != 0
            xd = x[ne]
            low = xd & (~xd + np.uint64(1))          # lowest set bit: the first byte that differs holds it
            first = (np.log2(low.astype(np.float64)).astype(np.int64)) >> 3
            res[act[ne]] = np.minimum(cap, off + first)
            act = act[~ne]
        return res


# ------------------------------------------------------------------------------------------------------ history from the trace
def history_from_trace(data, k, items):
    """(hpos, wsnap) of unit k from the items of the units before it.
    items: arrays `block`, `pos` (window offset when the item was encoded), `word` (item is a WORD), `mlen` (0 unless a match)."""
    data = bytes(data)
    sizes = unit_sizes(len(data))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blk = np.asarray(items["block"], dtype=np.int64)
    sel = blk < k
    blk = blk[sel]
    spos = offs[blk] + np.asarray(items["pos"], dtype=np.int64)[sel] - KPRE      # stream offsets of the item starts
    assert (np.diff(spos) > 0).all()
    hpos = KPRE - offs[k] + spos
    hpos = hpos[hpos >= 1]                                                        # window offset 0 is dead
    # words[]: a non-WORD item ending at y writes words[hash2(y - 3)] = the two bytes before y
    word = np.asarray(items["word"], dtype=bool)[sel]
    mlen = np.asarray(items["mlen"], dtype=np.int64)[sel]
    length = np.where(word, 2, np.where(mlen > 0, mlen, 1))
    y = (spos + length)[~word]
    sdata = np.concatenate([np.zeros(PAD, dtype=np.uint8), np.frombuffer(data, dtype=np.uint8)])   # zeros in front of the stream
    key = hash2(sdata, y - 3)            # (hash2 indexes with + PAD: stream offsets work like window offsets here)
    wsnap = np.zeros(65536, dtype=np.uint8)
    if len(y):
        rk = key[::-1]
        uniq, first = np.unique(rk, return_index=True)      # the last write of each key wins
        yy = y[::-1][first]
        wsnap[2 * uniq] = sdata[yy - 2 + PAD]
        wsnap[2 * uniq + 1] = sdata[yy - 1 + PAD]
    return hpos.astype(np.uint32), wsnap


# ------------------------------------------------------------------------------------------------------------- the references
def reference(data, k, hpos, wsnap):
    """every static table of unit k of `data`, from the definitions; hpos / wsnap as history_from_trace derives them"""
    W = Window(data, k)
    win, n = W.win, W.n
    hpos = np.asarray(hpos, dtype=np.int64)
    nhist = len(hpos)
    nent = nhist + n
    R = {"n": n, "nhist": nhist, "nent": nent, "nk": n + 1, "K": K, "stream_off": W.off}
    # ---- candidate lists: history item starts (ascending), then the new positions, stable by (ctx, 4-gram hash)
    pos = np.concatenate([hpos, np.arange(KPRE, KPRE + n, dtype=np.int64)])
    keys = bucket_key(win, pos)
    tail = (pos < KPRE) & (pos + 3 >= KPRE)
    if tail.any():
        keys[tail] = W.tailkeys[pos[tail] + 3 - KPRE]
    order = np.argsort(keys, kind="stable")
    epos = pos[order]
    skeys = keys[order]
    R["epos"] = epos.astype(np.uint32)
    R["keys"] = skeys
    slot_of = np.empty(nent, dtype=np.int64)
    slot_of[order] = np.arange(nent)
    idx = slot_of[nhist:]
    R["idx"] = idx.astype(np.uint32)
    present, first = np.unique(skeys, return_index=True)
    R["present_keys"] = present
    R["runstart_present"] = first.astype(np.uint32)
    rs_slot = np.repeat(first, np.diff(np.concatenate([first, [nent]])))          # first slot of the run, per slot
    depth = (np.arange(nent) - rs_slot)                                            # slots of the run below the slot
    newslot = epos >= KPRE
    depth_new = depth[idx]                                                         # per new position
    R["depth"] = depth_new
    R["rlen"] = np.minimum(255, depth_new).astype(np.uint8)
    nvw = nent // 64 + 2
    bits = np.zeros(nvw * 64, dtype=np.uint8)
    bits[:nent] = ~newslot
    R["vbits"] = np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8")
    # ---- slot records: 12 text bytes and the position
    T = Text(win, int(epos.min()) - 8, KPRE + n + 320)
    lo8 = T.w8[epos - T.lo]
    hi4 = T.w8[epos + 8 - T.lo] & np.uint64(0xffffffff)
    stext = np.empty(2 * nent, dtype=np.uint64)
    stext[0::2] = lo8
    stext[1::2] = hi4 | (epos.astype(np.uint64) << np.uint64(32))
    R["stext"] = stext
    R["hist_slots"] = np.nonzero(~newslot)[0]                                      # the compact lists' heads sit in these slots
    ccnt = np.zeros(NKEYS, dtype=np.uint32)
    np.add.at(ccnt, skeys[~newslot], 1)
    R["ccnt"] = ccnt
    # ---- rows: common prefix with the (k+1)-th predecessor in the run; 0 from the run's depth on
    p = np.arange(KPRE, KPRE + n, dtype=np.int64)
    rows = np.zeros((n, K), dtype=np.uint8)
    hist_pred = np.zeros((n, K), dtype=bool)
    for c in range(K):
        have = np.nonzero(depth_new > c)[0]
        if not len(have):
            break
        q = epos[idx[have] - 1 - c]
        rows[have, c] = T.lcp(p[have], q)
        hist_pred[have, c] = q < KPRE
    R["rows"] = rows
    R["hist_pred"] = hist_pred
    # ---- eight distance codes: the predecessors number 1, 2, 4, 8, 16, 32, 48, 64 -- of the r = min(K, depth) tabulated ones, a
    # sample beyond them stands for the oldest of them (FastRowsWave's comment; every reader clamps by the same r:
    # FastEval::count_from's kend, `span`, `nabove`) -- 255 when the run is empty
    r = np.minimum(K, depth_new)
    codes = np.zeros(n, dtype=np.uint64)
    dist = np.zeros((n, 8), dtype=np.int64)
    for m, smp in enumerate(DIST_SAMPLES):
        kk = np.minimum(smp, np.maximum(r, 1) - 1)
        q = epos[np.maximum(idx - 1 - kk, 0)]
        d = np.where(r > 0, p - q, 0)
        dist[:, m] = d
        code = np.where(r > 0, dist_code_up(d), np.uint64(255)).astype(np.uint64)
        codes |= code << np.uint64(8 * m)
    R["rdist"] = codes
    R["dist"] = dist
    # ---- word predictor lists: positions kPre-1 .. kPre+n-1 by hash2 of the position before, stable
    u = np.arange(KPRE - 1, KPRE + n, dtype=np.int64)
    kk2 = hash2(win, u - 1)
    korder = np.argsort(kk2, kind="stable")
    kpos = u[korder]
    kkeys = kk2[korder]
    R["kpos"] = kpos.astype(np.uint32)
    R["kkeys"] = kkeys
    kpresent, kfirst = np.unique(kkeys, return_index=True)
    krun = np.zeros(32768, dtype=np.uint32)
    krun[kpresent] = kfirst
    R["krun"] = krun
    kw = win[kpos + PAD].astype(np.uint16) | (win[kpos + 1 + PAD].astype(np.uint16) << 8)
    R["kw"] = kw
    nk = n + 1
    s = np.arange(nk)
    below = s - krun[kkeys].astype(np.int64)
    rk = np.minimum(64, below)
    wm = np.zeros(nk, dtype=np.uint64)
    for t in range(64):
        ok = rk > t
        src = np.maximum(s - 1 - t, 0)
        wm |= (ok & (kw[src] == kw)).astype(np.uint64) << np.uint64(63 - t)
    excl = (rk > 0) & (kpos[np.maximum(s - 1, 0)] == kpos - 1)
    wpair = wsnap[0::2].astype(np.uint16) | (wsnap[1::2].astype(np.uint16) << 8)
    snap = wpair[kkeys] == kw
    meta = rk.astype(np.uint16) | (excl.astype(np.uint16) << 7) | (snap.astype(np.uint16) << 8)
    newk = kpos >= KPRE
    wmask = np.zeros(n, dtype=np.uint64)
    kmeta = np.zeros(n, dtype=np.uint16)
    wmask[kpos[newk] - KPRE] = wm[newk]
    kmeta[kpos[newk] - KPRE] = meta[newk]
    R["wmask"] = wmask
    R["kmeta"] = kmeta
    # ---- history item starts per (subtile (x + 1) >> 12, ctx) and the exclusive prefix down the columns
    hcm = np.zeros((KHISTSUB, 256), dtype=np.uint32)
    if nhist:
        np.add.at(hcm, ((hpos + 1) >> 12, hash1(win, hpos - 1)), 1)
    hpre = np.zeros((KHISTSUB + 1, 256), dtype=np.uint32)
    np.cumsum(hcm, axis=0, out=hpre[1:])
    R["hcm"] = hcm.reshape(-1)
    R["hpre"] = hpre.reshape(-1)
    R["text"] = T
    R["end"] = KPRE + n
    return R


def compare(cap, ref):
    """names of the tables of the captured block that differ from the reference, with the first differing entry of each"""
    bad = []

    def eq(name, got, want):
        got = np.asarray(got)
        want = np.asarray(want)
        if got.shape != want.shape:
            bad.append("%s: %r entries, want %r" % (name, got.shape, want.shape))
            return
        ne = np.nonzero(got != want)[0]
        if len(ne):
            bad.append("%s: %d of %d entries differ, first at %d: got %r want %r" % (name, len(ne), got.size, ne[0], got[ne[0]], want[ne[0]]))

    for s in ("n", "nhist", "nent", "nk", "K", "stream_off"):
        if cap[s] != ref[s]:
            bad.append("%s: %r, want %r" % (s, cap[s], ref[s]))
    if bad:
        return bad
    for name in ("epos", "keys", "idx", "rlen", "vbits", "stext", "ccnt", "rdist", "kpos", "kkeys", "krun", "kw", "wmask", "kmeta", "hcm", "hpre"):
        eq(name, cap[name], ref[name])
    eq("rows", cap["rows"], ref["rows"].reshape(-1))
    # runstart is written for the keys that occur (ScatterSlots, orz_stream.h:139); the others keep what an earlier block left.
    # No reader asks for them -- every one takes the key of a slot or position of this block: FastSlotInitWave (orz_fast.h:277,
    # keys[j]), FastEval::scan_far (orz_fast.h:697, the key of p), FastRetire (orz_fast.h:969), FastListReset (orz_fast.h:1009,
    # keys[j]) and the source walk (orz_fast.h:1977, bucket_key of p)
    eq("runstart", cap["runstart"][ref["present_keys"]], ref["runstart_present"])
    # the compact lists' heads: the history slots hold their own record; the slots behind them are filled by FastRetire later
    h = ref["hist_slots"]
    cl = cap["cl"].reshape(-1, 2)
    eq("cl", cl[h].reshape(-1), ref["stext"].reshape(-1, 2)[h].reshape(-1))
    return bad


# ------------------------------------------------------------------------------------------------------------------ the inputs
PREFIXES = (3, 4, 11, 12, 13, 19, 20, 21, 27, 28, 29, 51, 52, 53, 239, 240, 241, 300)


def _collide3(rng):
    """two 4-grams that agree on three bytes and on the hash: a common prefix of exactly 3 inside one run"""
    z = np.zeros(PAD + 8, dtype=np.uint8)
    while True:
        z[PAD:PAD + 3] = rng.integers(0, 256, 3)
        hs = []
        for c in range(256):
            z[PAD + 3] = c
            hs.append(int(hash_dword(z, [0])[0] % KHASH))
        seen = {}
        for c, h in enumerate(hs):
            if h in seen:
                return bytes(z[PAD:PAD + 3]), seen[h], c
            seen[h] = c


def planted(total=2 * UNIT + 400 * 1024, seed=77):
    """pairs and chains of positions that share context and 4-gram with a chosen common prefix, at every alignment of both
    positions, in a background of random bytes; pairs inside the last unit, pairs that straddle its start (the predecessor is
    history), chains of 2 .. 40 members, and pairs whose prefix runs to within 8 / 20 / 240 bytes of the block's end and past it"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, total, dtype=np.uint8)
    sizes = unit_sizes(total)
    last = total - sizes[-1]                      # stream offset of the captured (last) unit
    stale0 = (total - sizes[-1] - sizes[-2]) + sizes[-1]   # input offset of the byte that lies right behind the block's end
    cur_h = [UNIT + 4096]                         # where the next history-side copy goes
    cur_n = [last + 4096]                         # ... and the next copy inside the last unit

    used = np.zeros(total, dtype=bool)

    def place(cur, token, align):
        at = cur[0] + ((align - cur[0]) % 8)
        out[at:at + len(token)] = np.frombuffer(token, dtype=np.uint8)
        used[at:at + len(token)] = True
        cur[0] = at + len(token) + 8
        return at

    def token(L, tails):
        """copies of one text of L bytes behind a 2-byte context; the byte behind it differs between the copies"""
        if L == 3:
            t3, c1, c2 = _collide3(rng)
            body = [t3 + bytes([c]) for c in (c1, c2)]
            ctx = bytes(rng.integers(97, 123, 2).astype(np.uint8))
            return [ctx + body[i % 2] + bytes(rng.integers(0, 256, 4).astype(np.uint8)) for i in range(tails)]
        ctx = bytes(rng.integers(97, 123, 2).astype(np.uint8))
        text = bytes(rng.integers(0, 256, L).astype(np.uint8))
        return [ctx + text + bytes([(7 + 31 * i) % 256]) for i in range(tails)]

    for L in PREFIXES:
        for a in range(8):
            for b in range(8):
                t = token(L, 2)
                # the predecessor in the history for half the alignments, inside the unit for the others
                place(cur_h if (a + b) % 2 else cur_n, t[0], (a - 2) % 8)
                place(cur_n, t[1], (b - 2) % 8)
    for depth in (2, 3, 31, 32, 33, 34, 40):      # chains: a text repeated, every copy with another byte behind it
        t = token(24, depth + 1)
        for i, tk in enumerate(t):
            place(cur_h if i < depth // 2 else cur_n, tk, int(rng.integers(0, 8)))
    assert cur_h[0] < last - 4096 and cur_n[0] < total - 4096
    # a predecessor at the exact distance of every code value of dist_code_up from 2^16 on, and one position further (the two
    # sides of a rounding step; the shorter distances occur by themselves): tokens whose (ctx, 4-gram) key nothing else has
    sdata = np.concatenate([np.zeros(PAD, dtype=np.uint8), out])
    taken = set(np.unique(bucket_key(sdata, np.arange(2, total - 4))).tolist())
    at = last + 300 * 1024
    for v in CODE_VALUES[(CODE_VALUES >= (1 << 16)) & (CODE_VALUES <= (1 << 20))]:
        for d in (int(v), int(v) + 1):
            while used[at - 2:at + 8].any() or used[at - d - 2:at - d + 8].any():
                at += 8
            while True:
                tk = bytes(rng.integers(97, 123, 2).astype(np.uint8)) + bytes(rng.integers(0, 256, 4).astype(np.uint8))
                z = np.concatenate([np.zeros(PAD, dtype=np.uint8), np.frombuffer(tk, dtype=np.uint8), np.zeros(8, dtype=np.uint8)])
                key = int(bucket_key(z, [2])[0])
                if key not in taken:
                    taken.add(key)
                    break
            for where in (at, at - d):
                out[where - 2:where + 4] = np.frombuffer(tk, dtype=np.uint8)
                used[where - 2:where + 8] = True
            at += 16
    assert at < total - 8192
    # prefixes that end near the block's end, and one that runs past it into what the window holds there (convention (a))
    for gap, L in ((6, 5), (18, 16), (230, 225), (3, 40)):
        ctx = bytes(rng.integers(97, 123, 2).astype(np.uint8))
        own = min(L, gap)                          # bytes of the prefix that are the block's own
        text = bytes(rng.integers(0, 256, own).astype(np.uint8))
        at = total - gap - 2
        out[at:at + 2 + own] = np.frombuffer(ctx + text, dtype=np.uint8)
        if L > own:   # the rest of the common prefix is what the window holds behind the block's end
            cont = bytes(out[stale0:stale0 + L - own])
            after = int(out[stale0 + L - own])
        else:
            cont = b""
            after = int(out[at + 2 + own])
        place(cur_h, ctx + text + cont + bytes([(after + 1) % 256]), 0)
    assert cur_h[0] < stale0 - 4096
    return out.tobytes()


def shapes(total=2 * UNIT + 160 * 1024):
    """zeros with noise, periods 1 ('a': the word list's "slot below is p-1"), 3 and 7, in stretches that recur in the history
    and in the last unit: runs deeper than 255, one hot context, sparse history"""
    import _data

    parts = []
    sec = 40 * 1024
    i = 0
    while sum(map(len, parts)) < total:
        which = i % 5
        parts.append([_data.zeros_noise(sec), b"a" * sec, _data.periodic(sec, 3), _data.periodic(sec, 7), _data.periodic(sec, 1)][which])
        i += 1
    return b"".join(parts)[:total]


def far(seed=99):
    """17 MiB of text: the captured unit is the first of the SECOND block (n = 1 MiB + 64 KiB, the short rest joined), so the
    history fills the window and the tail keys come from a block boundary (convention (b)).  For every code value of dist_code_up
    in (2^20, 2^24], a position of that unit whose newest run predecessor lies exactly that far back, and one a position further:
    tokens of bytes the text does not hold (so the copy in the history starts an item) under a key nothing else has"""
    import corpus

    total = BLOCK + UNIT + 64 * 1024
    out = np.frombuffer(corpus.enwik_like(total), dtype=np.uint8).copy()
    rng = np.random.default_rng(seed)
    sdata = np.concatenate([np.zeros(PAD, dtype=np.uint8), out])
    taken = set(np.unique(bucket_key(sdata, np.arange(2, total - 4))).tolist())
    del sdata
    at = BLOCK + 512 * 1024
    for v in CODE_VALUES[(CODE_VALUES > (1 << 20)) & (CODE_VALUES <= (1 << 24))]:
        for d in (int(v), int(v) + 1):
            while True:
                tk = bytes(rng.integers(128, 256, 12).astype(np.uint8))      # four bytes in front, two of context, six of text
                z = np.concatenate([np.zeros(PAD, dtype=np.uint8), np.frombuffer(tk, dtype=np.uint8), np.zeros(8, dtype=np.uint8)])
                key = int(bucket_key(z, [6])[0])
                if key not in taken:
                    taken.add(key)
                    break
            for where in (at, at - d):
                out[where - 6:where + 6] = np.frombuffer(tk, dtype=np.uint8)
            at += 64
    return out.tobytes()


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> (bytes, captured unit): the inputs of both tiers"""
    import _data
    import corpus

    small = corpus.enwik_like(8192)
    d = {
        "text_full_unit": (corpus.enwik_like(2 * UNIT), 1),                  # n = 1 MiB, 1 MiB of history
        "text_last_unit": (corpus.enwik_like(UNIT + 400 * 1024), 1),         # n = 400 KiB, 1 MiB of history
        "shapes": (shapes(), 2),
        "random": (_data.random_bytes(UNIT + 160 * 1024, seed=5), 1),
        "planted": (planted(), 2),
    }
    for n in (1, 63, 64, 65, 4095, 4097):
        d["text_n%d" % n] = (small[:n], 0)
    return d


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """the inputs of the GPU tier alone (the emulation would take minutes for them)"""
    return {"far": (far(), 16)}


# -------------------------------------------------------------------------------------------------------------------- coverage
def true_prefixes(ref):
    """(value, p % 8, q % 8) of every tabulated pair, with the uncapped prefix (up to 304) where the table says 240"""
    n = ref["n"]
    depth, idx, epos = ref["depth"], ref["idx"].astype(np.int64), ref["epos"].astype(np.int64)
    rows = ref["rows"].astype(np.int64)
    vals, pa, qa = [], [], []
    p = np.arange(KPRE, KPRE + n, dtype=np.int64)
    for c in range(K):
        have = np.nonzero(depth > c)[0]
        if not len(have):
            break
        q = epos[idx[have] - 1 - c]
        v = rows[have, c].copy()
        full = np.nonzero(v == MAXLEN)[0]
        if len(full):
            v[full] = ref["text"].lcp(p[have][full], q[full], cap=304)
        vals.append(v); pa.append(p[have] & 7); qa.append(q & 7)
    if not vals:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(vals), np.concatenate(pa), np.concatenate(qa)


def sampled_distances(ref):
    """the distances behind the block's distance codes"""
    rr = np.minimum(K, ref["depth"])
    return set(np.unique(ref["dist"][rr > 0]).tolist())


def dist_gaps(distances, top):
    """code values v of dist_code_up in [16, top] for which the distances v (coded exactly) and v + 1 (rounded up to the next
    code) are not both among `distances`: the two sides of every rounding step"""
    return [int(v) for v in CODE_VALUES if 16 <= v <= top and not ({int(v), int(v) + 1} <= distances)]
