"""A writer of LEGAL orz streams with a free parse (TEST INFRASTRUCTURE).

Every encoder this project has -- the oracle, the device encoders -- follows the reference's parse policy: optimal Huffman
tables, chunks of 2^20 items, the word symbol whenever it applies, matches from the hash chain only, no item past its chunk's
end field.  A decoder has to follow far more than that.  This writer keeps only the state a DECODER has (the ring buckets, the
512 rank tables, words[], after_literal, the window position), knows the data it is writing, and makes seeded random choices
among everything the format can express at each position.  What it writes is legal by construction; the tests hold that to the
oracle's decoder before any other decoder sees a stream (tests/test_freeparse_decoders.py).

Built from the pieces of tests/pyref/orz_py.py (BitWriter, SymRank, Bucket, huffman_lengths, huffman_codes, ROID, write_len).
"""
import random

from pyref.orz_py import (BLOCK, LENIDS, MIN_LEN, NSYMS, PREMATCH, RING, ROID, WORD, BitWriter, Bucket, SymRank, huffman_codes,
                          huffman_lengths, write_len)

NEW = BLOCK - PREMATCH  # bytes a block takes in; the window slides by this much
MAX_ITEM = 255          # len_expected is an 8-bit field of the reference's ring: no decoder follows longer items
ENC_SYMS = 240          # the third table codes enc < 240

COUNTERS = ("literals", "words", "matches", "words_declined", "rank388_literals", "overlapping_matches", "matches_241_255",
            "matches_below_8", "matches_above_32", "chunks", "one_item_chunks", "overruns", "overruns_past_end",
            "overruns_past_end_followed", "declared_above_actual", "tables_with_unused_symbols", "empty_third_tables",
            "codes_13_15_used", "slides")


def _alnum(c):
    return 48 <= c <= 57 or 65 <= c <= 90 or 97 <= c <= 122


def decoded_len(enc, mn, ex):
    """the length a decoder makes of `enc` at a node with len_min mn, len_expected ex, both clamped to at least 4 (lz.rs:459-467)"""
    if enc + mn > ex:
        return enc + mn
    return enc + mn - 1 if enc > 0 else ex


def enc_for(length, mn, ex):
    """an enc < 240 that a decoder turns back into `length`, or None"""
    for enc in (length - mn, length - mn + 1, 0):
        if 0 <= enc < ENC_SYMS and decoded_len(enc, mn, ex) == length:
            return enc
    return None


def lengths_at(lo, hi, mn, ex):
    """the lengths in lo..hi that some enc < 240 codes at a node (mn, ex), ascending: mn..mn+239 and ex itself, less the few at the
    upper edge that the rule does not reach"""
    out = list(range(max(lo, mn), min(hi, mn + ENC_SYMS - 1) + 1))
    if lo <= ex <= hi and not (out and out[0] <= ex <= out[-1]) and enc_for(ex, mn, ex) is not None:
        out.append(ex)
        out.sort()
    while out and enc_for(out[-1], mn, ex) is None:
        out.pop()
    if len(out) > 1 and enc_for(out[-2], mn, ex) is None:
        del out[-2]
    return out


def lcp(data, a, b, cap):
    """length of the common prefix of data[a:] and data[b:], at most cap (slices of bytes are compared, not single bytes)"""
    cap = min(cap, len(data) - max(a, b))
    if cap <= 0:
        return 0
    if data[a:a + cap] == data[b:b + cap]:
        return cap
    lo, hi = 0, cap  # data[a:a+lo] equal, data[a:a+hi] not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if data[a + lo:a + mid] == data[b + lo:b + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def put_table(bw, lens, declared):
    """encode_huffman_table (coder.rs) with any declared maximum at or above the longest length"""
    bw.varint(declared)
    last = None
    for sym, ln in enumerate(lens):
        if ln > 0:
            bw.varint(sym + 1 if last is None else sym - last)
            bw.varint(declared - ln)
            last = sym
    bw.varint(0)


class Writer:
    def __init__(self, data, seed, chunk_items=(1, 400), p_word=0.7, p_match=0.75, p_overrun=0.0, end_overrun=False, p_declared15=0.3,
                 census_max=60, p_longest=0.0, plan=None, table_hook=None, census=None, bad_symbol=None):
        self.data = bytes(data)
        self.n = len(self.data)
        self.rng = random.Random(seed)
        self.chunk_items, self.p_word, self.p_match = chunk_items, p_word, p_match
        self.p_overrun, self.end_overrun, self.p_declared15 = p_overrun, end_overrun, p_declared15
        self.p_longest = p_longest    # how often a match takes the longest length at hand without further ado (long inputs, few items)
        self.plan = plan              # optional: plan(writer, pos) -> None or an item tuple, asked before the random choice
        self.bad_symbol = bad_symbol  # optional: (chunk, item, symbol): that item is coded as `symbol` of its table, 389..511 included
        self.table_hook = table_hook  # optional: table_hook(k, lens, declared) -> (lens, declared) as written (for crafted tables)
        self.buckets = [None] * 256
        self.words = [(0, 0)] * 32768
        self.after_literal = True
        self.base = 0                 # member offset of window offset PREMATCH
        self.out = bytearray()
        self.c = dict.fromkeys(COUNTERS, 0)
        self.c["longest_code"] = [0, 0, 0]
        self.map = {"chunk_ends": [], "overruns": [], "matches": []}
        if census is None:
            census = self.rng.sample(range(NSYMS), self.rng.randint(0, census_max))
        self.census = list(census)
        seen = set(self.census)  # (a census with a repeated entry is written as it is: a crafted stream; the model takes each once)
        first = SymRank(sorted(seen, key=self.census.index) + [s for s in range(NSYMS) if s not in seen])
        self.symranks = [first.clone() for _ in range(512)]
        self.first_chunk = True

    # ---------------------------------------------------------------- what a decoder knows at a position
    def byte(self, off):
        return self.data[off] if off >= 0 else 0  # (window bytes in front of the member are zero)

    def hash1(self, off, byte=None):
        b = byte or self.byte
        return (b(off) & 0x7F) | (int(_alnum(b(off - 1))) << 7)

    def hash2(self, off, byte=None):
        b = byte or self.byte
        return (b(off) & 0x7F) | (self.hash1(off - 1, byte) << 7)

    def bucket(self, ctx):
        if self.buckets[ctx] is None:
            self.buckets[ctx] = Bucket()
        return self.buckets[ctx]

    def node(self, ctx, ro):
        """(member offset of the node's item or None when the node is dead, len_min, len_expected), both clamped"""
        b = self.bucket(ctx)
        k = (b.head + RING - ro) % RING
        p = b.pos[k]
        return (p - PREMATCH + self.base if p > 0 else None), max(b.len_min[k], MIN_LEN), max(b.len_exp[k], MIN_LEN)

    # ---------------------------------------------------------------- choices
    def _ros(self):
        r = self.rng
        return [0, 1, 2, r.randrange(3, 64), r.randrange(RING), r.randrange(RING)]

    def _pick_len(self, feasible):
        r = self.rng
        if self.p_longest and r.random() < self.p_longest:
            return feasible[-1]
        k = r.randrange(6)
        if k == 0:
            return feasible[-1]
        if k == 1:
            return feasible[0]
        if k == 2:
            long_ = [x for x in feasible if x >= 241]
            if long_:
                return r.choice(long_)
        if k == 3:
            short = [x for x in feasible if x < 8]
            if short:
                return r.choice(short)
        return r.choice(feasible)

    def _match(self, pos, ctx, room):
        """a random legal match at pos: (ro, src, len, enc) or None"""
        cands = []
        for ro in self._ros():
            src, mn, ex = self.node(ctx, ro)
            if src is None or src < 0 or src >= pos:
                continue
            l = lcp(self.data, src, pos, min(MAX_ITEM, room))
            if l < MIN_LEN:
                continue
            feasible = lengths_at(MIN_LEN, l, mn, ex)
            if feasible:
                cands.append((ro, src, mn, ex, feasible))
        if not cands:
            return None
        ro, src, mn, ex, feasible = self.rng.choice(cands)
        ln = self._pick_len(feasible)
        return ro, src, ln, enc_for(ln, mn, ex)

    def _overrun(self, pos, ctx, room, must_pass=0):
        """a match at pos that claims `big` bytes of which the first `keep` are the data's: (ro, src, big, enc, keep) or None.
        must_pass: big has to exceed it (the bytes left in the member, for an overrun past its end)"""
        cands = []
        for ro in self._ros() + [self.rng.randrange(8) for _ in range(4)]:
            src, mn, ex = self.node(ctx, ro)
            if src is None or src < 0 or src >= pos:
                continue
            l = lcp(self.data, src, pos, min(MAX_ITEM, self.n - pos))
            if l < 1:
                continue
            bigs = lengths_at(max(MIN_LEN, must_pass + 1), min(MAX_ITEM, room), mn, ex)
            if bigs:
                cands.append((ro, src, mn, ex, l, bigs))
        if not cands:
            return None
        ro, src, mn, ex, l, bigs = self.rng.choice(cands)
        big = self.rng.choice(bigs)
        top = min(l, big - 1)
        if must_pass and top > 1 and self.rng.random() < 0.9:
            top = min(top, must_pass - 1) or 1  # (leave bytes of the member for a chunk to follow)
        keep = self.rng.randint(1, max(top, 1))
        if keep >= big:
            return None
        return ro, src, big, enc_for(big, mn, ex), keep

    # ---------------------------------------------------------------- the stream
    def run(self):
        data, n, rng = self.data, self.n, self.rng
        pos = 0
        while pos < n:
            block_end = min(n, self.base + NEW)
            tail_zone = self.end_overrun and n - pos <= 260
            target = rng.randint(1, 8) if tail_zone else rng.randint(*self.chunk_items)
            want_overrun = tail_zone or rng.random() < self.p_overrun
            items, end = [], None
            while pos < block_end and end is None:
                ctx = self.hash1(pos - 1)
                expected = self.words[self.hash2(pos - 1)]
                unlikely = expected[0]
                sr = self.symranks[ctx | (int(self.after_literal) << 8)]
                al = int(self.after_literal)
                room = block_end - pos
                wpos = PREMATCH + pos - self.base
                if want_overrun and len(items) >= target - 1 and len(items) < target + 60:
                    window_room = self.base + NEW - pos  # (the reference refuses an item that ends beyond the block)
                    o = self._overrun(pos, ctx, window_room if tail_zone else min(window_room, n - pos), n - pos if tail_zone else 0)
                    if o is not None:
                        ro, src, big, enc, keep = o
                        sim = bytearray(big)
                        for k in range(big):
                            sim[k] = data[src + k] if src + k < pos else sim[src + k - pos]
                        assert bytes(sim[:keep]) == data[pos:pos + keep]
                        roid, robitlen, robits = ROID[ro]
                        items.append((al, sr.encode(256 + roid * LENIDS + min(LENIDS - 1, enc), unlikely), True, robitlen, robits, enc))
                        self.bucket(ctx).update(wpos, ro, big)
                        at = lambda off: sim[off - pos] if off >= pos else self.byte(off)
                        self.words[self.hash2(pos + big - 3, at)] = (at(pos + big - 2), at(pos + big - 1))
                        self.after_literal = False
                        self.c["matches"] += 1
                        self.c["overruns"] += 1
                        if src + big > pos:
                            self.c["overlapping_matches"] += 1
                        self.map["overruns"].append({"pos": pos, "keep": keep, "big": big, "src": src, "chunk": self.c["chunks"]})
                        if pos + big > n:
                            self.c["overruns_past_end"] += 1
                            if pos + keep < n:
                                self.c["overruns_past_end_followed"] += 1
                        pos += keep
                        end = pos
                        break
                item = self.plan(self, pos) if self.plan else None
                word_ok = room >= 2 and (data[pos], data[pos + 1]) == expected
                m = None
                if item is None and rng.random() < self.p_match:
                    m = self._match(pos, ctx, room)
                if item is not None:
                    kind = item[0]
                    if kind == "match":
                        m = item[1:]
                elif word_ok and rng.random() < self.p_word:
                    kind, m = "word", None
                elif m is not None:
                    kind = "match"
                else:
                    kind = "literal"
                    if word_ok:
                        self.c["words_declined"] += 1
                if kind == "match":
                    ro, src, ln, enc = m
                    roid, robitlen, robits = ROID[ro]
                    items.append((al, sr.encode(256 + roid * LENIDS + min(LENIDS - 1, enc), unlikely), True, robitlen, robits, enc))
                    self.bucket(ctx).update(wpos, ro, ln)
                    self.c["matches"] += 1
                    self.c["overlapping_matches"] += src + ln > pos
                    self.c["matches_241_255"] += ln >= 241
                    self.c["matches_below_8"] += ln < 8
                    self.c["matches_above_32"] += ln > 32
                    if len(self.map["matches"]) < 4096:
                        self.map["matches"].append((pos, src, ln))
                    pos += ln
                    self.after_literal = False
                    self.words[self.hash2(pos - 3)] = (self.byte(pos - 2), self.byte(pos - 1))
                elif kind == "word":
                    items.append((al, sr.encode(WORD, unlikely), False, 0, 0, 0))
                    self.bucket(ctx).update(wpos, 0, 0)
                    self.c["words"] += 1
                    pos += 2
                    self.after_literal = False
                else:
                    r = sr.encode(data[pos], unlikely)
                    items.append((al, r, False, 0, 0, 0))
                    self.bucket(ctx).update(wpos, 0, 0)
                    self.c["literals"] += 1
                    self.c["rank388_literals"] += r == NSYMS - 1
                    pos += 1
                    self.after_literal = True
                    self.words[self.hash2(pos - 3)] = (self.byte(pos - 2), self.byte(pos - 1))
                if len(items) >= (target + 60 if want_overrun else target):
                    end = pos
            if end is None:
                end = pos
            self._chunk(items, PREMATCH + end - self.base)
            self.map["chunk_ends"].append(end)
            if pos - self.base >= NEW:  # the decoder slides here (lib.rs:119-124)
                for b in self.buckets:
                    if b is not None:
                        b.forward(NEW)
                self.base += NEW
                self.c["slides"] += 1
        self.out += write_len(0)
        self.c["map"] = self.map
        return bytes(self.out), self.c

    def _lengths(self, k, used, size):
        """code lengths over random weights for the used symbols of table k, a few unused ones besides"""
        rng = self.rng
        weights = [0] * size
        for s in used:
            weights[s] = 1 << rng.randrange(21)
        if used:
            extra = [s for s in (rng.randrange(size) for _ in range(rng.randint(0, 4))) if s not in used]
            for s in extra:
                weights[s] = 1 << rng.randrange(21)
            self.c["tables_with_unused_symbols"] += bool(extra)
        lens = huffman_lengths(weights)
        actual = max(lens)
        declared = 15 if actual and rng.random() < self.p_declared15 else actual
        if self.table_hook:
            lens, declared = self.table_hook(k, lens, declared)
        self.c["declared_above_actual"] += declared > max(lens)
        self.c["longest_code"][k] = max(self.c["longest_code"][k], max(lens))
        return lens, declared

    def _chunk(self, items, end_field):
        bw = BitWriter()
        if self.first_chunk:
            bw.varint(len(self.census))
            for s in self.census:
                bw.put(9, s)
            self.first_chunk = False
        bw.varint(end_field)
        bw.varint(len(items))
        used = [set(), set(), set()]
        sizes = [NSYMS, NSYMS, ENC_SYMS]
        swap = None
        if self.bad_symbol and self.bad_symbol[0] == self.c["chunks"]:
            swap = (min(self.bad_symbol[1], len(items) - 1), self.bad_symbol[2])
            used[items[swap[0]][0]].add(swap[1])
            sizes[items[swap[0]][0]] = 512
        for al, r, is_match, _, _, enc in items:
            used[al].add(r)
            if is_match and enc >= LENIDS - 1:
                used[2].add(enc)
        tables = [self._lengths(k, used[k], sizes[k]) for k in range(3)]
        self.c["empty_third_tables"] += tables[2][1] == 0
        for lens, declared in tables:
            put_table(bw, lens, declared)
        codes = [huffman_codes(lens) for lens, _ in tables]
        for j, (al, r, is_match, robitlen, robits, enc) in enumerate(items):
            code, ln = codes[al][swap[1] if swap and swap[0] == j else r]
            bw.put(ln, code)
            self.c["codes_13_15_used"] += ln >= 13
            if is_match:
                bw.put(robitlen, robits)
                if enc >= LENIDS - 1:
                    code, ln = codes[2][enc]
                    bw.put(ln, code)
                    self.c["codes_13_15_used"] += ln >= 13
        chunk = bw.finish()
        self.out += write_len(len(chunk)) + chunk
        self.c["chunks"] += 1
        self.c["one_item_chunks"] += len(items) == 1


def write(data, seed, **knobs):
    """(stream, counters): one complete orz stream that decodes to `data`; counters["map"] says where chunks and overruns lie"""
    return Writer(data, seed, **knobs).run()


# ------------------------------------------------------------------------------------------------ the named cases
def make_input(kind, size, seed):
    """the inputs the named cases (tests/golden/freeparse_cases.json) speak of"""
    import _data

    if kind == "text":
        return _data.text(size)
    if kind == "mixed":
        return _data.mixed(size)
    if kind == "periodic":
        return _data.periodic(size, 3)
    if kind == "zeros_noise":
        return _data.zeros_noise(size)
    if kind == "tailed":  # text, then 700 bytes of short repeated patterns: long matches are at hand where the member ends
        rng = random.Random(1000 + seed)
        tail = bytearray()
        while len(tail) < 700:
            tail += bytes(rng.randrange(97, 101) for _ in range(rng.randint(1, 5))) * rng.randint(3, 30)
        return _data.text(size - 700, seed=seed + 1) + bytes(tail[:700])
    raise ValueError(kind)


class Case:
    def __init__(self, suite, spec):
        self.suite, self.spec = suite, spec
        self.name = "%s/%s-%d" % (suite, spec["input"], spec["seed"])
        self.data = make_input(spec["input"], spec["size"], spec["seed"])
        knobs = dict(spec.get("knobs", {}))
        if "chunk_items" in knobs:
            knobs["chunk_items"] = tuple(knobs["chunk_items"])
        self.stream, self.counters = write(self.data, spec["seed"], **knobs)
        self.map = self.counters["map"]


def load_cases(only=None):
    """{suite: [Case]} of the named cases, generated here (the file holds seeds and knob values only)"""
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freeparse_cases.json")
    suites = json.load(open(path))["suites"]
    return {s: [Case(s, spec) for spec in specs] for s, specs in suites.items() if only is None or s in only}


def total(cases, key):
    return sum(c.counters[key] for c in cases)


SUITES = ("plain", "overrun", "end-overrun")


def container(suites, oracle):
    """(parts, streams): every free-parse member of every suite, an oracle-encoded member after every third"""
    import _data

    parts, streams = [], []
    k = 0
    for s in SUITES:
        for c in suites[s]:
            parts.append(c.data)
            streams.append(c.stream)
            k += 1
            if k % 3 == 0:
                d = _data.mixed(1500 + 97 * k, seed=k)
                parts.append(d)
                streams.append(oracle.encode(d, k % 3))
    return parts, streams


def starts(lengths):
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += n
    return out


def member_ranges(c, rng):
    """[(what, member offset, length)] of one free-parse member: random ranges and ranges placed by the writer's map"""
    n = len(c.data)
    out = []
    for _ in range(4):
        ln = rng.choice([1, 2, 17, rng.randrange(1, 600)])
        out.append(("random", rng.randrange(0, n - ln + 1), ln))
    ends = c.map["chunk_ends"]
    over_chunks = [o["chunk"] for o in c.map["overruns"]]
    picks = sorted(set(over_chunks[:2] + over_chunks[-2:] + [rng.randrange(len(ends)) for _ in range(2)]))
    for k in picks:
        lo, e = (ends[k - 1] if k else 0), ends[k]
        nxt = ends[k + 1] if k + 1 < len(ends) else n
        if e > lo:
            out.append(("a chunk exactly", lo, e - lo))
        if nxt > e:
            out.append(("from an end field to the next", e, nxt - e))
        if 0 < e < n:
            out.append(("one byte each side of an end field", e - 1, 2))
        if lo > 0 and e + 1 <= n:
            out.append(("a chunk and one byte each side", lo - 1, e + 1 - (lo - 1)))
    for o in c.map["overruns"][:2] + c.map["overruns"][-2:]:
        out.append(("the kept part of an overrunning item", o["pos"], o["keep"]))
        out.append(("inside the kept part", o["pos"] + o["keep"] // 2, o["keep"] - o["keep"] // 2))
        if o["pos"] + o["keep"] < n:
            out.append(("just behind an overrunning item", o["pos"] + o["keep"], min(9, n - o["pos"] - o["keep"])))
    return out


RANGE_KINDS = {"a chunk exactly", "from an end field to the next", "one byte each side of an end field", "a chunk and one byte each side",
               "the kept part of an overrunning item", "inside the kept part", "just behind an overrunning item", "random"}


def read_rounds(parts, suites):
    """the reads of container()'s members, round by round as [(offset in the decoded data, length, what)]: round k asks every
    member for its k-th range, a member's ranges in increasing order -- so a member stops somewhere else in every round, and a
    cursor goes on from where the round before left it, inside and right behind the overrun chunks"""
    by_data = {c.data: c for s in SUITES for c in suites[s]}
    rng = random.Random(31)
    per = []
    for p, at in zip(parts, starts([len(p) for p in parts])):
        c = by_data.get(p)
        rs = member_ranges(c, rng) if c else [("random", rng.randrange(0, len(p) - 40), 40) for _ in range(3)]
        per.append(sorted(set((at + o, ln, what) for what, o, ln in rs if ln > 0)))
    assert {w for rs in per for _, _, w in rs} == RANGE_KINDS
    return [[rs[k] for rs in per if k < len(rs)] for k in range(max(len(rs) for rs in per))]


# ------------------------------------------------------------------------------------------------ the window-slide case
SLIDE_KEY = b"Q\x01"  # the two bytes in front of offset 2: an alphanumeric and 0x01 make a context (129) no other position of the input has
SLIDE_WORD = bytes(range(0xA0, 0xC8))  # 40 bytes that follow them, at offset 2 and once more behind the slide


def slide_input(extra=5000, seed=3):
    """one member of 2^24 + extra bytes, nearly all long runs of bytes that are neither alphanumeric nor 0x01 (so the context of
    SLIDE_KEY occurs where it is planted and nowhere else); SLIDE_KEY + SLIDE_WORD at offset 0 and again 1000 bytes behind the
    point where the window slides.  Returns (data, the offset of the second SLIDE_WORD)."""
    rng = random.Random(seed)
    pool = [0x20, 0x80, 0x8F, 0x90, 0xFE]
    out = bytearray(SLIDE_KEY + SLIDE_WORD)
    n = NEW + extra
    while len(out) < n:
        out += bytes([rng.choice(pool)]) * rng.randint(3000, 60000)
    del out[n:]
    again = NEW + 1000
    out[again - 3] = 0x20  # (not the context of offset 0, whose two bytes in front are zero)
    out[again - 2:again + len(SLIDE_WORD)] = SLIDE_KEY + SLIDE_WORD
    return bytes(out), again


def write_slide(seed=1):
    """(data, stream, counters): slide_input() by the free-parse writer, taking the longest match nearly always (some 10^5 items).
    The item at the second SLIDE_WORD is a match from the ring node of offset 2 -- window offset 1 once the window has slid, the
    last position that is still alive -- in a context that has seen one item; counters["slide_match"] says where it was made."""
    data, again = slide_input()
    fired = []

    def plan(w, pos):
        if pos != again:
            return None
        src, mn, ex = w.node(129, 0)
        assert w.hash1(pos - 1) == 129 and src == 2 and w.base == NEW and w.bucket(129).pos[w.bucket(129).head] == 1
        fired.append(pos)
        return ("match", 0, 2, len(SLIDE_WORD), enc_for(len(SLIDE_WORD), mn, ex))

    stream, c = write(data, seed, chunk_items=(200, 3000), p_longest=0.97, p_match=0.98, p_word=0.02, plan=plan)
    c["slide_match"] = fired
    return data, stream, c
