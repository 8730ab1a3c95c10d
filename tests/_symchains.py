"""Adversarial inputs for the symbol-ranking chain (orz_symrank_kernel behind orz_symrank_chains / emu_symrank), the plain
reference they are held to, and a model of the kernel's dispatch rules that says which of its paths an input reaches.

A launch is 512 contexts' tables in the encoder's layout ([512, 782] u16: value[389], index[389], cnt lo/hi, sum lo/hi),
gsym (symbol | excluded symbol << 16, grouped by context) and rstart[513].  Everything is generated from a seed at test time.

The reference is tests/pyref/orz_py.py's SymRank (SymRankCoder, src/symrank.rs:13-97, with Rust integer semantics).
`path_model` replays the kernel's rules -- NOT its code -- from the reference's own count/sum sequence:
  * a context's items go one at a time (plain) while count < 192 or fewer than 32 remain, else in groups of 32;
  * a group is run speculatively when it starts with count >= 327 and quotient q = sum / 16 / count < 32, and the
    speculation holds when the quotient after every one of its 32 items is still q;
  * the group's 9/10 scaling falls on lane r = 390 - count (none when r >= 32).
"""
import numpy as np

from pyref.orz_py import NSYMS, SymRank

WORDS = NSYMS * 2 + 4
MAX_SUM = 1000000 + 390 * (NSYMS - 1)
FRESH_SUM = 1000000


# ------------------------------------------------------------------------------------------------ tables and launches
def table_row(order, cnt=0, sum_=FRESH_SUM):
    row = np.zeros(WORDS, dtype=np.uint16)
    order = np.asarray(order, dtype=np.int64)
    row[:NSYMS] = order
    row[NSYMS + order] = np.arange(NSYMS)
    row[2 * NSYMS], row[2 * NSYMS + 1] = cnt & 0xFFFF, cnt >> 16
    row[2 * NSYMS + 2], row[2 * NSYMS + 3] = sum_ & 0xFFFF, sum_ >> 16
    return row


def census_order(counts):
    """CensusOrder / src/lz.rs:247-250: stable sort of the symbols by descending max(count, 1)"""
    return sorted(range(NSYMS), key=lambda s: (-max(int(counts[s]), 1), s))


def coder_of(row):
    c = SymRank()
    c.value = [int(x) for x in row[:NSYMS]]
    c.index = [int(x) for x in row[NSYMS:2 * NSYMS]]
    c.cnt = int(row[2 * NSYMS]) | (int(row[2 * NSYMS + 1]) << 16)
    c.sum = int(row[2 * NSYMS + 2]) | (int(row[2 * NSYMS + 3]) << 16)
    return c


def row_of(coder):
    return table_row(coder.value, coder.cnt, coder.sum)


class Launch:
    """one launch: tables [512, WORDS] and per-context item lists (symbol, excluded symbol)"""

    def __init__(self, name, tables=None):
        self.name = name
        self.tables = tables if tables is not None else np.tile(table_row(range(NSYMS)), (512, 1))
        self.items = [[] for _ in range(512)]

    def arrays(self):
        """-> (gsym uint32, rstart uint32[513])"""
        lens = [len(it) for it in self.items]
        rstart = np.zeros(513, dtype=np.uint32)
        rstart[1:] = np.cumsum(lens)
        flat = [v | (u << 16) for it in self.items for (v, u) in it]
        return np.array(flat, dtype=np.uint32), rstart


def reference(tables, gsym, rstart):
    """the plain loop over every context -> (ranks uint16, tables out, {ctx: (cnt0, sum0, raw ranks i)})"""
    ranks = np.zeros(len(gsym), dtype=np.uint16)
    out = np.array(tables, dtype=np.uint16, copy=True)
    raw = {}
    g = [int(x) for x in gsym]
    for c in range(512):
        a, e = int(rstart[c]), int(rstart[c + 1])
        if a == e:
            continue
        coder = coder_of(tables[c])
        cnt0, sum0 = coder.cnt, coder.sum
        idx = coder.index
        ii = []
        for k in range(a, e):
            v, u = g[k] & 0xFFFF, g[k] >> 16
            ii.append(idx[v])
            ranks[k] = coder.encode(v, u)
        raw[c] = (cnt0, sum0, ii)
        out[c] = row_of(coder)
    return ranks, out, raw


# ------------------------------------------------------------------------------------------------ the path model
def _step(cnt, sum_, i):
    if cnt > NSYMS:
        cnt, sum_ = cnt * 9 // 10, sum_ * 9 // 10
    return cnt + 1, sum_ + i


def path_model(cnt, sum_, ii):
    """the kernel's dispatch over one context's chain (start count/sum, raw ranks i = index[symbol] before each item) ->
    dict: plain (items), groups [dict(cnt, q, r, spec, ok, bad)], tail (items left plain after count reached 192, or None)"""
    n, j = len(ii), 0
    groups, plain, tail = [], 0, None
    while j < n:
        if cnt >= 192 and n - j >= 32:
            while n - j >= 32:
                q = (sum_ >> 4) // cnt
                g = dict(cnt=cnt, q=q, r=NSYMS + 1 - cnt, spec=cnt >= 327 and q < 32, bad=None, edge_only=True)
                for k in range(32):
                    cnt, sum_ = _step(cnt, sum_, ii[j + k])
                    if g["bad"] is None and (sum_ >> 4) // cnt != q:
                        g["bad"] = k
                    # (the quotient at most touches q + 1: the sum lies on the upper edge of q's interval, not beyond)
                    g["edge_only"] &= 16 * q * cnt <= sum_ <= 16 * (q + 1) * cnt
                g["edge_only"] &= g["bad"] is not None
                g["ok"] = g["spec"] and g["bad"] is None
                groups.append(g)
                j += 32
            tail = n - j
            continue
        if cnt >= 192 and tail is None:
            tail = n - j
        cnt, sum_ = _step(cnt, sum_, ii[j])
        plain += 1
        j += 1
    return dict(plain=plain, groups=groups, tail=tail)


class Coverage:
    """what a set of launches made the kernel do, by the path model"""

    def __init__(self):
        self.spec_ok = self.spec_fail = self.checked = 0
        self.fail_lanes = set()        # ("0" / "31" / "r-1" / "r" / k) of failed speculations
        self.r_ok, self.r_checked = set(), set()
        self.tails, self.start_cnts = set(), set()
        self.checked_q32 = 0
        self.edge_only = 0             # failed speculations whose sums at most touch the upper edge of q's interval
        self.out_ranks = set()

    def add(self, raw, ranks):
        for cnt0, sum0, ii in raw.values():
            m = path_model(cnt0, sum0, ii)
            if m["tail"] is not None:
                self.tails.add(m["tail"])
            for g in m["groups"]:
                self.start_cnts.add(g["cnt"])
                r = g["r"]
                if g["ok"]:
                    self.spec_ok += 1
                    if r < 32:
                        self.r_ok.add(r)
                    continue
                if g["spec"]:
                    self.spec_fail += 1
                    self.edge_only += g["edge_only"]
                    b = g["bad"]
                    self.fail_lanes.add(b)
                    if r < 32 and b == r - 1:
                        self.fail_lanes.add("r-1")
                    if r < 32 and b == r:
                        self.fail_lanes.add("r")
                self.checked += 1
                if r < 32:
                    self.r_checked.add(r)
                if g["q"] >= 32:
                    self.checked_q32 += 1
        self.out_ranks.update(int(x) for x in np.unique(ranks))

    def summary(self):
        return dict(spec_ok=self.spec_ok, spec_fail=self.spec_fail, edge_only=self.edge_only, checked=self.checked, checked_q32=self.checked_q32,
                    fail_lanes=sorted(str(x) for x in self.fail_lanes), r_ok=len(self.r_ok), r_checked=len(self.r_checked),
                    tails=len(self.tails), cnt192=192 in self.start_cnts, cnt327=327 in self.start_cnts,
                    out_ranks_0_387_388=sorted(self.out_ranks & {0, 387, 388}))


# ------------------------------------------------------------------------------------------------ chain drivers
class Driver:
    """builds one context's chain item by item on a reference coder, so that ranks can be aimed at"""

    def __init__(self, rng, row):
        self.rng = rng
        self.coder = coder_of(row)
        self.items = []

    def after(self, i):
        return _step(self.coder.cnt, self.coder.sum, i)

    def interval(self, target_q):
        """raw ranks i whose item leaves quotient target_q: [lo, hi] (empty: lo > hi)"""
        c1, s1 = _step(self.coder.cnt, self.coder.sum, 0)
        lo = max(0, 16 * target_q * c1 - s1)
        hi = min(NSYMS - 1, 16 * (target_q + 1) * c1 - 1 - s1)
        return lo, hi

    def quotient(self):
        return (self.coder.sum >> 4) // max(self.coder.cnt, 1)

    def push(self, i, unl=None):
        """the item whose symbol sits at rank i; excluded symbol: `unl` (a symbol), else a random one"""
        v = self.coder.value[i]
        u = int(self.rng.integers(NSYMS)) if unl is None else unl
        self.coder.encode(v, u)
        self.items.append((v, u))
        return v

    def push_sym(self, v, u):
        self.coder.encode(v, u)
        self.items.append((v, u))

    def rand_rank(self, skew=True):
        """mostly small ranks, as on real data, now and then any"""
        if skew and self.rng.random() < 0.9:
            return min(NSYMS - 1, int(self.rng.geometric(0.12)) - 1)
        return int(self.rng.integers(NSYMS))

    def aim(self, target_q, fallback_low=True):
        lo, hi = self.interval(target_q)
        if lo <= hi:
            return int(self.rng.integers(lo, hi + 1))
        return 0 if fallback_low else NSYMS - 1


def _zipf_counts(rng):
    c = np.zeros(NSYMS, dtype=np.int64)
    w = 1.0 / (1.0 + np.arange(NSYMS)) ** 1.1
    c[rng.permutation(NSYMS)] = (w * 100000).astype(np.int64)
    c[rng.integers(0, NSYMS, 60)] = rng.integers(0, 2, 60)  # some symbols seen once or never: max(count, 1) ties
    return c


def _fill(launch, ctx, drv):
    launch.items[ctx] = drv.items


# family a: fresh contexts (count 0, sum 1,000,000, census order) at every length that changes how the chain is split
def family_a(seed=1):
    rng = np.random.default_rng(seed)
    order = census_order(_zipf_counts(rng))
    L = Launch("a: fresh contexts", np.tile(table_row(order), (512, 1)))
    lens = [1, 31, 32, 33, 191, 192, 193, 223, 224, 225]
    lens += [192 + 32 * (1 + t % 3) + t for t in range(32)]  # after 1..3 groups every tail 0..31
    lens += [4000]  # decays into the steady state: speculative groups, the 9/10 scaling
    for k, n in enumerate(lens):
        drv = Driver(rng, L.tables[k])
        for _ in range(n):
            drv.push(drv.rand_rank())
        _fill(L, k, drv)
    return [L]


def _steady_row(rng, cnt, sum_):
    return table_row(rng.permutation(NSYMS), cnt, sum_)


def _aimed_chain(drv, q, move_lane, direction, nitems):
    """keep the quotient at q, move it by `direction` at item move_lane (None: never), then ranks at random"""
    for k in range(nitems):
        if move_lane is None or k < move_lane:
            drv.push(drv.aim(q))
        elif k == move_lane:
            i = drv.aim(q + direction, fallback_low=direction < 0)
            drv.push(i)
        else:
            drv.push(drv.rand_rank())


# family b: steady-state starts -- every scaling lane, sums at both edges of the quotient's interval, aimed moves
def family_b(seed=2):
    rng = np.random.default_rng(seed)
    launches = []
    L = Launch("b: steady-state starts")
    ctx = 0
    cnts = list(range(327, 391))  # r = 390 - cnt: 63..0 (32 and 63 included)
    qs = [0, 1, 31, 32, 33]
    edges = [0, 1, -2, -1]
    combo = 0
    for cnt in cnts:
        r = 390 - cnt
        lanes = [None, 0, 31] + ([r - 1] if 0 < r <= 32 else []) + ([r] if r < 32 else [])
        for lane in lanes:
            for direction in ((1,) if lane is None else (1, -1)):
                q = qs[combo % len(qs)]
                e = edges[(combo // len(qs)) % len(edges)]
                combo += 1
                sum_ = 16 * q * cnt + (e if e >= 0 else 16 * cnt + e)
                if sum_ > MAX_SUM:
                    continue
                drv = Driver(rng, _steady_row(rng, cnt, sum_))
                L.tables[ctx] = row_of(drv.coder)
                nitems = 64 + int(rng.integers(0, 32)) if lane is None else 32 + int(rng.integers(0, 40))
                _aimed_chain(drv, q, lane, direction, nitems)
                _fill(L, ctx, drv)
                ctx += 1
                if ctx == 512:
                    launches.append(L)
                    L, ctx = Launch("b: steady-state starts"), 0
    # the sum lands exactly on the upper edge of q's interval (the quotient becomes q + 1 by the smallest margin) at one lane,
    # and stays within q's interval or on its edge after it: a check that lets the edge pass would accept the group
    for cnt in range(327, 391):
        r = 390 - cnt
        for lane in (0, 31, r - 1, r, int(rng.integers(0, 32))):
            if not 0 <= lane < 32:
                continue
            q = (0, 1, 5, 22)[(cnt + lane) % 4]
            drv = Driver(rng, _steady_row(rng, cnt, 16 * (q + 1) * cnt - 1))
            L.tables[ctx] = row_of(drv.coder)
            hit = False
            for k in range(32 + int(rng.integers(0, 8))):
                lo, hi = drv.interval(q)
                if k < lane or (not hit and hi + 1 > NSYMS - 1):
                    drv.push(max(0, min(hi, NSYMS - 1)))
                elif not hit:
                    drv.push(hi + 1)
                    hit = True
                else:
                    top = max(0, min(hi + 1, NSYMS - 1))
                    drv.push(top if rng.random() < 0.5 or lo > top else int(rng.integers(max(lo, 0), top + 1)))
            _fill(L, ctx, drv)
            ctx += 1
            if ctx == 512:
                launches.append(L)
                L, ctx = Launch("b: steady-state starts"), 0
    # checked groups with a large quotient (q >= 256 needs count <= 281 under the largest sum) and q 32, 33 at the edges
    for cnt, q in [(192, 256), (200, 300), (240, 280), (281, 256), (192, 374), (250, 40), (300, 100), (327, 32), (390, 33)]:
        for e in (0, 16 * cnt - 1):
            sum_ = min(16 * q * cnt + e, MAX_SUM)
            drv = Driver(rng, _steady_row(rng, cnt, sum_))
            L.tables[ctx] = row_of(drv.coder)
            for _ in range(96 + int(rng.integers(0, 32))):
                drv.push(drv.rand_rank(skew=False))
            _fill(L, ctx, drv)
            ctx += 1
    # regression: a context that starts with count 0 and a sum of 2^20 or more -- its first quotient is 2^16 or more and
    # wraps in the reference's u16 arithmetic (the kernel's plain loop once computed it in 32 bits)
    for sum_ in (1048576 - 400, 1048576, 1048576 + 3000, 1050000, 1054000, MAX_SUM):
        for first in (0, 17, 100, 250, 388):
            drv = Driver(rng, _steady_row(rng, 0, sum_))
            L.tables[ctx] = row_of(drv.coder)
            drv.push(first)
            for _ in range(int(rng.integers(0, 40))):
                drv.push(drv.rand_rank())
            _fill(L, ctx, drv)
            ctx += 1
    launches.append(L)
    return launches


def _steady_start(rng, launch, ctx, q=None):
    cnt = int(rng.integers(327, 391))
    q = int(rng.integers(0, 4)) if q is None else q
    drv = Driver(rng, _steady_row(rng, cnt, 16 * q * cnt + int(rng.integers(0, 16 * cnt))))
    launch.tables[ctx] = row_of(drv.coder)
    return drv


def _rotation_n(drv, i):
    c1, s1 = drv.after(i)
    dec = (i // 16 + (((s1 // 16) // c1) & 0xFFFF)) & 0xFFFF
    nxt = max(i - dec if i > dec else 0, i // 2)
    return i - nxt


# family c: symbol patterns -- duplicates among the tracked lanes, every rotation size, the last ranks, the excluded symbol
def family_c(seed=3):
    rng = np.random.default_rng(seed)
    L = Launch("c: symbol patterns")
    ctx = 0

    def chain(n, fresh=False):
        nonlocal ctx
        if fresh:
            drv = Driver(rng, table_row(rng.permutation(NSYMS)))
            L.tables[ctx] = row_of(drv.coder)
        else:
            drv = _steady_start(rng, L, ctx)
        ctx += 1
        return drv, n

    for rep in range(8):
        # the same symbol over and over (excluded: random, or the symbol itself now and then)
        drv, n = chain(64 + 32 * (rep % 3) + rep)
        v = int(rng.integers(NSYMS))
        for _ in range(n):
            drv.push_sym(v, v if rng.random() < 0.2 else int(rng.integers(NSYMS)))
        _fill(L, ctx - 1, drv)
        # two symbols alternating, three in turn
        drv, n = chain(96 + rep)
        vs = [int(x) for x in rng.choice(NSYMS, 2 + rep % 2, replace=False)]
        for k in range(n):
            drv.push_sym(vs[k % len(vs)], int(rng.integers(NSYMS)))
        _fill(L, ctx - 1, drv)
        # rotations of a given size n = i - next_i: 0, 1, 2, 3 and larger
        for want in (0, 1, 2, 3, 5, 17, 100):
            drv, n = chain(64 + rep * 5)
            for _ in range(n):
                cands = [i for i in range(NSYMS) if _rotation_n(drv, i) == want]
                drv.push(int(rng.choice(cands)) if cands and rng.random() < 0.8 else drv.rand_rank())
            _fill(L, ctx - 1, drv)
        # the last ranks: 388, 387, ... (the sum climbs: quotient moves, failed speculation)
        drv, n = chain(64 + rep)
        for _ in range(n):
            drv.push(NSYMS - 1 - int(rng.integers(0, 8)) if rng.random() < 0.7 else drv.rand_rank())
        _fill(L, ctx - 1, drv)
        # match symbols 256..388 with literal excluded symbols
        drv, n = chain(80 + rep)
        for _ in range(n):
            drv.push_sym(int(rng.integers(256, NSYMS)), int(rng.integers(0, 256)))
        _fill(L, ctx - 1, drv)
        # the symbol is the excluded one (rank 388 out), and the excluded symbol is the one at rank 388 / rank 387
        drv, n = chain(64 + rep)
        for k in range(n):
            i = drv.rand_rank()
            v = drv.coder.value[i]
            m = k % 4
            u = v if m == 0 else drv.coder.value[NSYMS - 1] if m == 1 else drv.coder.value[NSYMS - 2] if m == 2 else None
            drv.push(i, u)
        _fill(L, ctx - 1, drv)
        # the excluded symbol is one that this item's rotation moves (the symbols at next_i and at the mid point)
        drv, n = chain(64 + 3 * rep)
        for _ in range(n):
            i = drv.rand_rank(skew=rng.random() < 0.5)
            c1, s1 = drv.after(i)
            dec = (i // 16 + (((s1 // 16) // c1) & 0xFFFF)) & 0xFFFF
            nxt = max(i - dec if i > dec else 0, i // 2)
            mid = nxt + (i - nxt) // 2
            drv.push(i, drv.coder.value[nxt if rng.random() < 0.5 else mid])
        _fill(L, ctx - 1, drv)
        # the excluded symbol is the previous item's symbol, or the next one's
        drv, n = chain(64 + rep)
        prev = int(rng.integers(NSYMS))
        for _ in range(n):
            i = drv.rand_rank()
            v = drv.push(i, prev)
            prev = v
        _fill(L, ctx - 1, drv)
        drv, n = chain(64 + rep)
        ranks = [drv.rand_rank() for _ in range(n + 1)]
        for k in range(n):
            v = drv.coder.value[ranks[k]]
            # the symbol the next item will take: whatever sits at its rank once this item has moved its symbols
            nxt_coder = drv.coder.clone()
            nxt_coder.encode(v, 0)
            drv.push(ranks[k], nxt_coder.value[ranks[k + 1]])
        _fill(L, ctx - 1, drv)
    # the same patterns from fresh tables (plain loop, checked groups with a large quotient)
    for rep in range(4):
        drv, n = chain(260 + rep * 13, fresh=True)
        v = int(rng.integers(NSYMS))
        for k in range(n):
            drv.push_sym(v if k % 3 else int(rng.integers(NSYMS)), v if k % 5 == 0 else int(rng.integers(NSYMS)))
        _fill(L, ctx - 1, drv)
    assert ctx <= 512
    return [L]


# family d: layout -- every context populated with its own length, one hot context, empty contexts between populated ones,
# random tables (any permutation, any count and sum in range)
def family_d(seed=4):
    rng = np.random.default_rng(seed)
    out = []
    L = Launch("d: all 512 contexts")
    for c in range(512):
        cnt = int(rng.integers(0, 391))
        sum_ = int(rng.integers(0, MAX_SUM + 1)) if c % 2 else min(MAX_SUM, 16 * int(rng.integers(0, 8)) * cnt + int(rng.integers(0, 16 * cnt + 1)))
        drv = Driver(rng, _steady_row(rng, cnt, sum_))
        L.tables[c] = row_of(drv.coder)
        for _ in range((c * 37) % 200):
            drv.push(drv.rand_rank())
        _fill(L, c, drv)
    out.append(L)
    L = Launch("d: one hot context (511)")
    drv = _steady_start(rng, L, 511)
    for _ in range(3000):
        drv.push(drv.rand_rank())
    _fill(L, 511, drv)
    out.append(L)
    L = Launch("d: empty contexts between populated ones")
    for c in range(0, 512, 7):
        drv = _steady_start(rng, L, c) if c % 2 else Driver(rng, L.tables[c])
        for _ in range(40 + (c % 90)):
            drv.push(drv.rand_rank())
        _fill(L, c, drv)
    out.append(L)
    return out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d}


def launches_a_to_d():
    out = []
    for f in FAMILIES.values():
        out.extend(f())
    return out


# family e: continuation -- chain A, then chain B on the tables A returned
def family_e(seed=5):
    """-> (first launch, second launch's items as a Launch without tables): run B on the tables A left"""
    rng = np.random.default_rng(seed)
    A = Launch("e: first launch")
    order = census_order(_zipf_counts(rng))
    A.tables[:] = table_row(order)
    B = Launch("e: second launch")
    coders = {}
    for c in range(0, 512, 3):
        drv = Driver(rng, A.tables[c]) if c % 2 else _steady_start(rng, A, c)
        for _ in range(int(rng.integers(1, 300))):
            drv.push(drv.rand_rank())
        _fill(A, c, drv)
        coders[c] = drv.coder
    for c in range(0, 512, 2):
        drv = Driver(rng, row_of(coders[c]) if c in coders else A.tables[c])
        for _ in range(int(rng.integers(1, 300))):
            drv.push(drv.rand_rank())
        _fill(B, c, drv)
    return A, B


# family f: one recorded block -- the oracle's own ranks of a single-block input
def recorded_block(oracle, data):
    """-> (tables, gsym, rstart, expected ranks) of the block: the items sorted by context (stable), the tables in the block's
    census order (fresh counts), the ranks the oracle's encoder wrote"""
    _, tr = oracle.encode(data, 1, trace_cap=len(data) + 16)
    sym = np.fromiter((t.symbol for t in tr), dtype=np.uint32, count=len(tr))
    unl = np.fromiter((t.unlikely for t in tr), dtype=np.uint32, count=len(tr))
    ctx = np.fromiter((t.ctx for t in tr), dtype=np.uint32, count=len(tr))
    rank = np.fromiter((t.rank for t in tr), dtype=np.uint16, count=len(tr))
    order = census_order(np.bincount(sym, minlength=NSYMS))
    perm = np.argsort(ctx, kind="stable")
    gsym = (sym | (unl << 16))[perm].astype(np.uint32)
    rstart = np.searchsorted(ctx[perm], np.arange(513)).astype(np.uint32)
    return np.tile(table_row(order), (512, 1)), gsym, rstart, rank[perm]


def recorded_inputs():
    import corpus

    return {"text": corpus.enwik_like(3_000_000), "random": np.random.default_rng(6).integers(0, 256, 1_000_000, dtype=np.uint8).tobytes()}
