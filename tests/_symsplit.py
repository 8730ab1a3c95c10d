"""The ranking kernel's split over two wavefronts: launches aimed at what the split adds, and a numpy restatement of it.

In an unchecked group (count >= 327, quotient q < 32, see tests/_symchains.py) wave 0 tracks the ranks of the group's 64
symbols and excluded symbols and never reads value[]; wave 1 follows a sub-batch of m items behind and replays the two
displaced moves of every item on value[] (value[i] <- value[ni1], value[ni1] <- value[next_i], both read before either is
written), with entries of tracked symbols stale until wave 0 rewrites them at the group's end.  `split_model` does exactly
that with arrays, for m = 4 and m = 8, and falls back to the reference coder where the kernel runs on wave 0 alone (plain
items, checked groups, a failed speculation's rerun).

`launches()` builds the cases; `describe()` says, by tests/_symchains.py's path model, what each context's chain makes the
kernel do, so that a test can insist that a case is what its name says.
"""
import numpy as np

import _symchains as sc
from pyref.orz_py import NSYMS, SymRank

SUBS = (4, 8)


# ------------------------------------------------------------------------------------------------ the split, restated
def _targets(i, q):
    t = (15 * i + 15 - 16 * q) >> 4  # i - i/16 - q, arithmetic shift
    nx = max(t, i >> 1, 0)
    return nx, (i + nx) >> 1


def split_model(row, items, m):
    """one context's chain through the kernel's dispatch -> (ranks, table row out, number of unchecked groups that passed)"""
    value = np.array(row[:NSYMS], dtype=np.int64)
    cnt = int(row[2 * NSYMS]) | (int(row[2 * NSYMS + 1]) << 16)
    sum_ = int(row[2 * NSYMS + 2]) | (int(row[2 * NSYMS + 3]) << 16)
    ranks, passed = [], 0

    def by_reference(chunk):
        nonlocal value, cnt, sum_
        c = SymRank([int(x) for x in value])
        c.cnt, c.sum = cnt, sum_
        for v, u in chunk:
            ranks.append(c.encode(v, u))
        value, cnt, sum_ = np.array(c.value, dtype=np.int64), c.cnt, c.sum

    n, j = len(items), 0
    while j < n:
        if not (cnt >= 192 and n - j >= 32):
            by_reference(items[j:j + 1])
            j += 1
            continue
        while n - j >= 32:
            group = items[j:j + 32]
            q = (sum_ >> 4) // cnt
            done = False
            if cnt >= 327 and q < 32:
                saved = value.copy()
                index = np.empty(NSYMS, dtype=np.int64)
                index[value] = np.arange(NSYMS)
                syms = np.array([s for vu in group for s in vu], dtype=np.int64)
                x = index[syms]  # lane 2k: item k's symbol, lane 2k + 1: its excluded symbol
                snaps = []
                for b in range(32 // m):
                    for k in range(b * m, b * m + m):  # wave 0: ranks only
                        snaps.append(x.copy())
                        i = int(x[2 * k])
                        nx, y = _targets(i, q)
                        m1, m2, m3 = x == i, x == y, x == nx
                        x = np.where(m3, y, x)
                        x = np.where(m2, i, x)
                        x = np.where(m1, nx, x)
                    for k in range(b * m, b * m + m):  # wave 1, behind the barrier: the displaced entries only
                        i = int(snaps[k][2 * k])
                        nx, y = _targets(i, q)
                        from_y, from_nx = value[y], value[nx]
                        value[i] = from_y
                        value[y] = from_nx
                # the check: count and sum after every item from the group's ranks
                ii = [int(snaps[k][2 * k]) for k in range(32)]
                c, s, ok = cnt, sum_, True
                for i in ii:
                    c, s = sc._step(c, s, i)
                    ok &= 16 * q * c <= s < 16 * (q + 1) * c
                if ok:
                    for k in range(32):
                        ri, ru = int(snaps[k][2 * k]), int(snaps[k][2 * k + 1])
                        ranks.append(NSYMS - 1 if ri == ru else ri - (ri > ru))
                    value[x] = syms  # every tracked symbol to where it ended up
                    cnt, sum_ = c, s
                    passed += 1
                    done = True
                else:
                    value = saved
            if not done:
                by_reference(group)
            j += 32
    assert sorted(value.tolist()) == list(range(NSYMS)), "value[] is no permutation any more"
    return np.array(ranks, dtype=np.uint16), sc.table_row(value, cnt, sum_), passed


def model_launch(tables, gsym, rstart, m):
    ranks = np.zeros(len(gsym), dtype=np.uint16)
    out = np.array(tables, dtype=np.uint16, copy=True)
    passed = 0
    for c in range(512):
        a, e = int(rstart[c]), int(rstart[c + 1])
        if a == e:
            continue
        items = [(int(g) & 0xFFFF, int(g) >> 16) for g in gsym[a:e]]
        ranks[a:e], out[c], p = split_model(tables[c], items, m)
        passed += p
    return ranks, out, passed


# ------------------------------------------------------------------------------------------------ the cases
def _steady(rng, launch, ctx, cnt, q, frac=0.5):
    """a context in the steady state: count cnt, quotient q, the sum `frac` of the way through q's interval"""
    sum_ = 16 * q * cnt + int(frac * 16 * cnt)
    drv = sc.Driver(rng, sc._steady_row(rng, cnt, sum_))
    launch.tables[ctx] = sc.row_of(drv.coder)
    return drv


def _hold(drv, n):
    """n items that keep the quotient where it is"""
    for _ in range(n):
        drv.push(drv.aim(drv.quotient()))


def _lengths(rng):
    L = sc.Launch("lengths 32, 33, 63, 64, 65, 32 + m")
    for ctx, n in enumerate([32, 33, 63, 64, 65, 36, 40]):
        drv = _steady(rng, L, ctx, 330 + ctx, 2)
        _hold(drv, n)
        L.items[ctx] = drv.items
    return L


def _scaling(rng):
    L = sc.Launch("the 9/10 scaling on item 0, m - 1, m and 31 of a group")
    for ctx, r in enumerate([0, 3, 4, 7, 8, 31]):
        drv = _steady(rng, L, ctx, 390 - r, 3)
        _hold(drv, 64)
        L.items[ctx] = drv.items
    return L


def _failed(rng):
    L = sc.Launch("a failed speculation in the first and in the last sub-batch, a passing group right behind")
    for ctx, (lane, direction) in enumerate([(1, 1), (30, 1), (2, -1), (29, -1), (0, 1), (31, 1)]):
        # the sum walks along the edge of q's interval (a rank can move it by 388 at most) until item `lane` steps over it
        cnt, q = 335 + ctx, 4
        drv = sc.Driver(rng, sc._steady_row(rng, cnt, 16 * (q + 1) * cnt - 1 if direction > 0 else 16 * q * cnt + 5))
        L.tables[ctx] = sc.row_of(drv.coder)
        for k in range(32):
            lo, hi = drv.interval(q)
            if k < lane:
                drv.push(min(hi, NSYMS - 1) if direction > 0 else lo + 5)
            elif k == lane:
                drv.push(drv.aim(q + direction, fallback_low=direction < 0))
            else:
                drv.push(drv.aim(drv.quotient()))
        _hold(drv, 32)
        L.items[ctx] = drv.items
    return L


def _repeats(rng):
    L = sc.Launch("one symbol in consecutive items; a symbol that is also an excluded symbol of its group")
    for ctx in range(6):
        drv = _steady(rng, L, ctx, 330 + 3 * ctx, 0, frac=0.1)  # q = 0: rank 0 over and over keeps the quotient
        v = drv.coder.value[int(rng.integers(0, 6))]
        w = drv.coder.value[int(rng.integers(6, 12))]
        for k in range(64):
            if ctx % 2 == 0:  # v, v, v, ... with itself, w or a random symbol excluded
                drv.push_sym(v, (v, w, int(rng.integers(NSYMS)))[k % 3])
            else:  # v and w by turns, each the other's excluded symbol
                drv.push_sym(v if k % 2 else w, w if k % 2 else v)
        L.items[ctx] = drv.items
    return L


def _displaced_tracked(rng):
    L = sc.Launch("items whose displaced entries are tracked symbols")
    for ctx in range(6):
        drv = _steady(rng, L, ctx, 332 + ctx, 2)
        for _ in range(2):  # two groups
            k = 0
            while k < 32:
                i = int(rng.integers(20, 57))
                nx, y = _targets(i, drv.quotient())
                at_nx, at_y = drv.coder.value[nx], drv.coder.value[y]
                if k + 3 <= 32:
                    # the symbols this item displaces are the next two items' symbols (and excluded symbols of each other)
                    drv.push(i, at_y)
                    drv.push_sym(at_nx, at_y)
                    drv.push_sym(at_y, at_nx)
                    k += 3
                else:
                    drv.push(i, at_nx)
                    k += 1
        L.items[ctx] = drv.items
    return L


def _end_ranks(rng):
    L = sc.Launch("ranks 0, 1 and 388")
    for ctx in range(4):
        drv = _steady(rng, L, ctx, 340 + ctx, 12)  # 16 q = 192: rank 388 adds 196 to the margin, ranks 0 and 1 take 192 / 191
        for k in range(64):
            drv.push((NSYMS - 1, 0, NSYMS - 1, 1)[k % 4] if ctx % 2 == 0 else (0, NSYMS - 1, 1, NSYMS - 1)[k % 4],
                     drv.coder.value[(0, 1, NSYMS - 1)[k % 3]] if ctx < 2 else None)
        L.items[ctx] = drv.items
    return L


def _hot(rng):
    L = sc.Launch("one hot context beside 511 empty ones")
    drv = _steady(rng, L, 200, 350, 2)
    for k in range(2000):
        drv.push(drv.aim(drv.quotient()) if rng.random() < 0.97 else drv.rand_rank())
    L.items[200] = drv.items
    return L


def _all_forty(rng):
    L = sc.Launch("every context has 40 items")
    for ctx in range(512):
        drv = _steady(rng, L, ctx, 327 + ctx % 64, ctx % 5)
        _hold(drv, 40)
        L.items[ctx] = drv.items
    return L


def launches(seed=11):
    rng = np.random.default_rng(seed)
    return [f(rng) for f in (_lengths, _scaling, _failed, _repeats, _displaced_tracked, _end_ranks, _hot, _all_forty)]


def split_chain(seed=12):
    """-> (launch with the whole chains, {context: item count of the first of two launches}): cut at a group boundary
    (64 | 64), in mid-group (80 | 48), inside the first sub-batch of a group (66 | 62) and one item short of a group (95 | 33)"""
    rng = np.random.default_rng(seed)
    L = sc.Launch("one chain over two launches")
    cuts = {0: 64, 1: 80, 2: 66, 3: 95}
    for ctx in cuts:
        drv = _steady(rng, L, ctx, 340 + ctx, 2)
        _hold(drv, 128)
        L.items[ctx] = drv.items
    return L, cuts


def halves(L, cuts):
    A, B = sc.Launch(L.name + ", first part", L.tables.copy()), sc.Launch(L.name + ", second part")
    for ctx, n in cuts.items():
        A.items[ctx], B.items[ctx] = L.items[ctx][:n], L.items[ctx][n:]
    return A, B


def describe(L, gsym, rstart):
    """{context: path model of its chain}"""
    _, _, raw = sc.reference(L.tables, gsym, rstart)
    return {c: sc.path_model(cnt0, sum0, ii) | {"ranks": ii} for c, (cnt0, sum0, ii) in raw.items()}
