"""Shared by test_tail_block_clean.py (GPU), test_tail_block_clean_nogpu.py and tools/tail_block_clean.py: the clean block
rounds of the tail (17 <= K <= 192 bidders at the default tail threshold; kernels_tail.hpp).

A block round is CLEAN when every bidder bids on a different object and every object bid on has an owner: then every
bidder wins, every list slot passes to the owner its bidder evicts, and the list keeps its length and order.  Both halves
can be read off the oracle's state around one step(), without evaluating a row: after a clean round every bidder of the
round is assigned (nobody lost a contested object) and K is what it was (no bidder won an unowned object)."""
import numpy as np

from oracle import oracle as orc

K_LO, K_HI, K_FAST = 17, 192, 64  # block rounds; up to K_FAST bidders wavefront 0 resolves alone, above it the LDS hash table


def count_clean(loc, val, problem="max"):
    """One stepping pass of the oracle.  Returns {"K<=64": [block rounds, clean, contested, chain end], "K>64": [...],
    "rounds": all rounds of the solve}; a round that is both contested and ends a chain counts as contested.
    (K is followed on the list itself -- it is compact, and -1 behind its end: the oracle's meta call evaluates the
    objective, which a count over the 372 465 rounds of the largest config cannot afford.)"""
    o = orc.from_sparse(loc, val.copy(), problem=problem, max_iter=10**8, cardinality_check=False)
    o.set_assign_by_bidders(True)  # (same result, O(bids) per round instead of O(objects))
    L = orc.lib()
    out = {"K<=64": [0, 0, 0, 0], "K>64": [0, 0, 0, 0]}
    K, r = o.N, 0
    while True:
        b = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))[:K].copy()  # live views, taken anew every round
        r += 1
        done = o.step()
        lost = np.ctypeslib.as_array(L.oracle_person_to_object(o._h), (o.N,))[b] < 0
        ended = bool(lost.all())  # (some bidder always wins: the phase ended and the step has emptied the assignment)
        Kn = o.N if ended else int(np.count_nonzero(np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))[:K] >= 0))
        if K_LO <= K <= K_HI:
            row = out["K<=64" if K <= K_FAST else "K>64"]
            row[0] += 1
            row[3 if ended else 2 if lost.any() else 1 if Kn == K else 3] += 1
        K = Kn
        if done:
            break
    out["rounds"] = r
    return out


# ---- the located rounds of test_tail_block_clean.py -----------------------------------------------------------------------
# The problems are those of tests/_tail_block.py (test_tail_winning_lane._problem, enlarged to have block rounds).  Events are
# 1-based round numbers: the state AFTER that round is what a solve capped there (max_iter = r) leaves.
import functools  # noqa: E402

from test_tail_winning_lane import LINE, _colliding_ids, _problem  # noqa: E402

CLEAN_KS = (17, 32, 33, 64, 65, 192)  # half-wave, sweep, fast-path / hash-path and threshold edges
SEEDS = range(1, 25)

# the input families: (persons, kind, problem, generator options)
LANES = (600, "lanes", "max", ())
LANES_MIN = (600, "lanes_min", "min", (("long_every", 8),))
LANES_64 = (600, "lanes64", "max", (("long_every", 8),))
LANES_LONG = (600, "lanes", "max", (("long_every", 8),))
LANES_COLLIDE = (600, "lanes", "max", (("collide", True),))
LANES_WIDE = (600, "lanes", "max", (("wide", True),))
LANES_WIDE_MIN = (600, "lanes_min", "min", (("wide", True),))
LANES_WIDE_64 = (600, "lanes64", "max", (("wide", True),))
INTS200 = (200, "ints", "max", (("full_rows", 20),))

CLEAN = ["clean K=%d" % k for k in CLEAN_KS]
SEQUENCES = ["clean then dirty", "dirty then clean"]
MISS = "clean, a row without a line bids"
REBUILD = "clean, a row longer than a line bids"  # 30 < row length <= ROW_NEVER_CACHED: a miss rebuilds the line
# what each family must show within SEEDS (the GPU test checks the device at these rounds)
REQUIRED = {
    LANES: CLEAN + ["clean odd K"] + SEQUENCES + ["K falls by one", "hole in the last slot"],
    INTS200: ["contested, equal bids", "K falls by one", "hole in slot 0", "hole in the last slot"],
    LANES_COLLIDE: ["clean, two objects on one hash"],
    LANES_LONG: [MISS],
    LANES_MIN: [MISS],
    LANES_64: [MISS],
    LANES_WIDE: [REBUILD],
    LANES_WIDE_MIN: [REBUILD],
    LANES_WIDE_64: [REBUILD],
}
NO_LINES = ["clean K=33", "clean K=65", "clean odd K"] + SEQUENCES  # LANES with lines switched off: every bid is a row scan
# one solve_batch group (a batch: one number of persons): the uncapped solve and three that stop inside block rounds
BATCH_KEYS = [(600, 1, "lanes", "max", ()), (600, 2, "lanes", "max", ()), (600, 3, "lanes", "max", ()),
              (600, 4, "lanes", "max", (("long_every", 8),))]
BATCH_CAPS = [None, "clean", "clean then dirty", MISS]


LANES_KW = dict(eps_start=2.0 ** -6)


ROW_NEVER_CACHED = 256  # kCandRowMax: a longer row keeps no line, every bid of its person is a row scan (the scan pass)


WIDE = 42  # persons / objects of the wide lane (generator option `wide`): rows longer than a line, far below ROW_NEVER_CACHED


def _lanes(n, seed, per=3, long_every=0, wide=False):
    """n persons / n objects in n / per independent lanes: the persons of a lane value its objects alone, all of them but
    one at 1000 + d (d differs from lane to lane), the last at 1000.  Behind the first rounds of the phase a lane has ONE
    unassigned person, which outbids an owner by eps (LANES_KW: far below d) round after round until the good objects'
    prices have risen by d.  So K = the lanes still at war: every round in which no lane ends its war is clean, and K passes
    through every value from n / per downwards, staying there for many rounds.  Rows of `per` edges: every line holds its
    row whole -- but with `long_every` the first person of every so-many-th lane has 300 more edges, which it never wants:
    its row keeps no line.  `collide`: the objects are numbered in pairs that share their hash in the kernels' tables;
    kind "lanes_min": the same problem as costs to minimise, "lanes64": values that are not fp32-exact.
    `wide`: the last WIDE / per lanes are ONE lane of WIDE persons and objects, all objects but one at 1000.5 (+ noise far
    below eps).  Its single bidder raises the cheapest good object by eps, so the good objects' prices rise in turn; a
    person's line holds the 24..30 best of its 42 near-equal edges, and by the time the person is evicted and bids again
    every one of them has fallen below the line's tau: the line does not decide, the scan pass answers and REBUILDS it."""
    rng = np.random.default_rng(seed)
    nl = n // per
    perm = rng.permutation(nl * per)
    order = rng.permutation(nl)
    loc, val = [], []
    nw = WIDE // per if wide else 0
    for i in range((nl - nw) * per, nl * per if wide else 0):
        row = [(int(perm[(nl - nw) * per + q]), 1000.0 + (0.5 if q < WIDE - 1 else 0.0) + float(rng.integers(0, 16)) * 2.0 ** -14)
               for q in range(WIDE)]
        for j, v in sorted(row):
            loc.append((i, j))
            val.append(v)
    for lane in range(nl - nw):
        d = 0.5 + float(order[lane]) * 2.0 ** -5  # (every lane its own: the wars end one at a time; fp32-exact values)
        for p in range(per):
            row = [(int(perm[lane * per + q]), 1000.0 + (d if q < per - 1 else 0.0) + float(rng.integers(0, 16)) * 2.0 ** -14)
                   for q in range(per)]
            if long_every and lane % long_every == 0 and p == 0:  # + 300 objects of other lanes it never wants
                mine = set(j for j, _ in row)
                row += [(int(j), 1.0 + float(rng.integers(0, 16)) * 2.0 ** -14)
                        for j in rng.permutation(nl * per)[:300 + per] if int(j) not in mine][:300]
            for j, v in sorted(row):
                loc.append((lane * per + p, j))
                val.append(v)
    loc, val = np.array(loc, dtype=np.int32), np.array(val, dtype=np.float64)
    order = np.lexsort((loc[:, 1], loc[:, 0]))  # (rows ascending, columns ascending inside a row)
    return loc[order], val[order]


def problem(n, seed, kind, **opts):
    if kind.startswith("lanes"):
        loc, val = _lanes(n, seed, long_every=opts.get("long_every", 0), wide=opts.get("wide", False))
        if kind == "lanes_min":
            val = 1024.0 - val  # (fp32-exact like the values: multiples of 2^-14 below 1024)
        if opts.get("collide"):
            loc[:, 1] = _colliding_ids(n)[loc[:, 1]]
            order = np.lexsort((loc[:, 1], loc[:, 0]))  # (the rows stay sorted by column)
            loc, val = loc[order], val[order]
        return loc, (val * (1.0 + 2.0 ** -30) if kind == "lanes64" else val)  # (lanes64: not fp32-exact, 12 B/edge layout)
    return _problem(n, seed, kind, **opts)


def kw_of(kind):
    """The solver options a family is solved with (oracle and device alike)."""
    return dict(LANES_KW) if kind.startswith("lanes") else {}


def clean_hash(obj):  # kernels_tail.hpp
    return (((int(obj) * 2654435761) & 0xFFFFFFFF) >> 20) >> 1


@functools.lru_cache(maxsize=None)
def trace(key):
    """One stepping pass of the oracle over a problem: loc, val, the events {name: [rounds]} of its block rounds, the round
    count.  The rows' values are evaluated for all bidders of a round at once on padded rows (as tests/_tail_block.py)."""
    n, seed, kind, prob, opts = key
    loc, val = problem(n, seed, kind, **dict(opts))
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False, **kw_of(kind))
    L = orc.lib()
    rows, cols = loc[:, 0], loc[:, 1]
    row_ptr = np.searchsorted(rows, np.arange(o.N + 2))
    cost = val if prob == "max" else -val
    lens = np.diff(row_ptr)[: o.N]
    width = int(lens.max())
    pos = np.arange(width)[None, :]
    valid = pos < lens[:, None]
    idx = np.minimum(row_ptr[: o.N, None] + pos, len(cols) - 1)
    cpad = np.where(valid, cost[idx], -np.inf)
    jpad = np.where(valid, cols[idx], 0)
    ev, r, before = {}, 0, None  # before: the round in front was a block round, and whether it was clean

    def add(name):
        ev.setdefault(name, []).append(r)

    while True:
        m = o.raw_meta()
        K = m.num_unassigned
        eps = float(np.float32(m.final_eps))
        r += 1
        now = None
        if K_LO <= K <= K_HI:
            price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))  # live views, taken anew every round
            b = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))[:K].astype(np.int64)
            o2p = np.ctypeslib.as_array(L.oracle_object_to_person(o._h), (o.M,))
            if ((b >= 0) & (b < o.N)).all():  # (behind a step that ended a phase the list is rebuilt inside the next step)
                add("block")
                v = cpad[b] - np.where(valid[b], price[jpad[b]], 0.0)
                V = v.max(axis=1)
                g = width - 1 - np.argmax(((v == V[:, None]) & valid[b])[:, ::-1], axis=1)  # the LAST stored index among equal maxima
                rest = v.copy()
                rest[np.arange(K), g] = -np.inf
                obj = jpad[b, g]
                bid = (cpad[b, g] - rest.max(axis=1)) + eps
                ends = o2p[obj] < 0
                uniq, cnt = np.unique(obj, return_counts=True)
                now = len(uniq) == K and not ends.any()
                if now:
                    add("clean")
                    if K in CLEAN_KS:
                        add("clean K=%d" % K)
                    if K % 2:
                        add("clean odd K")
                    if len(set(clean_hash(j) for j in obj)) < K:
                        add("clean, two objects on one hash")
                    if (lens[b] > ROW_NEVER_CACHED).any():
                        add(MISS)
                    if ((lens[b] > LINE) & (lens[b] <= ROW_NEVER_CACHED)).any():
                        add(REBUILD)
                for j in uniq[cnt > 1]:
                    top = np.sort(bid[obj == j])[-2:]
                    if top[0] == top[1]:
                        add("contested, equal bids")
                if len(uniq) == K and ends.sum() == 1:  # one chain ends, nothing else happens: K falls by one
                    add("K falls by one")
                    if ends[0]:
                        add("hole in slot 0")
                    if ends[K - 1]:
                        add("hole in the last slot")
                if before is not None and before != now:
                    add("clean then dirty" if before else "dirty then clean")
        before = now
        if o.step():
            break
        assert r < 2_000_000, "the solve does not end"
    return loc, val, ev, r


def locate(family, names):
    """{event: (seed, round)} for the first seed of SEEDS in which each named event occurs, and the names not found."""
    n, kind, prob, opts = family
    todo, found = list(dict.fromkeys(names)), {}
    for seed in SEEDS:
        if not todo:
            break
        ev = trace((n, seed, kind, prob, opts))[2]
        for e in [e for e in todo if ev.get(e)]:
            found[e] = (seed, ev[e][0])
            todo.remove(e)
    return found, todo
