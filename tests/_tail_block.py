"""Shared by test_tail_block_lane.py (GPU) and test_tail_block_lane_nogpu.py: the input families of the tail's block rounds
(17 <= K <= 192 bidders at the default tail threshold) and the oracle search that locates the rounds both files name.

The problems are those of test_tail_winning_lane.py's `_problem`, enlarged so that they have block rounds.  A block round
serves list slots 2m and 2m + 1 in the two 32-lane halves of one wavefront (kernels_tail.hpp), so a slot's half is its
parity and "one wavefront's pair" is the slots (2m, 2m + 1).  Events are 1-based round numbers: the state AFTER that round
is what a solve capped there (max_iter = r) leaves."""
import functools

import numpy as np

from oracle import oracle as orc
from test_tail_winning_lane import LINE, _problem

K_LO, K_HI = 17, 192  # block rounds at the default tail threshold
SEEDS = range(1, 9)

# the input families: (persons, kind, problem, generator options)
TIE200 = (200, "tie", "max", (("full_rows", 100),))
TIE200_MIN = (200, "tie", "min", (("full_rows", 100),))
TIE200_64 = (200, "tie64", "min", (("full_rows", 100),))
INTS200 = (200, "ints", "max", (("full_rows", 20),))
TIE400 = (400, "tie", "max", (("full_rows", 100),))
INTS400 = (400, "ints", "max", (("full_rows", 20),))
SINGLE40 = (40, "ints", "max", (("single", 2),))
# rows of 40 edges: longer than a line (test_tail_winning_lane.LONG, enlarged to have block rounds); one input
LONG = (96, 17, "tie", "max", (("full_rows", 4), ("long_rows", 36)))

SHAPES = ["K=17", "K=32", "K=33", "K=64", "K=65", "odd K"]
POSITIONS = ["first slot half0", "first slot half1", "last slot half0", "last slot half1"]
TIES = ["tie half0", "tie half1", "tie both halves"]

# what each family must show within SEEDS (the GPU test checks the device at these rounds)
REQUIRED = {
    TIE200: SHAPES + POSITIONS + TIES + ["chain end"],
    INTS200: ["K=17", "K=33", "K=64", "odd K"] + POSITIONS + ["equal values", "contested, different bids", "contested, equal bids",
                                   "one pair, one object", "chain end"],
    TIE400: ["K>160", "tie both halves"],
    INTS400: ["K>160", "contested, equal bids"],
    SINGLE40: ["single edge"],
    TIE200_MIN: POSITIONS + TIES,
    TIE200_64: POSITIONS + TIES,
}
# one solve_batch group (a batch: one number of persons): the uncapped solve and three that stop inside block rounds
BATCH_KEYS = [(200, 1, "tie", "max", TIE200[3]), (200, 2, "tie", "max", TIE200[3]), (200, 3, "ints", "max", TIE200[3]),
              (200, 4, "ints", "max", TIE200[3])]
BATCH_CAPS = [None, "block", "odd K", "contested, equal bids"]
NO_LINES = ["K=33", "K=64", "odd K", "contested, equal bids", "chain end"]  # INTS200 with lines switched off
CLEAN_SEEDS = (3, 4, 6, 7)  # INTS200: a clean block round (no object bid on twice, no chain ends) in each of them


@functools.lru_cache(maxsize=None)
def trace(key):
    """One stepping pass of the oracle over a problem.  Returns loc, val, the events {name: [rounds]} of its block rounds
    and the round count.  The rows' values are evaluated for all bidders of a round at once on padded rows."""
    n, seed, kind, prob, opts = key
    loc, val = _problem(n, seed, kind, **dict(opts))
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False)
    L = orc.lib()
    rows, cols = loc[:, 0], loc[:, 1]
    row_ptr = np.searchsorted(rows, np.arange(o.N + 2))
    cost = val if prob == "max" else -val
    lens = np.diff(row_ptr)[: o.N]
    width = int(lens.max())
    pos = np.arange(width)[None, :]
    valid = pos < lens[:, None]
    idx = np.minimum(row_ptr[: o.N, None] + pos, len(cols) - 1)
    cpad = np.where(valid, cost[idx], -np.inf)  # a row's edges in stored order, -inf behind its end
    jpad = np.where(valid, cols[idx], 0)
    ev = {}
    r = 0

    def add(name):
        ev.setdefault(name, []).append(r)

    while True:
        m = o.raw_meta()
        K = m.num_unassigned
        eps = float(np.float32(m.final_eps))
        r += 1
        if K_LO <= K <= K_HI:
            price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))  # live views, taken anew every round
            U = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))
            o2p = np.ctypeslib.as_array(L.oracle_object_to_person(o._h), (o.M,))
            b = U[:K].astype(np.int64)
            if ((b >= 0) & (b < o.N)).all():  # (behind a step that ended a phase the list is rebuilt inside the next step)
                add("block")
                for name, yes in (("K=%d" % K, K in (17, 32, 33, 64, 65)), ("odd K", K % 2 == 1), ("K>160", K > 160)):
                    if yes:
                        add(name)
                v = cpad[b] - np.where(valid[b], price[jpad[b]], 0.0)
                V = v.max(axis=1)
                isV = (v == V[:, None]) & valid[b]
                g = width - 1 - np.argmax(isV[:, ::-1], axis=1)  # the LAST stored index among equal maxima
                rest = v.copy()
                rest[np.arange(K), g] = -np.inf
                W = rest.max(axis=1)  # second best, counting multiplicity (-inf: a single edge)
                obj = jpad[b, g]
                bid = (cpad[b, g] - W) + eps
                ends = o2p[obj] < 0
                hi = np.stack([V, W]).view(np.uint64) >> np.uint64(32)
                tie = (V != W) & (hi[0] == hi[1])
                half = np.arange(K) & 1
                full = lens[b] == LINE
                lined = (lens[b] <= LINE).all()  # every row fits its line: the maintenance pass built it whole
                if lined:
                    for h in (0, 1):
                        if (full & (half == h) & (g == 0)).any():
                            add("first slot half%d" % h)
                        if (full & (half == h) & (g == LINE - 1)).any():
                            add("last slot half%d" % h)
                        if (tie & (half == h)).any():
                            add("tie half%d" % h)
                    pairs = K // 2
                    if (tie[0:2 * pairs:2] & tie[1:2 * pairs:2]).any():
                        add("tie both halves")
                    if ((V == W) & (lens[b] > 1)).any():
                        add("equal values")
                    if (lens[b] == 1).any():
                        add("single edge")
                    if (obj[0:2 * pairs:2] == obj[1:2 * pairs:2]).any():
                        add("one pair, one object")
                    uniq, cnt = np.unique(obj, return_counts=True)
                    for j in uniq[cnt > 1]:
                        top = np.sort(bid[obj == j])[-2:]
                        add("contested, equal bids" if top[0] == top[1] else "contested, different bids")
                    if ends.any():
                        add("chain end")
                    if len(uniq) == K and not ends.any():
                        add("clean")
        if o.step():
            break
        assert r < 2_000_000, "the solve does not end"
    return loc, val, ev, r


def locate(family, names, per_event=1):
    """{event: (seed, rounds)} for the first seed of SEEDS in which each named event occurs, and the names not found."""
    n, kind, prob, opts = family
    todo, found = list(dict.fromkeys(names)), {}
    for seed in SEEDS:
        if not todo:
            break
        ev = trace((n, seed, kind, prob, opts))[2]
        for e in [e for e in todo if ev.get(e)]:
            found[e] = (seed, ev[e][:per_event])
            todo.remove(e)
    return found, todo
