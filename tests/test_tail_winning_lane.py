"""GPU suite: the lane-wise form of the tail's line evaluations (cand_eval1_lane in the chain and team rounds, its two-line
copy in the pair rounds).  The lane that holds the winning candidate forms the bid and the hit test, and stores (chain,
pair) or publishes (team) the round's result from its own registers; only the owner of the winning object is read out in
front of the request of the next line.  What this form can get wrong and the scalar one could not is tied to WHICH lane
wins and to the rounds that leave the common path, so the cases below are located with the oracle:

  * the winner in the first and in the last candidate slot of a line (lanes 1 and 30; 33 and 62 for the second bidder of a
    pair round) in a chain, a pair and a team round;
  * a tie on the values' high word (the winner comes from the exact passes) in a chain round, in either half and in both
    halves of a pair round, and in a team round; equal values in a line (the last stored slot wins);
  * unclean pair rounds: one object for both bidders with different and with equal bids, one chain end, both chains end,
    K falls 2 -> 1; unclean team rounds: a contested object, a chain end, two objects with one hash (pipe_hash);
  * lines that do not decide: W == tau (the line still answers), V == tau (it does not) and a row scan that picks another
    object than the line's best, located with a restatement of the line builder's threshold search; rows longer than a
    line without the maintenance pass; a line with a single candidate (W = -inf, the bid is +inf);
  * the 12 B/edge layout, problem="min", max_iter ending inside each of the three modes, a batched solve.

Problems of 24..96 persons (12 where a phase has to start in the team rounds), about 12 edges per row and rows of exactly
30 edges (a full line: its slot k holds the row's k-th edge): every round runs inside the tail kernels.  The rounds are
found by an oracle search over the seeds of an input family; a test fails, it does not skip, when the search finds none.
The device state after each located round -- max_iter stopping there -- is compared with the oracle capped at the same
round: its, K, the list in order, prices bit for bit, p2o / o2p."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import AuctionSolver, from_sparse

pytestmark = pytest.mark.gpu

LINE = 30  # kCandMax: candidate slots of a line; a row of at most so many edges is held whole, in stored order
MODES = ("chain", "pair", "team")


def _mode_of(K):
    return "chain" if K == 1 else "pair" if K == 2 else "team" if 3 <= K <= 16 else None


def _pipe_hash(obj):  # kernels_tail.hpp
    return ((int(obj) * 2654435761) & 0xFFFFFFFF) >> 20


def _colliding_ids(m):
    """m object numbers, ascending, made of pairs that share their pipe_hash (two such objects in one team round send it
    through the exact RESOLVE although nothing is contested)."""
    by_hash, ids = {}, []
    for j in range(1 << 15):
        by_hash.setdefault(_pipe_hash(j), []).append(j)
    for group in by_hash.values():
        if len(group) >= 2 and len(ids) < m:
            ids += group[:2]
    assert len(ids) >= m
    return np.array(sorted(ids[:m]), dtype=np.int32)


def _problem(n, seed, kind, full_rows=6, long_rows=0, single=0, collide=False):
    """n persons / n + 1 objects (the reference ignores the last row: its N is the largest row index).  Every row holds
    the person's own object (a perfect matching exists) plus random others: `full_rows` rows of exactly 30 edges,
    `long_rows` of 40 (longer than a line: tau is finite), `single` rows of one edge, the rest 8..14."""
    rng = np.random.default_rng(seed)
    m = n + 1
    own = rng.permutation(m)[: n + 1]
    lens = rng.integers(8, 15, n + 1)
    special = rng.permutation(n)
    lens[special[:full_rows]] = LINE
    lens[special[full_rows:full_rows + long_rows]] = 40
    lens[special[full_rows + long_rows:full_rows + long_rows + single]] = 1
    loc = []
    for i in range(n + 1):
        k = int(min(lens[i], m))
        others = rng.permutation(np.delete(np.arange(m), own[i]))[: k - 1]
        for j in sorted([int(own[i])] + others.tolist()):
            loc.append((i, j))
    loc = np.array(loc, dtype=np.int32)
    if collide:
        loc[:, 1] = _colliding_ids(m)[loc[:, 1]]  # (ascending: the rows stay sorted)
    e = loc.shape[0]
    if kind == "ints":
        val = rng.integers(1, 4, e).astype(np.float64)  # equal values, equal bids, contested objects
    else:
        # fp32-exact; integer steps far above eps keep the price wars long, the 2^-14 steps below them tie on the high word
        val = 1000.0 + rng.integers(0, 8, e) + rng.integers(0, 16, e) * 2.0 ** -14
        if kind == "tie64":
            val = val * (1.0 + 2.0 ** -30)  # no longer fp32-exact: the 12 B/edge layout (Slot64)
    return loc, val


@functools.lru_cache(maxsize=None)
def _trace(key):
    """One stepping pass of the oracle over a problem.  Returns loc, val, the events {name: [rounds]} (1-based: the state
    AFTER that round is what a solve capped there leaves) and the round count.  Every person's line exists before its first
    bid in the tail: the maintenance pass ahead of the tail kernels builds them all (a row of at most 30 edges whole, in
    stored order, tau = -inf), so every bid of these rows is answered by its line."""
    n, seed, kind, prob, opts = key
    loc, val = _problem(n, seed, kind, **dict(opts))
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False)
    L = orc.lib()
    rows, cols = loc[:, 0], loc[:, 1]
    row_ptr = np.searchsorted(rows, np.arange(o.N + 2))
    cost = val if prob == "max" else -val
    has_line = np.ones(o.N + 1, dtype=bool)
    ev = {}
    r = 0

    def add(name):
        ev.setdefault(name, []).append(r)

    while True:
        m = o.raw_meta()
        K = m.num_unassigned
        eps = float(np.float32(m.final_eps))
        price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))  # live views, taken anew every round (the oracle
        U = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))  # replaces its list when a phase ends)
        o2p = np.ctypeslib.as_array(L.oracle_object_to_person(o._h), (o.M,))
        r += 1
        mode = _mode_of(K)
        bidders = U[:K].tolist()
        if any(i < 0 or i >= o.N for i in bidders):  # (behind a step that ended a phase the list is rebuilt only inside
            mode = None                              # the next step: such a round is not classified, and its bidders'
            bidders = []                             # lines are simply not counted on)
        if mode is not None:
            add(mode)
            objs, bids, ends, tie = [], [], [], []
            lined = all(has_line[i] for i in bidders)  # every bid of the round is answered by a line
            for s, i in enumerate(bidders):
                a, b = row_ptr[i], row_ptr[i + 1]
                v = cost[a:b] - price[cols[a:b]]
                V = v.max()
                g = int(np.flatnonzero(v == V)[-1])  # the LAST stored index among equal maxima
                W = np.delete(v, g).max() if b - a > 1 else -np.inf
                objs.append(int(cols[a + g]))
                bids.append((cost[a + g] - W) + eps)
                ends.append(o2p[cols[a + g]] < 0)
                hi = np.array([V, W]).view(np.uint64) >> np.uint64(32)
                tie.append(bool(V != W and hi[0] == hi[1]))
                if has_line[i] and b - a == 1:
                    add(mode + " single edge")
                if lined and b - a <= LINE:
                    if mode != "pair" or s == 0:
                        if g == 0:
                            add(mode + " lane1")
                        if g == LINE - 1:
                            add(mode + " lane30")
                    else:
                        if g == 0:
                            add("pair lane33")
                        if g == LINE - 1:
                            add("pair lane62")
                    if V == W:
                        add(mode + " equal values")
            if lined:
                if mode == "pair":
                    if tie[0] and tie[1]:
                        add("pair tie both")
                    elif tie[0]:
                        add("pair tie half0")
                    elif tie[1]:
                        add("pair tie half1")
                    if objs[0] == objs[1]:
                        add("pair same object, equal bids" if bids[0] == bids[1] else "pair same object, different bids")
                    elif ends[0] and ends[1]:
                        add("pair both chains end")
                    elif ends[0] or ends[1]:
                        add("pair one chain ends")
                elif any(tie):
                    add(mode + " tie")
                if mode == "team":
                    if len(set(objs)) < K:
                        add("team contested")
                    elif any(ends):
                        add("team chain end")
                    elif len(set(_pipe_hash(j) for j in objs)) < K:
                        add("team hash false positive")
        done = o.step()
        if mode == "pair" and not done and o.raw_meta().num_unassigned == 1 and o.raw_meta().nreductions == m.nreductions:
            add("pair K 2->1")
        if done:
            break
        assert r < 400_000, "the solve does not end"
    return loc, val, ev, r


def _first(rounds, k=2):
    return list(rounds[:k])


def _check_state(loc, val, prob, r, **kw):
    okw = {k: v for k, v in kw.items() if k == "eps_start"}  # (the other keywords are the device's own options)
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, **okw)
    o.solve()
    so = o.state()
    g = from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, **kw)
    g.solve()
    sg = g.state()
    assert sg["its"] == so["its"] and sg["K"] == so["K"], r
    assert np.array_equal(sg["U"], so["U"]), r
    assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
    assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
    return g


SEEDS = range(1, 41)


def _check_events(family, names, per_event=2, **kw):
    """Oracle search over the seeds of an input family (persons, kind, problem, generator options) for rounds in which each
    named event occurs; the search must find them all.  Every located round is then checked on the device."""
    n, kind, prob, opts = family
    todo, found = list(names), {}
    for seed in SEEDS:
        if not todo:
            break
        ev = _trace((n, seed, kind, prob, opts))[2]
        for e in [e for e in todo if ev.get(e)]:
            found[e] = (seed, ev[e][:per_event])
            todo.remove(e)
    print("events:", found)
    assert not todo, ("not found in any seed", todo)
    g = None
    for seed in sorted(set(sd for sd, _ in found.values())):
        loc, val, _, total = _trace((n, seed, kind, prob, opts))
        rounds = sorted(set(r for sd, rr in found.values() if sd == seed for r in rr) | {total})
        for r in rounds:
            g = _check_state(loc, val, prob, r, **kw)
    return g


# the input families: (persons, kind, problem, generator options)
TIES = (64, "tie", "max", (("full_rows", 32),))
TIES_MIN = (64, "tie", "min", (("full_rows", 32),))
TIES64 = (64, "tie64", "min", (("full_rows", 32),))
INTS = (96, "ints", "max", (("full_rows", 10), ("collide", True)))
# single inputs: (persons, seed, kind, problem, generator options)
SMALL = (24, 11, "ints", "max", (("full_rows", 0),))
SINGLE = (12, 6, "ints", "max", (("full_rows", 0), ("single", 2)))
LONG = (64, 17, "tie", "max", (("full_rows", 4), ("long_rows", 24)))

POSITIONS = [m + " lane1" for m in MODES] + [m + " lane30" for m in MODES] + ["pair lane33", "pair lane62"]


@pytest.mark.parametrize("key", [TIES, TIES_MIN, TIES64], ids=["max", "min", "slot64"])
def test_winner_lane_positions(key, gpu_lib):
    """The storing / publishing lane is the winning lane: first and last candidate slot, in each mode and in both halves of
    a pair round; max_iter ends inside each of the three modes."""
    g = _check_events(key, list(MODES) + POSITIONS)
    assert g.gpu["bytes_per_edge"] == (12 if key[1] == "tie64" else 8)


@pytest.mark.parametrize("key", [TIES_MIN, TIES64], ids=["f32", "slot64"])
def test_high_word_ties(key, gpu_lib):
    """The winner comes from the exact passes: chain, either half and both halves of a pair round, team."""
    _check_events(key, ["chain tie", "pair tie half0", "pair tie half1", "pair tie both", "team tie"])


def test_equal_values_in_a_line(gpu_lib):
    """Equal maxima in a line: the last stored slot wins and W counts multiplicity (the bid is cost - V + eps)."""
    _check_events(INTS, [m + " equal values" for m in MODES])


def test_unclean_pair_rounds(gpu_lib):
    _check_events(INTS, ["pair same object, different bids", "pair same object, equal bids", "pair one chain ends",
                         "pair both chains end", "pair K 2->1"])


def test_unclean_team_rounds(gpu_lib):
    """Reached through the dirty word that the winning lane writes: a contested object, a chain end, two objects that share
    a hash."""
    _check_events(INTS, ["team contested", "team chain end", "team hash false positive"])


def test_small_problem_every_mode(gpu_lib):
    loc, val, ev, total = _trace(SMALL)
    for m in MODES:
        assert ev.get(m), m
    for r in sorted(set(r for m in MODES for r in _first(ev[m], 4)) | {total}):
        _check_state(loc, val, "max", r)


def test_single_edge_bidder(gpu_lib):
    """A line with a single candidate: W = -inf and the bid is +inf, formed and stored by the winning lane; +inf is a legal
    bid whose high word, 0x7ff00000, the running per-lane bad_hi must not take for an error.  Thirteen persons, so the first
    round of the solve is already a team round, and the maintenance pass has built every line before it: both persons with
    a single edge bid +inf from their lines in round 1 (the device answers all thirteen bids of that round from lines, and
    the prices of their objects are +inf).  In later phases their line holds one candidate at the price +inf: every value is
    -inf, no lane of the ballot is alone, the hit test fails on V > tau and the row scan answers.  Every round is checked."""
    loc, val, ev, total = _trace(SINGLE)
    assert 1 in ev.get("team single edge", []) and all(ev.get(m) for m in MODES), sorted(ev)
    singles = [i for i in range(int(loc[:, 0].max()) + 1) if (loc[:, 0] == i).sum() == 1]
    assert len(singles) == 2
    for r in range(1, total + 1):
        g = _check_state(loc, val, "max", r)
        if r == 1:
            assert g.gpu["bids_made"] == g.gpu["cand_hits"] == int(loc[:, 0].max()) + 1
            p = g.state()["p"]
            assert all(np.isposinf(p[loc[loc[:, 0] == i, 1][0]]) for i in singles)


def test_lines_that_do_not_decide(gpu_lib):
    """Rows of 40 edges keep the best 24..30 in their line (tau is finite) and no maintenance pass renews them (cand=2): a
    spent line is answered by the row scan inside the miss blocks, whose result lane 0 stores / publishes.  Whole solve and
    a spread of rounds in every mode, with many long rows at once; what is asserted here is that built lines did miss
    (the single rounds at the boundary of the hit test: test_lines_that_do_not_decide_located)."""
    loc, val, ev, total = _trace(LONG)
    for m in MODES:
        assert ev.get(m), m
    sel = sorted(set(ev[m][i] for m in MODES for i in np.linspace(0, len(ev[m]) - 1, 6).astype(int)) | {total})
    for r in sel:
        g = _check_state(loc, val, "max", r, cand=2)
    n = int(loc[:, 0].max())
    misses = g.gpu["bids_made"] - g.gpu["cand_hits"]
    print("bids", g.gpu["bids_made"], "line hits", g.gpu["cand_hits"], "persons", n)
    assert g.gpu["cand_hits"] > 0 and misses > n  # more row scans than first bids: built lines missed


def test_winning_lane_in_a_batch(gpu_lib):
    """solve_batch (one group) runs the k_batched instances of the same bodies; one problem stops inside its team rounds,
    one inside its pair rounds."""
    keys = [(64, 1, "tie", "max", TIES[3]), (64, 3, "ints", "max", TIES[3]), (64, 2, "tie", "max", TIES[3]),
            (64, 4, "ints", "max", (("full_rows", 10),))]  # (a batch: one number of persons)
    caps = [None, "team", "pair", None]
    refs, solvers = [], []
    for key, cap in zip(keys, caps):
        loc, val, ev, total = _trace(key)
        r = 10**8 if cap is None else ev[cap][len(ev[cap]) // 2]
        o = orc.from_sparse(loc, val.copy(), problem=key[3], max_iter=r, cardinality_check=False)
        o.solve()
        refs.append(o.state())
        solvers.append(from_sparse(loc, val.copy(), problem=key[3], max_iter=r, cardinality_check=False))
    sols, info = AuctionSolver.solve_batch(solvers)
    assert info["groups"] >= 1
    for s, so, sol in zip(solvers, refs, sols):
        sg = s.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"]
        assert np.array_equal(sg["U"], so["U"])
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
        assert np.array_equal(sol, so["p2o"])


# ---- lines that do not decide, located ---------------------------------------------------------------------------------
# Which edges a line of a row longer than 30 holds, and its tau, come from cand_build's threshold search
# (csrc/device_common.hpp).  The search is restated below, probe by probe in the same double arithmetic, for the one long row
# of a 13-person problem: 13 <= kTeamMax, so every round of the solve is a team, pair or chain round, and the first phase is
# followed from the maintenance pass's build (prices 0, hint 0) through every rebuild a miss causes (the hint is the serving
# wavefront's: the list slot's wavefront in the team kernel, the one wavefront of the pair / chain kernel; each kernel is
# launched once per phase).  The model is checked against the device: the row scans it predicts up to a capped round are
# the bids the device did not answer from a line.
CAND_MIN, CAND_MAX = 24, 30
P_ROW = 0  # the person with the long row


def _cand_build(v, V, W, eps, hint):
    """cand_build for a row longer than a line: (tau, member indices in stored order, hint) or None (the old line stays)."""
    count = lambda t: int((v >= t).sum())
    n = count(W)
    if n > CAND_MAX:
        return None
    t = W
    d_ok, d_bad = 0.0, np.inf
    d = hint if hint > 0.0 else 4.0 * max(V - W, eps)
    k = 0
    while k < 40 and n < CAND_MIN:
        t2 = W - d
        n2 = count(t2)
        if n2 <= CAND_MAX:
            d_ok, t, n = d, t2, n2
            d = 2.0 * d if d_bad == np.inf else 0.5 * (d_ok + d_bad)
        else:
            d_bad = d
            d = 0.5 * (d_ok + d_bad)
        if not (d > d_ok) or not (d < d_bad):
            break
        k += 1
    return t, np.flatnonzero(v >= t), (d_ok if d_ok > 0.0 else hint)


def _decide_problem(seed):
    """13 persons.  Person 0: a few shared objects at high integer costs, a block of objects of its own at one cost, a few of
    its own far below (31..40 edges).  The others: 8..12 edges on a pool of shared objects that is smaller than the number of
    persons wants (a price war), plus an object of their own."""
    rng = np.random.default_rng(seed)
    n = 13
    pool = int(rng.integers(6, 15))
    rows = [dict() for _ in range(n)]
    nobj = pool
    highs = rng.permutation(pool)[: int(rng.integers(2, min(pool, 9)))]
    for j in highs:
        rows[P_ROW][int(j)] = float(rng.integers(6, 13))
    block, block_cost = int(rng.integers(20, 29)), float(rng.integers(1, 7)) + float(rng.integers(0, 4)) * 0.25
    for _ in range(block):
        rows[P_ROW][nobj] = block_cost
        nobj += 1
    for _ in range(max(31 - len(rows[P_ROW]), int(rng.integers(1, 9)))):
        rows[P_ROW][nobj] = 0.5
        nobj += 1
    for i in range(1, n):
        for j in rng.permutation(pool)[: int(rng.integers(min(pool, 8), min(pool, 12) + 1))]:
            rows[i][int(j)] = float(rng.integers(6, 13))
        rows[i][nobj] = float(rng.integers(1, 4))
        nobj += 1
    relabel = rng.permutation(nobj)  # (mixes own and shared objects in the stored order of a row)
    loc = [(i, int(relabel[j])) for i in range(n) for j in rows[i]]
    val = [rows[i][j] for i in range(n) for j in rows[i]]
    order = sorted(range(len(loc)), key=lambda k: loc[k])
    return np.array([loc[k] for k in order], dtype=np.int32), np.array([val[k] for k in order], dtype=np.float64)


DECIDE_KW = dict(eps_start=0.25)


@functools.lru_cache(maxsize=None)
def _decide_trace(seed):
    """Events of person 0's bids in the first phase: {name: [rounds]}, the predicted row scans up to each round, the round
    count of the phase."""
    loc, val = _decide_problem(seed)
    o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False, **DECIDE_KW)
    L = orc.lib()
    cols = loc[:, 1]
    row_ptr = np.searchsorted(loc[:, 0], np.arange(o.N + 1))
    price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))
    a, b = row_ptr[P_ROW], row_ptr[P_ROW + 1]
    assert o.N <= 16 and b - a > CAND_MAX and all(row_ptr[i + 1] - row_ptr[i] <= CAND_MAX for i in range(1, o.N))
    m = o.raw_meta()
    eps = float(np.float32(m.final_eps))
    v0 = val[a:b] - price[cols[a:b]]
    V0 = v0.max()
    W0 = np.delete(v0, int(np.flatnonzero(v0 == V0)[-1])).max()
    line = _cand_build(v0, V0, W0, eps, 0.0)  # the maintenance pass: every line is built before the first bid
    if line is None:
        return None
    tau, members, _ = line
    hint_team, hint_duo = np.zeros(16), 0.0
    ev, scans, r = {}, [0], 0
    while True:
        m = o.raw_meta()
        if m.nreductions != 0:
            break
        K = m.num_unassigned
        price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))  # (live views, taken anew every round)
        bidders = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))[:K].tolist()
        if any(i < 0 or i >= o.N for i in bidders):
            break
        r += 1
        missed = 0
        if P_ROW in bidders:
            v = val[a:b] - price[cols[a:b]]
            V = v.max()
            g = int(np.flatnonzero(v == V)[-1])
            W = np.delete(v, g).max()
            vl = v[members]
            Vl = vl.max()
            gl = int(members[np.flatnonzero(vl == Vl)[-1]])
            Wl = np.delete(vl, int(np.flatnonzero(vl == Vl)[-1])).max() if len(members) > 1 else -np.inf
            mode = _mode_of(K)
            if Vl > tau and Wl >= tau:
                assert gl == g and Wl == W  # (the line's answer is the row's)
                if Wl == tau:
                    ev.setdefault("W == tau", []).append(r)
            else:
                missed = 1
                if Vl == tau:
                    ev.setdefault("V == tau", []).append(r)
                if gl != g:
                    ev.setdefault("scan picks another object", []).append(r)
                ev.setdefault("miss in " + mode, []).append(r)
                s = bidders.index(P_ROW)
                hint = hint_team[s] if mode == "team" else hint_duo
                line = _cand_build(v, V, W, eps, hint)
                if line is not None:
                    tau, members, hint = line
                    if mode == "team":
                        hint_team[s] = hint
                    else:
                        hint_duo = hint
        scans.append(scans[-1] + missed)
        if o.step():
            break
    return loc, val, ev, scans, r


DECIDE_EVENTS = ("W == tau", "V == tau", "scan picks another object")
DECIDE_SEEDS = range(1, 201)


def test_lines_that_do_not_decide_located(gpu_lib):
    """The boundary of the lane-wise hit test (strict on V, not on W) and the scan that overrides lane G's object, owner
    and next line: rounds with W == tau (the line answers), V == tau (it does not) and a scan that picks another object than
    the line's best, found by search over seeds.  The device state after each is compared with the oracle, and the device's
    count of bids that no line answered with the scans the model predicts (every other person's line is its whole row and
    always answers)."""
    found = {}
    for seed in DECIDE_SEEDS:
        if len(found) == len(DECIDE_EVENTS):
            break
        tr = _decide_trace(seed)
        if tr is None:
            continue
        for e in DECIDE_EVENTS:
            if e not in found and tr[2].get(e):
                found[e] = (seed, tr[2][e][:2])
    print("events:", found)
    assert len(found) == len(DECIDE_EVENTS), ("not found in any seed", [e for e in DECIDE_EVENTS if e not in found])
    for seed in sorted(set(sd for sd, _ in found.values())):
        loc, val, ev, scans, total = _decide_trace(seed)
        rounds = sorted(set(r for sd, rr in found.values() if sd == seed for r in rr))
        for r in sorted(set(rounds + [min(x + 1, total) for x in rounds])):  # (+ the round behind: the re-requested line)
            g = _check_state(loc, val, "max", r, **DECIDE_KW)
            misses = g.gpu["bids_made"] - g.gpu["cand_hits"]
            assert misses == scans[r], (seed, r, misses, scans[r])
