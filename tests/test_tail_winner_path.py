"""GPU suite: the winner path of the tail's line evaluations (cand_eval1_r in the chain and team rounds, its two-line copy
in the pair rounds): the value of a lane without a candidate is -inf by the subtraction itself, the high words' maximum
is taken wave-uniformly from two lanes, and the winner is the ballot's only lane -- or, when a bidder's two best values
differ but share their upper 32 bits, what the exact 64-bit passes say.  The inputs below make such rounds frequent
(values 1000 + j * 2^-14: one high word, fp32-exact); the rounds are located with the oracle, and the device state after
each of them -- max_iter stopping there -- is compared with the oracle capped at the same round: its, K, the list in
order, prices bit for bit, p2o / o2p.  Further: equal values in a line / equal bids / chain ends (three integer values),
lines that miss (no maintenance pass: tau = +inf lines, every slot empty), the 12 B/edge layout, a batched solve."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import AuctionSolver, from_sparse, synth

pytestmark = pytest.mark.gpu

CLASSES = ("K=1", "K=2", "3<=K<=16")


def _class_of(K):
    return "K=1" if K == 1 else "K=2" if K == 2 else "3<=K<=16" if 3 <= K <= 16 else None


def _tie_inputs(n, s, J, f64=False):
    loc, _ = synth.gen_sparse(n, n, 12.0 / n, seed=s)
    j = np.random.default_rng(s).integers(0, J, loc.shape[0])
    val = 1000.0 + j * 2.0 ** -14  # fp32-exact, every value in one 20-bit high word
    if f64:
        val = val * (1.0 + 2.0 ** -30)  # no longer fp32-exact: the 12 B/edge layout (lines of slots + lines of fp64 costs)
    return loc, val


def _int_inputs(n, s):
    return synth.gen_sparse(n, n, 12.0 / n, seed=s, integer_values=3)


@functools.lru_cache(maxsize=None)
def _trace(key):
    """One stepping pass of the oracle: per class the rounds (1-based) that start in it, per class those of them in which
    some bidder's two largest  cost - price  differ but share their upper 32 bits, and the round count of the solve."""
    kind, n, s, J, prob = key
    loc, val = _int_inputs(n, s) if kind == "ints" else _tie_inputs(n, s, J, f64=kind == "tie64")
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False)
    L = orc.lib()
    rows, cols = loc[:, 0], loc[:, 1]
    row_ptr = np.searchsorted(rows, np.arange(o.N + 1))  # rows are sorted
    cost = val if prob == "max" else -val  # the solver works on -val for 'min' (auction_.pyx:236-237)
    rounds = {c: [] for c in CLASSES}
    ties = {c: [] for c in CLASSES}
    r = 0
    while True:
        K = o.raw_meta().num_unassigned
        r += 1
        c = _class_of(K)
        if c is not None:
            price = np.ctypeslib.as_array(L.oracle_prices(o._h), (o.M,))  # live views
            U = np.ctypeslib.as_array(L.oracle_unassigned(o._h), (o.N,))
            rounds[c].append(r)
            tie = False
            for i in U[:K].tolist():
                a, b = row_ptr[i], row_ptr[i + 1]
                if b - a < 2:
                    continue
                v = np.sort(cost[a:b] - price[cols[a:b]])[-2:]
                hi = v.view(np.uint64) >> np.uint64(32)
                if v[0] != v[1] and hi[0] == hi[1]:
                    tie = True
                    break
            if tie:
                ties[c].append(r)
        if o.step():
            break
    return loc, val, rounds, ties, r


def _spread(rounds, k):
    if len(rounds) <= k:
        return list(rounds)
    idx = np.unique(np.linspace(0, len(rounds) - 1, k).round().astype(int))
    return [rounds[i] for i in idx]


def _check_state(loc, val, prob, r, **kw):
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False)
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


@pytest.mark.parametrize("kind,n,s,J,prob", [
    ("tie", 400, 44, 16, "max"),
    ("tie", 400, 46, 8, "max"),
    ("tie", 300, 45, 16, "min"),
    ("tie64", 400, 46, 8, "max"),  # 12 B/edge layout: Slot64
])
def test_high_word_ties_round_by_round(kind, n, s, J, prob, gpu_lib):
    """Rounds in which a bidder's two best values tie on the high word, in the chain, the pair and the team rounds."""
    loc, val, _, ties, total = _trace((kind, n, s, J, prob))
    counts = {c: len(ties[c]) for c in CLASSES}
    print("rounds with a high-word tie:", counts, "of", total)
    for c in CLASSES:
        assert counts[c] >= 5, (c, counts)
    for r in sorted(set(x for c in CLASSES for x in _spread(ties[c], 24)) | {total}):
        g = _check_state(loc, val, prob, r)
        assert g.gpu["bytes_per_edge"] == (12 if kind == "tie64" else 8)


@pytest.mark.parametrize("n,s,prob", [(300, 12, "max"), (300, 13, "min")])
def test_equal_values_round_by_round(n, s, prob, gpu_lib):
    """Three integer values: equal values in a line (the LAST stored slot wins, W counts multiplicity), equal bids on one
    object, chain ends (an unowned object won) -- the K = 1 and the 3 <= K <= 16 rounds (K = 2: test_tail_pair.py)."""
    loc, val, rounds, _, total = _trace(("ints", n, s, 0, prob))
    for c in ("K=1", "3<=K<=16"):
        assert rounds[c], c
    for r in sorted(set(_spread(rounds["K=1"], 24) + _spread(rounds["3<=K<=16"], 24)) | {total}):
        _check_state(loc, val, prob, r)


@functools.lru_cache(maxsize=None)
def _miss_case(seed):
    loc, val = synth.gen_sparse(2000, 2000, 12.0 / 2000, seed=seed)
    o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False)
    osol = o.solve()
    return loc, val, o, osol


@pytest.mark.parametrize("cand", [2, True])
def test_lines_that_miss_whole_solve(cand, gpu_lib):
    """cand=2: no maintenance pass, so lines miss (tau = +inf lines with every slot empty, exhausted lines): whole-solve
    parity."""
    loc, val, o, osol = _miss_case(21)
    g = from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False, cand=cand)
    gsol = g.solve()
    assert np.array_equal(gsol, osol)
    assert g.meta["its"] == o.meta["its"] and g.meta["nreductions"] == o.meta["nreductions"]
    assert np.array_equal(g.state()["p"].view(np.uint64), o.state()["p"].view(np.uint64))
    assert g.gpu["edges_scanned"] == o.extra["edges_scanned"] and g.gpu["obj_f64"] == o.extra["obj_f64"]
    assert g.gpu["tail_modes"]["solo"]["rounds"] > 0 and g.gpu["tail_modes"]["team"]["rounds"] > 0
    assert g.gpu["cand_hits"] > 0


def _team_rounds(loc, val, prob):
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False)
    out, r = [], 0
    while True:
        K = o.raw_meta().num_unassigned
        r += 1
        if 3 <= K <= 16:
            out.append(r)
        if o.step():
            break
    return out


def test_winner_path_in_a_batch(gpu_lib):
    """solve_batch: every problem ends exactly as its own oracle solve, also the one that max_iter stops inside its
    team rounds."""
    probs = [synth.gen_sparse(2000, 2000, 12.0 / 2000, seed=31 + s) for s in range(4)]
    caps = [10**8, None, 10**8, 10**8]
    refs, solvers = [], []
    for (loc, val), cap in zip(probs, caps):
        if cap is None:  # stop inside the team rounds
            rounds = _team_rounds(loc, val, "max")
            assert rounds
            cap = rounds[len(rounds) // 2]
        o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=cap, cardinality_check=False)
        o.solve()
        refs.append(o.state())
        solvers.append(from_sparse(loc, val.copy(), problem="max", max_iter=cap, cardinality_check=False))
    sols, info = AuctionSolver.solve_batch(solvers)
    assert info["groups"] >= 1
    for s, so, sol in zip(solvers, refs, sols):
        sg = s.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"]
        assert np.array_equal(sg["U"], so["U"])
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
        assert np.array_equal(sol, so["p2o"])
