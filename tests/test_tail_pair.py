"""GPU suite: the two-bidder tail rounds (K = 2, handles with candidate lines), which run on one wavefront with both
lines in the two 32-lane halves.  The rounds are located with the oracle (K before the round == 2) and the device state
after each of them -- max_iter stopping inside the K = 2 rounds -- is compared with the oracle capped at the same round:
prices bit for bit, the list in order, p2o / o2p.  Cases: fp32-exact values, small integer values (equal bids on one
object), rows whose lines miss (no maintenance pass), the 12 B/edge layout, and a batched solve."""
import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import AuctionSolver, from_sparse, synth

pytestmark = pytest.mark.gpu


def _inputs(kind, n, seed):
    if kind == "f64":
        loc, _ = synth.gen_sparse(n, n, 12.0 / n, seed=seed)
        r = np.random.default_rng(seed)
        val = r.random(loc.shape[0]) * 10.0 + r.random(loc.shape[0]) * 1e-9  # full 53-bit mantissas
        return loc, val
    return synth.gen_sparse(n, n, 12.0 / n, seed=seed, integer_values=3 if kind == "ints" else 0)


def _pair_rounds(loc, val, prob):
    """Rounds (1-based) that start with K == 2, and the round count of the whole solve."""
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=10**8, cardinality_check=False)
    out, r, K = [], 0, None
    while True:
        K = o.state()["K"]
        r += 1
        if K == 2:
            out.append(r)
        if o.step():
            break
    return out, r


def _spread(rounds, k):
    if len(rounds) <= k:
        return rounds
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


@pytest.mark.parametrize("cand", [True, 2])
@pytest.mark.parametrize("kind,n,seed,prob", [
    ("f32", 400, 11, "max"),
    ("ints", 300, 12, "max"),   # three integer values: equal bids on one object
    ("ints", 300, 13, "min"),
    ("f64", 400, 14, "min"),    # 12 B/edge layout: lines of slots + lines of fp64 costs
])
def test_pair_rounds_round_by_round(kind, n, seed, prob, cand, gpu_lib):
    loc, val = _inputs(kind, n, seed)
    rounds, total = _pair_rounds(loc, val, prob)
    assert rounds, "no round with K == 2"
    for r in _spread(rounds, 24) + [total]:
        g = _check_state(loc, val, prob, r, cand=cand)
        assert g.gpu["bytes_per_edge"] == (12 if kind == "f64" else 8)


@pytest.mark.parametrize("kind,n,seed", [("f32", 2000, 21), ("ints", 1500, 22), ("f64", 2000, 23)])
def test_pair_rounds_whole_solve(kind, n, seed, gpu_lib):
    """Whole solves whose tails run many K = 2 rounds, lines with and without the maintenance pass (more misses):
    assignment, meta, prices, scanned edges."""
    loc, val = _inputs(kind, n, seed)
    o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False)
    osol = o.solve()
    for cand in (True, 2):
        g = from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False, cand=cand)
        gsol = g.solve()
        assert np.array_equal(gsol, osol), cand
        assert g.meta["its"] == o.meta["its"] and g.meta["nreductions"] == o.meta["nreductions"]
        assert np.array_equal(g.state()["p"].view(np.uint64), o.state()["p"].view(np.uint64))
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"] and g.gpu["obj_f64"] == o.extra["obj_f64"]
        assert g.gpu["tail_modes"]["solo"]["rounds"] > 0
        assert g.gpu["cand_hits"] > 0


def test_pair_rounds_in_a_batch(gpu_lib):
    """solve_batch: problems with K = 2 tail rounds share the one-wavefront launch of their group; each ends exactly
    as its own oracle solve, also when max_iter stops one of them inside its K = 2 rounds."""
    probs = [_inputs(k, 600, 30 + s) for s, k in enumerate(("f32", "ints", "f32", "ints"))]
    caps = [10**8, 10**8, None, 10**8]
    refs, solvers = [], []
    for (loc, val), cap in zip(probs, caps):
        if cap is None:  # stop inside the K = 2 rounds
            rounds, _ = _pair_rounds(loc, val, "max")
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
