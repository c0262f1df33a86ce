"""GPU suite: the device state against the oracle after the rounds at which a solve changes its code path.

A round is served by one of five paths, chosen by K, the bidders at its start: grid kernels (K > 2048), the fused small
round (thr < K <= 2048), and the tail instances block (16 < K <= thr; LDS hash table above 64), team (3..16) and pair /
chain (K <= 2), thr the handle's tail threshold.  Every eps-phase walks down that ladder and hands the list, the price
records, the candidate lines and the round count from one kernel instance to the next.  tests/_round_modes.py picks, from
the oracle's own K trace, the rounds that start at each boundary K (or at the nearest K on its side), every round that
crosses from one path to another with the round before and the round after, the rounds that end a phase and the first
round of the next, and the rounds that jump over a path; a fresh handle with max_iter = r is solved for each and its
state() compared with the oracle's: its, K, the list in order, prices bit for bit, p2o, o2p, nreductions, fp32 eps.
(test_round_modes_nogpu.py checks that selector and those expected states on the CPU.)"""
import numpy as np
import pytest

import _round_modes as rm
from sslap_amd import AuctionSolver, from_sparse

pytestmark = pytest.mark.gpu

# (input, solver options).  cand: default / 2 = lines without the maintenance pass (more misses) / False = no lines
# (k_tail_nolines takes every tail mode, default threshold 40); tail_threshold 16: the small round hands straight to
# team, 512: k_tail_block and its hash table serve 193..512; tiled_min_k=1, engine=1: the tile engine on the grid
# side of the 2048 hand-off.
VARIANTS = [
    ("f32max", {}), ("f32max", dict(cand=2)), ("f32max", dict(cand=False)), ("f32max", dict(tail_threshold=16)),
    ("f32max", dict(tail_threshold=512)), ("f32max", dict(tiled_min_k=1, engine=1)),
    ("f32min", {}), ("f32min", dict(cand=False)),
    ("ints", {}), ("ints", dict(cand=2)), ("ints", dict(tail_threshold=16)),
    ("f64", {}), ("f64", dict(tail_threshold=512)), ("f64", dict(cand=False)),
    ("planted_a", {}), ("planted_a", dict(cand=False)), ("planted_b", {}), ("planted_b", dict(cand=False)),
]


def _thr(kw):
    return kw.get("tail_threshold", rm.default_thr(kw.get("cand")))


def _id(v):
    name, kw = v
    return name + "".join("-%s%s" % (k.replace("tail_threshold", "thr").replace("tiled_min_k", "tmk"), w) for k, w in kw.items())


def _solver(name, r, **kw):
    loc, val, prob, okw = rm.reference(name)[:4]
    return from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, **okw, **kw)


def _same(g, want, what):
    sg = g.state()
    assert sg["its"] == want["its"] and sg["K"] == want["K"], what
    assert np.array_equal(sg["U"], want["U"]), what
    assert np.array_equal(sg["p"].view(np.uint64), want["p"].view(np.uint64)), what
    assert np.array_equal(sg["p2o"], want["p2o"]) and np.array_equal(sg["o2p"], want["o2p"]), what
    assert sg["nreductions"] == want["nreductions"] and np.float32(sg["eps"]) == np.float32(want["eps"]), what
    assert g.status().error_bits == 0, what


@pytest.mark.parametrize("variant", VARIANTS, ids=_id)
def test_state_after_boundary_rounds(variant, gpu_lib):
    name, kw = variant
    tr, sels, snaps = rm.reference(name)[4:]
    thr = _thr(kw)
    sel = sels[thr]
    if name.startswith("planted"):
        assert any(k.startswith("skip ") for k in sel["kinds"])
    else:
        assert all(n >= 3 for n in sel["paths"].values()), sel["paths"]
    for r in sel["rounds"]:
        K0 = int(tr["Kb"][r])
        kinds = [k for k, v in sel["kinds"].items() if r in v]
        g = _solver(name, r, **kw)
        assert g.tail_threshold == thr
        g.solve()
        _same(g, snaps[r], "%s %s: stop after round r=%d, which starts with K=%d on the %s path and ends with K=%d (%s)"
              % (name, kw, r, K0, rm.path_of(K0, thr), int(tr["Ka"][r]), ", ".join(kinds)))
        assert g.gpu["bytes_per_edge"] == (12 if name == "f64" else 8)
        if "engine" in kw:
            assert g.gpu["tiled_active"] == 1


@pytest.mark.parametrize("n", [2, 3, 16, 17, 64, 65, 192, 193])
def test_first_round_starts_in_each_path(n, gpu_lib):
    """n persons: round 1 starts directly in a path, nothing handed over.  State after round 1, round 2 and at the end."""
    for prob in ("max", "min"):
        name = "start%d%s" % (n, prob)
        loc, val, _, okw, tr = rm.reference(name)[:5]
        for r in sorted({1, 2, tr["total"]}):
            want = rm.capped_state(loc, val, prob, okw, r)
            for kw in ({}, dict(cand=False)):
                g = _solver(name, r, **kw)
                g.solve()
                _same(g, want, "n=%d %s %s: stop after round r=%d of %d; round 1 starts with K=%d on the %s path"
                      % (n, prob, kw, r, tr["total"], n, rm.path_of(n, _thr(kw))))


def _hand_off(tr, sel, thr, a, b):
    """The middle one of the selected rounds that start on path a and end on path b."""
    rounds = [r for r in sel["kinds"]["cross %s->%s" % (a, b)]
              if tr["Ka"][r] > 0 and (rm.path_of(tr["Kb"][r], thr), rm.path_of(tr["Ka"][r], thr)) == (a, b)]
    return rounds[len(rounds) // 2]


def test_lockstep_batch_stops_at_a_hand_off_and_a_phase_end(gpu_lib):
    """solve_batch: four problems in lockstep, one stopped by max_iter exactly at the small -> block hand-off, one at the
    end of a middle phase; each ends as its own oracle solve."""
    names = ["f32max", "ints", "f32min", "f64"]
    refs = {n: rm.reference(n) for n in names}
    r_cross = _hand_off(refs["f32max"][4], refs["f32max"][5][rm.THR_LINES], rm.THR_LINES, "small", "block")
    tr_i, sel_i = refs["ints"][4], refs["ints"][5][rm.THR_LINES]
    ends = [r for r in sel_i["kinds"]["phase end"] if tr_i["Ka"][r] == 0]
    r_end = ends[len(ends) // 2]
    assert 0 < r_end < tr_i["total"]
    caps = [r_cross, r_end, refs["f32min"][4]["total"], refs["f64"][4]["total"]]
    solvers = [_solver(n, cap) for n, cap in zip(names, caps)]
    sols, info = AuctionSolver.solve_batch(solvers)
    assert info["groups"] >= 1
    for n, cap, s, sol in zip(names, caps, solvers, sols):
        want = refs[n][6][cap]
        _same(s, want, "%s in a batch, stopped after round r=%d (starts with K=%d)" % (n, cap, int(refs[n][4]["Kb"][cap])))
        assert np.array_equal(sol, want["p2o"]), n


def test_warm_resolve_stops_at_hand_offs(gpu_lib):
    """resolve(prices, eps_start) on a handle that has run a cold solve, stopped at the crossing rounds of the WARM trace
    (the oracle started from the same prices, as in test_warm_start.py).  reset_state invalidates the lines, so the first
    tail entry after the warm start rebuilds them.  A handle's max_iter is fixed at create and holds for both solves:
    the handle capped at r runs its cold solve for r rounds, then the warm one for r rounds."""
    loc, val, prob, okw, tr, _, snaps = rm.reference("f32max")
    cold = _solver("f32max", 10**8)
    cold.solve()
    assert np.array_equal(cold.prices.view(np.uint64), snaps[tr["total"]]["p"].view(np.uint64))
    p0, eps = snaps[tr["total"]]["p"] * 0.5, 0.5  # below the prices the cold solve's lines were built at
    wkw = dict(okw, eps_start=eps)
    wtr = rm.trace(loc, val, prob, wkw, p0=p0)
    sel = rm.select(wtr, rm.THR_LINES)
    rounds = sorted(set(r for k, v in sel["kinds"].items() if k.startswith("cross ") for r in v))
    assert len(set(k for k in sel["kinds"] if k.startswith("cross "))) == 4, sorted(sel["kinds"])
    wsnaps = rm.snapshots(loc, val, prob, wkw, wtr, rounds, p0=p0)
    for r in rounds:
        g = _solver("f32max", r)
        g.solve()
        g.resolve(prices=p0, eps_start=eps)
        _same(g, wsnaps[r], "warm resolve stopped after round r=%d, which starts with K=%d and ends with K=%d"
              % (r, int(wtr["Kb"][r]), int(wtr["Ka"][r])))
    # ... and the whole warm solve on the handle of the whole cold one
    cold.resolve(prices=p0, eps_start=eps)
    _same(cold, rm.capped_state(loc, val, prob, wkw, wtr["total"], p0=p0), "whole warm solve")


@pytest.mark.parametrize("name", ["f32max", "f32min", "ints", "f64"])
def test_mode_accounting(name, gpu_lib):
    """Whole solves, default options.  The counters as the kernels define them: Ctl::grid_rounds is incremented by the
    launch that closes a round outside the tail kernels (k_compact_* behind the grid kernels, k_round_small,
    k_round_fused), i.e. once per round that starts with K > thr; a tail kernel adds the rounds it ran to
    Ctl::tail_rounds (K <= thr) and, per mode, to dbg[0..2]: solo = rounds that start with K <= 2, team with 3..16, block
    with 17..thr.  A round's mode depends on its starting K alone, so the oracle's K trace gives every count exactly."""
    tr, _, snaps = rm.reference(name)[4:]
    g = _solver(name, 10**8)
    g.solve()
    _same(g, snaps[tr["total"]], "%s whole solve" % name)
    want = rm.mode_rounds(tr, rm.THR_LINES)
    modes = {k: v["rounds"] for k, v in g.gpu["tail_modes"].items()}
    assert modes["solo"] > 0 and modes["team"] > 0 and modes["block"] > 0, modes
    assert g.gpu["grid_rounds"] > 0
    assert g.gpu["grid_rounds"] + g.gpu["tail_rounds"] == g.meta["its"] == tr["total"]
    assert g.gpu["grid_rounds"] == want["grid"] + want["small"], (g.gpu["grid_rounds"], want)
    assert modes == dict(solo=want["pair"], team=want["team"], block=want["block"]), (modes, want)
