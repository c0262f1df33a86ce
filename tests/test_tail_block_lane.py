"""GPU suite: the lane-wise form of the tail's block rounds (17 <= K <= 192 bidders; cand_eval2_lane, kernels_tail.hpp).  A
wavefront evaluates the lines of list slots 2m and 2m + 1 in its two 32-lane halves, and the lane that holds a half's
winning candidate forms the bid and the hit test and publishes the slot's result -- key, its column, the owner and the
owner's row start of its gathered record -- to LDS itself.  What this form can get wrong and the scalar one could not is
tied to WHICH lane wins, in WHICH half, to an inactive second half (odd K) and to what reads the published slots, so the
rounds below are located with the oracle (tests/_tail_block.py; test_tail_block_lane_nogpu.py asserts on the CPU that the
search finds every one of them):

  * the shape of the round: K = 17, 32, 33 (one sweep / two sweeps of the 1024-thread kernel), 64, 65 (resolve in wavefront
    0 / LDS hash table), odd K, K > 160 (six sweeps);
  * the winner in the first and in the last candidate slot of a full 30-edge line, in half 0 and in half 1;
  * a tie on the high word of V / W (the winner comes from the exact passes) in half 0, in half 1 and in both halves of one
    wavefront's pair; equal values in a line;
  * behind the publish: a contested object with different and with equal top bids, both bidders of one wavefront's pair on
    one object, a chain end, a clean round;
  * single-edge rows (the bid is +inf), lines that do not decide (the scan pass overwrites the slot), the 12 B/edge layout,
    problem="min", a handle without lines, max_iter ending inside a block round, a batched solve.

The device state after each located round -- max_iter stopping there -- is compared with the oracle capped at the same
round: its, K, the list in order, prices bit for bit, p2o / o2p.  A test fails, it does not skip, when an event is not
found."""
import numpy as np
import pytest

import _tail_block as tb
from oracle import oracle as orc
from sslap_amd import AuctionSolver, from_sparse
from test_tail_winning_lane import _check_state

pytestmark = pytest.mark.gpu


def _check_family(family, names=None, extra=(), **kw):
    """Every event the family must show (tests/_tail_block.py: REQUIRED), located by the oracle and checked on the device."""
    names = list(tb.REQUIRED[family] if names is None else names)
    found, missing = tb.locate(family, names)
    print("events:", found)
    assert not missing, ("not found in any seed", missing)
    n, kind, prob, opts = family
    g = None
    for seed in sorted(set(sd for sd, _ in found.values())):
        loc, val, _, total = tb.trace((n, seed, kind, prob, opts))
        rounds = sorted(set(r for sd, rr in found.values() if sd == seed for r in rr) | set(extra))
        for r in rounds:
            g = _check_state(loc, val, prob, r, **kw)
            assert g.gpu["tail_modes"]["block"]["rounds"] >= 1, r  # (the located round is a block round of the device too)
    return g


@pytest.mark.parametrize("family", [tb.TIE200, tb.INTS200], ids=["tie", "ints"])
def test_block_rounds_located(family, gpu_lib):
    """Shapes, winner positions, high-word ties (tie) / equal values and contested objects (ints), chain ends; every capped
    solve ends inside a block round."""
    g = _check_family(family)
    assert g.gpu["bytes_per_edge"] == 8


@pytest.mark.parametrize("family", [tb.TIE400, tb.INTS400], ids=["tie", "ints"])
def test_many_sweeps(family, gpu_lib):
    """K > 160: six sweeps of the 1024-thread kernel, every wavefront's both halves in use."""
    _check_family(family)


def test_clean_block_rounds(gpu_lib):
    """No object bid on twice and no chain end: every bidder of the round wins with the bid its lane published."""
    n, kind, prob, opts = tb.INTS200
    for seed in tb.CLEAN_SEEDS:
        loc, val, ev, _ = tb.trace((n, seed, kind, prob, opts))
        assert ev.get("clean"), seed
        _check_state(loc, val, prob, ev["clean"][0])


def test_single_edge_rows(gpu_lib):
    """Forty persons (forty-one rows on the device: the generator's last row, which the reference ignores, bids there too):
    the first round of the solve is a block round, and the maintenance pass has built every line before it.  A line with a
    single candidate: W = -inf, the bid +inf is formed and published by the winning lane, and its high word 0x7ff00000 is
    no error for the per-lane bad_hi.  Every bid of round 1 is answered by a line."""
    found, missing = tb.locate(tb.SINGLE40, tb.REQUIRED[tb.SINGLE40])
    assert not missing, missing
    n, kind, prob, opts = tb.SINGLE40
    seed, rounds = found["single edge"]
    assert rounds[0] == 1
    loc, val, ev, total = tb.trace((n, seed, kind, prob, opts))
    singles = [i for i in range(n) if (loc[:, 0] == i).sum() == 1]
    assert len(singles) == 2
    for r in sorted(set(ev["block"]) | {total}):
        g = _check_state(loc, val, prob, r)
        if r == 1:
            assert g.gpu["bids_made"] == g.gpu["cand_hits"] == int(loc[:, 0].max()) + 1
            p = g.state()["p"]
            assert all(np.isposinf(p[loc[loc[:, 0] == i, 1][0]]) for i in singles)


def test_lines_that_do_not_decide(gpu_lib):
    """Rows of 40 edges keep the best 24..30 in their line (tau is finite) and no maintenance pass renews them (cand=2): a
    spent line's slot is queued by its wavefront and answered by the scan pass, which overwrites the slot.  A spread of block
    rounds and the whole solve; built lines did miss."""
    loc, val, ev, total = tb.trace(tb.LONG)
    blk = ev["block"]
    assert len(blk) >= 8
    sel = sorted(set(blk[i] for i in np.linspace(0, len(blk) - 1, 8).astype(int)) | {total})
    for r in sel:
        g = _check_state(loc, val, "max", r, cand=2)
    n = int(loc[:, 0].max())
    misses = g.gpu["bids_made"] - g.gpu["cand_hits"]
    print("bids", g.gpu["bids_made"], "line hits", g.gpu["cand_hits"], "persons", n)
    assert n >= 96 and g.gpu["cand_hits"] > 0 and misses > n  # more row scans than first bids: built lines missed


@pytest.mark.parametrize("family", [tb.TIE200_MIN, tb.TIE200_64], ids=["min", "slot64"])
def test_min_and_slot64(family, gpu_lib):
    """problem="min" and the 12 B/edge layout (a slot's cost comes from the parallel line of fp64 costs)."""
    g = _check_family(family)
    assert g.gpu["bytes_per_edge"] == (12 if family[1] == "tie64" else 8)


def test_handle_without_lines(gpu_lib):
    """cand=0: no line ever hits, every slot of every block round goes through the miss queue and the scan pass.  (Without
    lines the default tail threshold leaves no block rounds: it is set to the one handles with lines use.)"""
    g = _check_family(tb.INTS200, tb.NO_LINES, cand=0, tail_threshold=tb.K_HI)
    assert g.gpu["cand_hits"] == 0 and g.gpu["bids_made"] > 0


def test_block_rounds_in_a_batch(gpu_lib):
    """solve_batch (one group) runs the k_batched instances of the same bodies; three problems stop inside block rounds."""
    refs, solvers = [], []
    for key, cap in zip(tb.BATCH_KEYS, tb.BATCH_CAPS):
        loc, val, ev, total = tb.trace(key)
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
