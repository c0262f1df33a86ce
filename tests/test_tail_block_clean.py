"""GPU suite: the clean rounds of the tail's block mode (17 <= K <= 192 bidders; kernels_tail.hpp).  The threads that hold
a published slot enter its object into an LDS table of {round, object} keys in front of the round's second barrier
(clean_insert) and raise a dirty word for a second bid on an object or an unowned object; behind the barrier one LDS read
decides.  A clean round -- every bidder on a different, owned object -- is finished by the threads = slots: every bidder
wins, the slot passes to the owner its bidder evicts, K and the order stay; any other round runs the exact RESOLVE / ASSIGN
/ push_all_left.  The first sweep's next lines are requested when the winners are known and are used by the next round
where the slot then holds the person they belong to.  What this can get wrong is tied to the round's shape and to what
the rounds around it were, so the rounds below are located with the oracle (tests/_tail_block_clean.py;
test_tail_block_clean_nogpu.py asserts on the CPU that the search finds every one of them):

  * a clean round at K = 17, 32, 33 (one sweep / two), 64, 65 (the exact path's two forms), 192 (the threshold), at an odd K
    (the last pair has an inactive half) -- in solves of 200 independent lanes whose block rounds are clean except where a
    lane's price war ends;
  * a clean round directly followed by a dirty one and a dirty one followed by a clean one (the requested lines are dropped
    / used);
  * a contested object with equal bids (the earlier list position keeps it); a round in which one chain ends and K falls by
    one, with the hole in slot 0 and in the last slot;
  * a clean round with two different objects on one hash of the clean table (the smaller key moves to the next slot: the
    round stays clean, the result is the oracle's);
  * a clean round in which a person whose row keeps no line bids (the scan pass; its slot's clean test is the scanner's):
    max, min, the 12 B/edge layout; a handle without lines, where every slot of every round goes through the scan pass;
  * a clean round in which a person with a row of 42 near-equal edges bids from a spent line: the scan pass answers and
    REBUILDS the line (tail_build), the slot's clean test follows the rebuild, and the round behind starts the slot's next
    person from its own line: max, min, the 12 B/edge layout;
  * the 512-thread instance's block rounds (a launch budget of 8 rounds, a handle without lines);
  * the same bodies through solve_batch.

Every checked solve also compares the device's count of rounds finished on the clean path with the oracle's clean rounds.

The device state after each located round -- max_iter stopping there -- is compared with the oracle capped at the same
round: its, K, the list in order, prices bit for bit, p2o / o2p.  A test fails, it does not skip, when an event is not
found."""
import numpy as np
import pytest

import _tail_block_clean as tc
from oracle import oracle as orc
from sslap_amd import AuctionSolver, from_sparse
from test_tail_winning_lane import _check_state

pytestmark = pytest.mark.gpu


def _check_family(family, names=None, behind=(), **kw):
    """Every event the family must show, located by the oracle and checked on the device; for the events named in `behind`
    also the round behind the located one (a requested line is used / dropped there)."""
    names = list(tc.REQUIRED[family] if names is None else names)
    found, missing = tc.locate(family, names)
    print("events:", found)
    assert not missing, ("not found in any seed", missing)
    n, kind, prob, opts = family
    g = None
    for seed in sorted(set(sd for sd, _ in found.values())):
        loc, val, ev, total = tc.trace((n, seed, kind, prob, opts))
        rounds = set(r for sd, r in found.values() if sd == seed)
        rounds |= set(min(r + 1, total) for e, (sd, r) in found.items() if sd == seed and e in behind)
        for r in sorted(rounds):
            g = _check_state(loc, val, prob, r, **dict(tc.kw_of(kind), **kw))
            _check_clean_count(g, ev, r)
    return g


def _check_clean_count(g, ev, r):
    """The device finished on its clean path exactly the block rounds the oracle calls clean (meta tail_stats[10]).  The host
    learns K with a delay, so the first rounds of a phase's block range may have run in the grid kernels: those are allowed
    for, nothing else."""
    blk = g.gpu["tail_modes"]["block"]
    assert blk["rounds"] >= 1, r  # (the located round is a block round of the device too)
    want_block = sum(1 for x in ev["block"] if x <= r)
    want_clean = sum(1 for x in ev.get("clean", []) if x <= r)
    elsewhere = want_block - blk["rounds"]
    assert 0 <= elsewhere <= 2 * (g.meta["nreductions"] + 1), (r, want_block, blk)
    assert want_clean - elsewhere <= blk["clean_rounds"] <= want_clean, (r, want_clean, blk)


def test_clean_rounds_at_the_edges_of_K(gpu_lib):
    """K = 17, 32, 33, 64, 65, 192 and an odd K; each with the round behind it, which starts from the requested lines."""
    g = _check_family(tc.LANES, tc.CLEAN + ["clean odd K"], behind=tc.CLEAN + ["clean odd K"])
    assert g.gpu["bytes_per_edge"] == 8


def test_clean_and_dirty_rounds_in_sequence(gpu_lib):
    _check_family(tc.LANES, tc.SEQUENCES, behind=tc.SEQUENCES)


@pytest.mark.parametrize("family", [tc.LANES, tc.INTS200], ids=["lanes", "ints"])
def test_contested_objects_and_chain_ends(family, gpu_lib):
    """Equal bids on one object (the earlier list position keeps it); one chain ends and K falls by one, the hole in slot 0
    / in the last slot is filled from the right."""
    names = [e for e in tc.REQUIRED[family] if e not in tc.CLEAN + ["clean odd K"] + tc.SEQUENCES]
    _check_family(family, names, behind=names)


def test_two_objects_on_one_hash_of_the_clean_table(gpu_lib):
    """The column numbers come in pairs that share clean_hash: the second insert meets another object's key of this round and
    walks on.  Nothing is contested: the device must not lose a bid, and the result is the oracle's."""
    _check_family(tc.LANES_COLLIDE, behind=tc.REQUIRED[tc.LANES_COLLIDE])


@pytest.mark.parametrize("family", [tc.LANES_LONG, tc.LANES_MIN, tc.LANES_64], ids=["max", "min", "slot64"])
def test_row_scans_inside_clean_rounds(family, gpu_lib):
    """Every eighth lane has a person whose row (303 edges) keeps no line: its bids are answered by the scan pass, inside
    rounds that are otherwise clean and answered by lines."""
    g = _check_family(family, behind=[tc.MISS])
    assert g.gpu["bytes_per_edge"] == (12 if family[1] == "lanes64" else 8)
    assert 0 < g.gpu["cand_hits"] < g.gpu["bids_made"]


@pytest.mark.parametrize("family", [tc.LANES_WIDE, tc.LANES_WIDE_MIN, tc.LANES_WIDE_64], ids=["max", "min", "slot64"])
def test_line_rebuilds_inside_clean_rounds(family, gpu_lib):
    """One lane of 42 persons with 42 near-equal edges each: a person's line (the 24..30 best) is spent by the time the person
    bids again, so its slot goes through the scan pass, which rebuilds the line (tail_build) and does the slot's clean test
    behind the rebuild -- inside clean rounds whose other slots are answered by lines.  Six located rounds spread over the
    solve, each with the round in front (the difference of the two solves' counters is the round's own misses and
    rebuilds) and the round behind it (the slot's next person must start from its own line, not from a requested one)."""
    n, kind, prob, opts = family
    found, missing = tc.locate(family, [tc.REBUILD])
    assert not missing, missing
    loc, val, ev, total = tc.trace((n, found[tc.REBUILD][0], kind, prob, opts))
    located = [r for r in ev[tc.REBUILD] if r - 1 in ev["block"]]
    located = [located[i] for i in np.linspace(len(located) // 4, len(located) - 1, 6).astype(int)]
    own = []
    for r in located:
        c = []
        for q in (r - 1, r, min(r + 1, total)):
            g = _check_state(loc, val, prob, q, **tc.kw_of(kind))
            _check_clean_count(g, ev, q)
            c.append((g.gpu["bids_made"] - g.gpu["cand_hits"], g.gpu["tail_cand"]["builds"]))
        own.append((c[1][0] - c[0][0], c[1][1] - c[0][1]))
    print("misses / rebuilds inside the located clean rounds:", list(zip(located, own)))
    assert g.gpu["bytes_per_edge"] == (12 if kind == "lanes64" else 8)
    assert sum(1 for m, b in own if m >= 1 and b >= 1) >= 3, own  # the scan pass and tail_build ran INSIDE clean rounds


def test_handle_without_lines_in_the_512_thread_instance(gpu_lib, monkeypatch):
    """A launch budget of 8 rounds (read per create): the 1024-thread instance returns after two rounds and the 512-thread
    instance, which holds every mode, runs the rest of the launch's block rounds -- three sweeps in flight, the clean test and
    the clean finish between full barriers."""
    monkeypatch.setenv("MISSLAP_TAIL_LAUNCH_ROUNDS", "8")
    g = _check_family(tc.LANES, tc.NO_LINES, behind=tc.NO_LINES, cand=0, tail_threshold=tc.K_HI)
    assert g.gpu["cand_hits"] == 0 and g.gpu["tail_modes"]["block"]["clean_rounds"] >= 8


def test_handle_without_lines(gpu_lib):
    """cand=0: every slot of every block round goes through the miss queue and the scan pass, clean rounds included.  (Without
    lines the default tail threshold leaves no block rounds: it is set to the one handles with lines use.)"""
    g = _check_family(tc.LANES, tc.NO_LINES, behind=tc.NO_LINES, cand=0, tail_threshold=tc.K_HI)
    assert g.gpu["cand_hits"] == 0 and g.gpu["bids_made"] > 0


def test_clean_rounds_in_a_batch(gpu_lib):
    """solve_batch (one group) runs the k_batched instances of the same bodies; three problems stop inside block rounds."""
    refs, solvers = [], []
    for key, cap in zip(tc.BATCH_KEYS, tc.BATCH_CAPS):
        loc, val, ev, total = tc.trace(key)
        r = 10**8 if cap is None else ev[cap][len(ev[cap]) // 2]
        kw = tc.kw_of(key[2])
        o = orc.from_sparse(loc, val.copy(), problem=key[3], max_iter=r, cardinality_check=False, **kw)
        o.solve()
        refs.append(o.state())
        solvers.append(from_sparse(loc, val.copy(), problem=key[3], max_iter=r, cardinality_check=False, **kw))
    sols, info = AuctionSolver.solve_batch(solvers)
    assert info["groups"] >= 1
    for s, so, sol in zip(solvers, refs, sols):
        sg = s.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"]
        assert np.array_equal(sg["U"], so["U"])
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
        assert np.array_equal(sol, so["p2o"])
