"""CPU-only: the round selector and the expected states of test_round_modes.py (tests/_round_modes.py).  The GPU tests
compare the device with snapshots of ONE stepping pass of the oracle; here every such snapshot is compared with what a
solve capped at that round (max_iter = r) leaves -- the thing the GPU solve is -- and the selector is shown to reach
every boundary member, every adjacent crossing and every path."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _round_modes as rm

SMALLEST = "f32max"  # gen_sparse(2600, 2600, 12 / 2600, seed=41), max: the fewest rounds of the inputs that start above 2048


def test_path_of_and_ladder():
    assert [rm.path_of(K, 192) for K in (0, 1, 2, 3, 16, 17, 64, 65, 192, 193, 2048, 2049)] == \
        [None, "pair", "pair", "team", "team", "block", "block", "block", "block", "small", "small", "grid"]
    assert [rm.path_of(K, 16) for K in (2, 3, 16, 17)] == ["pair", "team", "team", "small"]
    assert [rm.path_of(K, 512) for K in (512, 513)] == ["block", "small"]
    assert rm.ladder(192, 2600) == list(rm.LADDER)
    assert rm.ladder(16, 2600) == ["grid", "small", "team", "pair"]
    assert rm.ladder(192, 65) == ["block", "team", "pair"] and rm.ladder(192, 2) == ["pair"]
    assert rm.boundaries(16) == [1, 2, 3, 16, 17, 64, 65, 2048, 2049]
    assert len(rm.boundaries(192)) == 11


def test_selector_reaches_every_boundary_crossing_and_path():
    _, _, _, _, tr, sels, _ = rm.reference(SMALLEST)
    Kb, Ka = tr["Kb"], tr["Ka"]
    for thr, sel in sels.items():
        lad = sel["ladder"]
        for b in rm.boundaries(thr):
            rounds = sel["kinds"].get("K=%d" % b)
            assert rounds, (thr, b)
            want = sel["nearest"].get(b, b)
            assert all(Kb[r] == want for r in rounds), (thr, b)
            if b in sel["nearest"]:  # nothing starts at b itself; the nearest K on b's side of its boundary
                assert not (Kb[1:] == b).any()
                assert want < b if rm._is_lower(b, thr) else want > b, (thr, b, want)
                between = (Kb[1:] > min(b, want)) & (Kb[1:] < max(b, want))
                assert not between.any(), (thr, b, want)
        for a, b in zip(lad, lad[1:]):
            rounds = sel["kinds"].get("cross %s->%s" % (a, b))
            assert rounds, (thr, a, b)
            hand_offs = [r for r in rounds if rm.path_of(Kb[r], thr) == a and rm.path_of(Ka[r], thr) == b]
            assert hand_offs, (thr, a, b)
            for r in hand_offs:  # a stop one round either side of the hand-off
                assert r - 1 in rounds or r == 1, (thr, r)
                assert r + 1 in rounds, (thr, r)
        assert all(n >= 3 for n in sel["paths"].values()) and list(sel["paths"]) == lad, (thr, sel["paths"])
        ends = [r for r in sel["kinds"]["phase end"] if Ka[r] == 0]
        assert len(ends) == 3 and tr["total"] in ends
        assert all(r + 1 in sel["kinds"]["phase end"] for r in ends if r < tr["total"])
    assert 192 in sels and rm.boundaries(192) == [1, 2, 3, 16, 17, 64, 65, 192, 193, 2048, 2049]


def test_snapshots_equal_capped_solves():
    """Every expected state of the smallest input, at every threshold it is checked with, against a solve capped at
    that round: K, U, price bits, p2o, o2p, its, nreductions, fp32 eps."""
    loc, val, prob, kw, tr, sels, snaps = rm.reference(SMALLEST)
    rounds = sorted(snaps)
    assert rounds == sorted(set(r for s in sels.values() for r in s["rounds"]))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        capped = list(ex.map(lambda r: rm.capped_state(loc, val, prob, kw, r), rounds))
    for r, want in zip(rounds, capped):
        assert set(rm.STATE_FIELDS) <= set(want)
        assert want["its"] == r
        assert rm.state_diff(snaps[r], want) is None, (r, int(tr["Kb"][r]), rm.state_diff(snaps[r], want))
    # a stepped snapshot of a round that ends a phase is NOT that state (the step has reduced eps and reset the list):
    # such rounds must come from the capped path
    r = next(r for r in rounds if tr["Ka"][r] == 0 and r < tr["total"])
    o = rm._new(loc, val, prob, kw, 10**8)
    for _ in range(r):
        o.step()
    assert rm.state_diff(o.state(), snaps[r]) is not None


@pytest.mark.parametrize("name", sorted(rm.PLANTED))
def test_planted_inputs_skip_paths_and_stay_short(name):
    """The mode-skipping inputs: the oracle finishes within the round bound, a round jumps two or more paths, and a phase
    ends from the team or the block path."""
    _, _, _, _, tr, sels, snaps = rm.reference(name)
    assert tr["finished"] and tr["total"] <= rm.PLANTED_MAX_ROUNDS
    sel = sels[rm.THR_LINES]
    assert any(k.startswith("skip ") for k in sel["kinds"]), sorted(sel["kinds"])
    assert any(k in sel["kinds"] for k in ("end from team", "end from block")), sorted(sel["kinds"])
    Kb, Ka = tr["Kb"], tr["Ka"]
    lad = sel["ladder"]
    jumps = [r for r in range(1, tr["total"] + 1) if Ka[r] > 0 and
             lad.index(rm.path_of(Ka[r], rm.THR_LINES)) - lad.index(rm.path_of(Kb[r], rm.THR_LINES)) >= 2]
    assert jumps and all(r in snaps for r in rm.spread(jumps, 3))


def test_small_starts_begin_in_every_path():
    got = set()
    for n in (2, 3, 16, 17, 64, 65, 192, 193):
        for prob in ("max", "min"):
            _, _, _, _, tr, _, _ = rm.reference("start%d%s" % (n, prob))
            assert tr["Kb"][1] == n and tr["finished"]
            got.add(rm.path_of(n, rm.THR_LINES))
    assert got == {"pair", "team", "block", "small"}
