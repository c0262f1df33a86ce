"""CPU-only: what test_sharded_modes.py takes for granted (tests/_sharded_modes.py).  The oracle's traces of the inputs
reach every shard-size edge the GPU module names, the expected states and edge counts are those of capped oracle solves,
the expected number of sharded rounds is positive where a case claims sharded rounds, and the caps of each test add up to
a bounded number of exchanged rounds (printed per test: run with -s)."""
import numpy as np
import pytest

import _round_modes as rm
import _sharded_modes as sm

MAX_EXCHANGED_PER_TEST = 3000  # sharded rounds over all caps of one parametrised GPU test (two exchanges each)


def _report(test, exchanged):
    print("%-60s %5d sharded rounds" % (test, exchanged))
    assert 0 < exchanged <= MAX_EXCHANGED_PER_TEST, (test, exchanged)


def test_sharded_rounds_formula():
    tr = dict(Kb=np.array([0, 600, 251, 250, 193, 192, 600, 3]))
    assert sm.sharded_rounds(tr, 7, 0, 0) == 7 and sm.sharded_rounds(tr, 3, 0, 0) == 3
    assert sm.sharded_rounds(tr, 7, 251, 192) == 3 and sm.sharded_rounds(tr, 7, 252, 192) == 2
    assert sm.sharded_rounds(tr, 7, 0, 192) == 5 and sm.sharded_rounds(tr, 7, 1, 0) == 7
    assert sm.sharded_rounds(tr, 7, 0, -1) == 7  # (a negative threshold: no tail)


@pytest.mark.parametrize("name", sm.A_INPUTS)
def test_small_inputs_reach_every_shard_size_edge(name):
    """K = W-1, W and W+1 start a round of each input for W = 2, 3, 5, 8 -- exactly: no substitute is in use."""
    tr = sm.reference(name)[4]
    Kb = tr["Kb"]
    assert tr["finished"] and Kb[1] == Kb[1:].max()
    ends = sm.phase_ends(tr)
    assert len(ends) >= 3
    for world in sm.WORLDS:
        edge = sm.shard_size_caps(tr, world)
        assert sorted(edge) == [world - 1, world, world + 1]
        for b, (k, r) in edge.items():
            assert k == b and Kb[r] == b and not (Kb[1:r] == b).any(), (name, world, b, k, r)
        caps = sm.caps_a(tr, world)
        assert set(range(1, 26)) <= set(caps) and {ends[0], ends[0] + 1, ends[1], ends[1] + 1} <= set(caps)
        assert Kb[ends[0] + 1] == Kb[1] and Kb[ends[1] + 1] == Kb[1]  # (the round after a phase end is a full round again)
        # uneven ranges and empty shards among the caps: K % W != 0, and K < W
        assert any(Kb[r] % world for r in caps) and any(Kb[r] < world for r in caps)
        for cand in ("lines", "nolines"):
            _report("A %s W=%d %s" % (name, world, cand), sum(sm.sharded_rounds(tr, r, 0, 0) for r in caps))
    if name == "ties600":
        first = {k: int(np.nonzero(Kb[1:] == k)[0][0]) + 1 for k in (7, 8, 9)}
        assert first == {7: 11, 8: 148, 9: 139}
        assert all(r <= 25 for w in (2, 3, 5) for _, r in sm.shard_size_caps(tr, w).values())
    if name == "single400":
        assert all(r <= 101 for w in sm.WORLDS for _, r in sm.shard_size_caps(tr, w).values())
        assert sm.A_FULL == (name, 3) and tr["total"] == 1206
        _report("A whole %s W=3" % name, sm.sharded_rounds(tr, tr["total"], 0, 0))


def test_expected_states_and_edges_are_those_of_capped_solves():
    """The 600-row input at W = 5 and the caps of case B: every expected state and edge count against an oracle solve
    capped at that round -- among them rounds that end a phase, where a stepped snapshot would be past the reset."""
    name = "ties600"
    loc, val, prob, kw, tr = sm.reference(name)
    caps = sorted(set(sm.caps_a(tr, 5)) | set(sm.caps_b(tr)) | {tr["total"]})
    assert any(tr["Ka"][r] == 0 and r < tr["total"] for r in caps)
    want = sm.expected(name, caps)
    for r in caps:
        o = rm._new(loc, val, prob, kw, r)
        o.solve()
        assert rm.state_diff(want[r][0], o.state()) is None, (r, rm.state_diff(want[r][0], o.state()))
        assert want[r][0]["its"] == r and want[r][1] == o.extra["edges_scanned"], r
    assert sm.expected(name, caps[:3])[caps[0]][0] is want[caps[0]][0]  # computed once


def test_shard_min_k_boundary_round():
    tr = sm.reference(sm.B_INPUT)[4]
    Kb, Ka, thr = tr["Kb"], tr["Ka"], rm.THR_LINES
    q = sm.boundary_round(tr)
    n = int(Kb[1])
    assert tr["phase"][q] == 1 and thr < Kb[q] < n and Kb[q] == 251
    assert Kb[q - 1] > Kb[q] > Kb[q + 1] > thr  # sharded with either value in front of it, a replicated small round behind
    caps = sm.caps_b(tr)
    assert caps == sorted(caps) and len(set(caps)) == 6
    first_tail, last, nxt = caps[3:]
    assert Kb[first_tail] <= thr < Kb[first_tail - 1] and tr["phase"][first_tail] == 1
    assert Ka[last] == 0 and tr["phase"][last] == 1 and Kb[nxt] == n and tr["phase"][nxt] == 2
    lo = [sm.sharded_rounds(tr, r, int(Kb[q]), thr) for r in caps]
    hi = [sm.sharded_rounds(tr, r, int(Kb[q]) + 1, thr) for r in caps]
    assert lo[0] == hi[0] > 0 and all(a == b + 1 for a, b in zip(lo[1:], hi[1:])), (lo, hi)
    assert lo[1] == lo[0] + 1 and lo[2] == lo[1] == lo[3] == lo[4] and lo[5] == lo[4] + 1  # q sharded, nothing behind it, then K = N
    whole = [sm.sharded_rounds(tr, tr["total"], int(Kb[q]) + d, thr) for d in (0, 1)]
    assert whole[0] > whole[1] > 0
    for d in (0, 1):
        _report("B shard_min_k=%d" % (int(Kb[q]) + d), sum((lo, hi)[d]) + whole[d])


@pytest.mark.parametrize("name,world,part,parts", sm.C_CASES)
def test_round_ladder_caps_stay_cheap(name, world, part, parts):
    tr, sels = rm.reference(name)[4:6]
    caps = sels[rm.THR_LINES]["rounds"]
    assert tr["finished"] and caps[-1] == tr["total"]
    # the parts of an input's rounds are disjoint and leave none out
    mine = [c for c in sm.C_CASES if c[:2] == (name, world)]
    assert sorted(r for c in mine for r in caps[c[2]::c[3]]) == caps and [c[2] for c in mine] == list(range(parts))
    caps = caps[part::parts]
    counts = [sm.sharded_rounds(tr, r, 0, rm.THR_LINES) for r in caps]
    assert all(c > 0 for c in counts)
    assert set(sels[rm.THR_LINES]["paths"]) == set(rm.LADDER)  # every hand-off has sharded rounds in front of it
    _report("C %s W=%d part %d of %d" % (name, world, part + 1, parts), sum(counts))


@pytest.mark.parametrize("name", [n + s for n in sm.D_RECT for s in ("", "_shuffled")])
def test_engine_inputs_are_short_and_reach_tiny_partial_rounds(name):
    tr = sm.reference(name)[4]
    Kb = tr["Kb"]
    assert tr["finished"] and tr["total"] <= sm.D_RECT_MAX_ROUNDS
    n = int(Kb[1])
    partial = Kb[1:][Kb[1:] < n]
    assert len(partial) >= tr["total"] // 2 and (Kb[1:] == n).sum() >= 5  # several phases: the walk direction alternates within each
    for world in sm.D_WORLDS:
        assert (partial < world).any() and (partial % world != 0).any() and (partial > world).any(), (name, world)
    assert partial.min() <= 2 and (partial <= 8).sum() >= 3
    for world in sm.D_WORLDS:
        _report("D %s W=%d" % (name, world), sum(sm.sharded_rounds(tr, r, 1, 0) for r in range(1, tr["total"] + 1)))


def test_capped_inputs_run_past_their_last_cap():
    for name, caps in (("ties5000", sm.D_TIES_CAPS),) + tuple((n, sm.E_CAPS) for n in sm.E_INPUTS):
        tr = sm.reference(name)[4]
        assert tr["total"] > max(caps)  # (no cap is the last round of a limited trace)
        _report("%s caps" % name, sum(sm.sharded_rounds(tr, r, 0, 0) for r in caps))
    Kb = sm.reference("ties5000")[4]["Kb"]
    assert (Kb[2:201] % 3 != 0).any() and Kb[200] >= 3


def test_degenerate_inputs_have_fewer_bidders_than_ranks():
    for loc, val in sm.F_INPUTS:
        for prob in ("max", "min"):
            tr = rm.trace(loc, val, prob, limit=sm.F_MAX_ITER)
            assert 1 <= tr["Kb"][1:].max() < sm.F_WORLD and tr["total"] <= sm.F_MAX_ITER
            assert sm.sharded_rounds(tr, tr["total"], 0, 0) == tr["total"]
    assert rm.trace(*sm.F_INPUTS[1], "max", limit=sm.F_MAX_ITER)["total"] == sm.F_MAX_ITER  # one object: runs to max_iter


def test_counting_group_counts_per_rank_and_fails_fast():
    """The runner's group on host arrays: exact reductions, one count per rank and kind, and a rank that aborts makes the
    others raise instead of wait."""
    import threading
    group = sm.CountingGroup(3, timeout_s=5.0)
    out, errs = {}, []
    left = [threading.Event() for _ in range(3)]  # rank k has left the second all-reduce

    def main(rank):
        try:
            a = group.all_reduce(rank, np.array([rank, 5 - rank], dtype=np.int64), "max")
            b = group.all_reduce(rank, np.array([rank + 7, 2**31 - 1], dtype=np.int32), "min")
            out[rank] = (a.tolist(), b.tolist())
            left[rank].set()
            if rank == 1:
                assert left[0].wait(5.0) and left[2].wait(5.0)
                raise ValueError("rank 1 fails")
            group.all_reduce(rank, np.zeros(1, dtype=np.int32), "min")
        except BaseException as e:  # noqa: BLE001
            errs.append((rank, type(e)))
            group.abort()
    th = [threading.Thread(target=main, args=(k,)) for k in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join(20.0)
    assert not any(t.is_alive() for t in th)
    assert out == {k: ([2, 5], [7, 2**31 - 1]) for k in range(3)}
    assert sorted(errs) == [(0, threading.BrokenBarrierError), (1, ValueError), (2, threading.BrokenBarrierError)]
    assert [c["max"] for c in group.calls] == [1, 1, 1] and [c["min"] for c in group.calls] == [2, 1, 2]
