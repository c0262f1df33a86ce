"""GPU suite: the sharded solve (misslap_solve_sharded, shard=(rank, world)) against the oracle round by round, at the
edges of the shard ranges.

W rank threads share the GPU (tests/_sharded_modes.py: run_ranks); every rank's handle is capped at r rounds and must end
in the oracle's state after r rounds -- its, K, the list in order, prices bit for bit, p2o, o2p, nreductions, fp32 eps --
with no error bit, all ranks alike, `sharded_rounds` and the number of MAX and of MIN exchanges equal to the number of
rounds of the oracle's K trace with K >= shard_min_K and K > tail threshold, and the edges the ranks scanned in sharded
rounds plus the edges of the replicated rounds (the same on every rank) adding up to the oracle's edges_scanned.

  A  the wave-per-row kernels (k_bid, k_tiebreak, k_apply), every round sharded, W = 2, 3, 5, 8: the first 25 rounds, the
     ends of the first two phases, and the rounds that start with K = W-1 (a rank with an empty shard), W (one bidder
     each) and W+1 (the first uneven split); integer values tie across ranks, one-entry rows send +inf keys through the
     MAX exchange, fp64 values take the 12 B/edge layout
  B  shard_min_K set to the K of one round of the second phase and to that K + 1: the round is the last sharded one /
     the first replicated one of its phase; behind it replicated small rounds and the tail, on line tables that differ by
     rank, then a sharded full scan again
  C  the round ladder of test_round_modes.py (threshold 192) with every round above the threshold sharded
  D  the tile engine sharded in every round (person-ordered shards, order_pos in the tie-break, the alternating walk
     direction), in its four record formats
  E  the fp32 filter in sharded rounds
  F  N = 1, three persons for one object, one wide row at W = 8: K < W from the first round on

test_sharded_modes_nogpu.py checks on the CPU that the inputs reach every edge named here.  RCCL is not covered: it needs
one GPU per rank."""
import pytest

import _round_modes as rm
import _sharded_modes as sm

pytestmark = pytest.mark.gpu


def _run(name, world, caps, what, lines_from=None, check=None, **opts):
    """One sharded solve per cap; lines_from: caps at or above it must have answered bids from candidate lines on every
    rank.  Returns the sharded rounds over all caps."""
    loc, val, prob, okw, tr = sm.reference(name)
    want = sm.expected(name, caps)
    total = 0
    for r in caps:
        res = sm.run_ranks(loc, val, prob, world, r, okw, **opts)
        where = "%s %s W=%d: stop after round r=%d, which starts with K=%d and ends with K=%d" % (
            what, opts, world, r, int(tr["Kb"][r]), int(tr["Ka"][r]))
        total += sm.check_ranks(res, want[r][0], want[r][1], tr, r, where, lines=lines_from is not None and r >= lines_from)
        if check:
            check(res, where)
    return total


@pytest.mark.parametrize("cand", [None, False], ids=["lines", "nolines"])
@pytest.mark.parametrize("world", sm.WORLDS)
@pytest.mark.parametrize("name", sm.A_INPUTS)
def test_every_round_sharded_at_the_shard_size_edges(name, world, cand, gpu_lib):
    tr = sm.reference(name)[4]
    opts = dict(sm.A_OPTS) if cand is None else dict(sm.A_OPTS, cand=cand)

    def layout(res, where):
        assert all(x["shard_min_K"] == 0 and x["tail_threshold"] == 0 for x in res), where
        assert all(x["gpu"]["bytes_per_edge"] == (12 if name == "f64_700" else 8) for x in res), where
    caps = sm.caps_a(tr, world)
    assert _run(name, world, caps, "A " + name, check=layout, **opts) == sum(caps)  # (every round of every cap exchanged)


def test_whole_solve_with_every_round_sharded(gpu_lib):
    name, world = sm.A_FULL
    tr = sm.reference(name)[4]
    assert _run(name, world, [tr["total"]], "A whole " + name, lines_from=1, **sm.A_OPTS) == tr["total"]


@pytest.mark.parametrize("above", [0, 1], ids=["last_sharded", "first_replicated"])
def test_shard_min_k_boundary_and_the_regimes_behind_it(above, gpu_lib):
    tr = sm.reference(sm.B_INPUT)[4]
    q = sm.boundary_round(tr)
    smk = int(tr["Kb"][q]) + above

    def routed(res, where):
        assert all(x["shard_min_K"] == smk and x["tail_threshold"] == rm.THR_LINES for x in res), where
    caps = sm.caps_b(tr)
    _run(sm.B_INPUT, sm.B_WORLD, caps, "B", check=routed, shard_min_k=smk)
    # ... and the whole solve: every phase opens with sharded rounds and ends in the tail
    assert _run(sm.B_INPUT, sm.B_WORLD, [tr["total"]], "B whole", lines_from=1, check=routed, shard_min_k=smk) > 0


@pytest.mark.parametrize("name,world,part,parts", sm.C_CASES, ids=["%s-W%d-%dof%d" % (c[0], c[1], c[2] + 1, c[3]) for c in sm.C_CASES])
def test_round_ladder_behind_sharded_rounds(name, world, part, parts, gpu_lib):
    tr, sels = rm.reference(name)[4:6]
    caps = sels[rm.THR_LINES]["rounds"]
    assert caps[-1] == tr["total"]
    caps = caps[part::parts]  # (the whole solve is in one of the parts: only there are line hits claimed)

    def routed(res, where):
        assert all(x["shard_min_K"] == 0 and x["tail_threshold"] == rm.THR_LINES for x in res), where
        assert all(x["gpu"]["bytes_per_edge"] == (12 if name == "f64" else 8) for x in res), where
    assert _run(name, world, caps, "C " + name, lines_from=tr["total"], check=routed, shard_min_k=-1) > 0


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("world", sm.D_WORLDS)
@pytest.mark.parametrize("name", sm.D_RECT)
def test_tile_engine_sharded_every_round(name, world, fmt, gpu_lib):
    name = name + "_shuffled" if fmt >= 2 else name
    tr = sm.reference(name)[4]

    def engine(res, where):
        assert all(x["gpu"]["tiled_active"] == 1 and x["gpu"]["tiled_format"] == fmt for x in res), where
        assert all(x["shard_min_K"] == 1 and x["tail_threshold"] == 0 for x in res), where
    caps = list(range(1, tr["total"] + 1))
    assert _run(name, world, caps, "D " + name, check=engine, force_f64=bool(fmt & 1), **sm.D_OPTS) == sum(caps)


@pytest.mark.parametrize("fmt", [0, 1])
def test_tile_engine_sharded_with_heavy_ties(fmt, gpu_lib):
    def engine(res, where):
        assert all(x["gpu"]["tiled_active"] == 1 and x["gpu"]["tiled_format"] == fmt for x in res), where
        assert all(x["shard_min_K"] == 1 for x in res), where
    caps = list(sm.D_TIES_CAPS)
    assert _run("ties5000", 3, caps, "D ties5000", check=engine, force_f64=bool(fmt & 1), **sm.D_OPTS) == sum(caps)


@pytest.mark.parametrize("cand", [True, False], ids=["lines", "nolines"])
@pytest.mark.parametrize("name", sm.E_INPUTS)
def test_f32_filter_in_sharded_rounds(name, cand, gpu_lib, monkeypatch):
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")  # (read at create)

    def gather(res, where):
        assert all(x["gpu"]["tiled_active"] == 0 and x["gpu"]["filter_undecided"] >= 0 for x in res), where
    caps = list(sm.E_CAPS)
    assert _run(name, 3, caps, "E " + name, check=gather, cand=cand, **sm.E_OPTS) == sum(caps)


def test_degenerate_shapes_on_more_ranks_than_bidders(gpu_lib):
    for loc, val in sm.F_INPUTS:
        for prob in ("max", "min"):
            tr = rm.trace(loc, val, prob, limit=sm.F_MAX_ITER)
            r = tr["total"]  # (rounds run: the one-object input runs to max_iter like the reference)
            o = rm._new(loc, val, prob, {}, sm.F_MAX_ITER)
            o.solve()
            res = sm.run_ranks(loc, val, prob, sm.F_WORLD, sm.F_MAX_ITER, **sm.A_OPTS)
            n = sm.check_ranks(res, o.state(), o.extra["edges_scanned"], tr, r, "F %s %s" % (loc.tolist(), prob))
            assert n == r and int(tr["Kb"][1:].max()) < sm.F_WORLD
