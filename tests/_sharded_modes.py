"""Shared by test_sharded_modes.py (GPU) and test_sharded_modes_nogpu.py: the sharded solve (misslap_solve_sharded) round
by round against the oracle, at the edges of the shard ranges.

The bidders of a sharded round are split over W ranks by list position, [K*r/W, K*(r+1)/W); the ranks exchange a per-object
arg-max (all-reduce MAX over the bid keys, all-reduce MIN over the list positions of the bidders that hold the maximum) and
then apply the round redundantly.  A round is sharded when K >= shard_min_K and K > tail threshold (host_comm.hpp); every
other round is replicated.  Here the W ranks are THREADS of one process that share the GPU (sslap_amd.dist.ThreadGroup,
Comm.in_process: the library's own loop and exchange calls, the buffers staged through the host and reduced with numpy);
each rank's handle is capped at r rounds (max_iter = r) and its state() compared with the oracle's after r rounds, as
tests/_round_modes.py does for the single-GPU paths.  The expected states, the oracle's K trace and the round selection
come from _round_modes; this module adds the inputs, the caps that sit at the shard-size edges (K = W-1, W, W+1: empty
shards, one bidder each, the first uneven split), the expected number of sharded rounds and of scanned edges per cap, and
the rank-thread runner.

RCCL itself cannot be covered on one GPU (it needs a device per rank): what is pinned is everything on the library's side of
the two all-reduce calls.  The all-reduces here are exact by construction (numpy maximum / minimum over the W buffers)."""
import functools
import threading

import numpy as np

import cases
import _round_modes as rm
from sslap_amd.dist import ThreadGroup

WORLDS = (2, 3, 5, 8)
TIMEOUT_S = 60.0

# name -> (cases.synth_inputs spec, problem, rounds of the oracle trace to take: None = the whole solve)
INPUTS = {
    # A: small square inputs whose every round is sharded (tail_threshold=0, shard_min_k=-1)
    "ties600": (dict(kind="sparse", n=600, m=600, density=0.03, ints=3), "max", None),   # integer values: ties across ranks
    "single400": (dict(kind="single", n=400, density=0.04, n_single=12), "min", None),   # one-entry rows: +inf bid keys
    "f64_700": (dict(kind="f64", n=700, density=0.02), "max", None),                      # 12 B/edge layout
    # D: the tile engine (test_tiled_bid_kernel_round_by_round's inputs); rows in stored order / shuffled within rows
    "rect6000": (dict(kind="sparse", n=6000, m=40000, density=0.001), "max", None),
    "rect6000_shuffled": (dict(kind="shuffled", n=6000, m=40000, density=0.001), "max", None),
    "rect4500": (dict(kind="sparse", n=4500, m=33000, density=0.0012, ints=3), "min", None),
    "rect4500_shuffled": (dict(kind="shuffled", n=4500, m=33000, density=0.0012, ints=3), "min", None),
    "ties5000": (dict(kind="sparse", n=5000, m=5000, density=0.01, ints=6), "max", 201),
    # E: the fp32 filter (test_f32_filter_scan_round_by_round's inputs)
    "filter_ints": (dict(kind="sparse", n=2500, m=4000, density=0.01, ints=4), "max", 161),
    "filter_single": (dict(kind="single", n=1500, density=0.02, n_single=40), "min", 161),
}
A_INPUTS = ("ties600", "single400", "f64_700")
A_OPTS = dict(tail_threshold=0, shard_min_k=-1)
A_PLAIN_ROUNDS = 25           # every round 1..25 is a cap
A_FULL = ("single400", 3)     # one whole solve: input, world
B_INPUT, B_WORLD = "ties600", 3
# inputs of _round_modes at threshold 192: (input, world, part, parts) -- a case takes every parts-th selected round
C_CASES = (("f32max", 3, 0, 1), ("ints", 3, 0, 1), ("ints", 8, 0, 2), ("ints", 8, 1, 2), ("f64", 3, 0, 1), ("planted_a", 3, 0, 1))
D_OPTS = dict(tiled_min_k=1, engine=1, tail_threshold=0)  # (the engine threshold moves shard_min_K along: 1)
D_RECT = ("rect6000", "rect4500")
D_RECT_MAX_ROUNDS = 32
D_WORLDS = (3, 8)
D_TIES_CAPS = (1, 2, 3, 5, 8, 13, 21, 40, 80, 200)
E_OPTS = dict(tiled_min_k=-1, tail_threshold=0, shard_min_k=-1)
E_INPUTS = ("filter_ints", "filter_single")
E_CAPS = (1, 2, 3, 4, 6, 9, 14, 30, 70, 160)
F_INPUTS = (  # test_degenerate_shapes: N = 1; three persons, one object (runs to max_iter); one wide row
    (np.array([[0, 0]], dtype=np.int32), np.array([3.0])),
    (np.array([[0, 0], [1, 0], [2, 0]], dtype=np.int32), np.array([3.0, 1.0, 2.0])),
    (np.array([[0, 0], [0, 3], [0, 7]], dtype=np.int32), np.array([1.0, 5.0, 2.0])),
)
F_WORLD, F_MAX_ITER = 8, 50


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(loc, val, problem, oracle keywords, trace) of a named input: one of INPUTS, or an input of _round_modes."""
    if name not in INPUTS:
        return rm.reference(name)[:5]
    spec, prob, limit = INPUTS[name]
    loc, val = cases.synth_inputs(spec)
    _freeze(loc, val)
    return loc, val, prob, {}, rm.trace(loc, val, prob, limit=limit)


@functools.lru_cache(maxsize=None)
def edges(name):
    """edges[r]: the oracle's edges_scanned after r rounds (one stepping pass; a bid scans its whole row, nothing else
    counts, so a solve capped at r ends with the same figure whether or not round r ends a phase)."""
    loc, val, prob, kw, tr = reference(name)
    o = rm._new(loc, val, prob, kw, 10**8)
    out = np.zeros(tr["total"] + 1, dtype=np.int64)
    for r in range(1, tr["total"] + 1):
        o.step()
        out[r] = o.raw_meta().edges_scanned
    return out


_STATES = {}


def expected(name, caps):
    """{r: (the oracle's state after a solve capped at r, its edges_scanned)} -- computed once per (input, round), shared by
    every test and never written again."""
    loc, val, prob, kw, tr = reference(name)
    have = _STATES.setdefault(name, {})
    if name not in INPUTS:
        have.update({r: s for r, s in rm.reference(name)[6].items() if r not in have})
    todo = [r for r in caps if r not in have]
    assert all(1 <= r <= tr["total"] and (tr["finished"] or r < tr["total"]) for r in todo), (name, todo)
    if todo:
        for r, s in rm.snapshots(loc, val, prob, kw, tr, todo).items():
            _freeze(*(a for a in s.values() if isinstance(a, np.ndarray)))
            have[r] = s
    e = edges(name)
    return {r: (have[r], int(e[r])) for r in caps}


def sharded_rounds(tr, r, shard_min_K, thr):
    """Rounds q <= r that the loop shards and exchanges: Kb[q] >= shard_min_K and Kb[q] > thr."""
    Kb = tr["Kb"][1:r + 1]
    return int(((Kb >= shard_min_K) & (Kb > max(thr, 0))).sum())


def phase_ends(tr):
    return [r for r in range(1, tr["total"] + 1) if tr["Ka"][r] == 0]


# ---- A: caps at the shard-size edges ----------------------------------------------------------------------------------------
def shard_size_caps(tr, world):
    """{b: (K, r)} for b = W-1, W, W+1: the first round r that starts with K = b bidders -- or, where no round does, with the
    nearest K on b's side (below for W-1 and W, above for W+1), as _round_modes.select does."""
    Kb = tr["Kb"]
    out = {}
    for b, lower in ((world - 1, True), (world, True), (world + 1, False)):
        ks = Kb[1:][(Kb[1:] <= b) if lower else (Kb[1:] >= b)]
        assert len(ks), (world, b)
        k = int(ks.max() if lower else ks.min())
        out[b] = (k, int(np.nonzero(Kb[1:] == k)[0][0]) + 1)
    return out


def caps_a(tr, world):
    """Rounds 1..25, the ends of the first two phases with the round after each, the shard-size edges of this W."""
    caps = set(range(1, A_PLAIN_ROUNDS + 1))
    for e in phase_ends(tr)[:2]:
        caps |= {e, e + 1}
    caps |= {r for _, r in shard_size_caps(tr, world).values()}
    return sorted(caps)


# ---- B: the shard_min_K boundary ----------------------------------------------------------------------------------------------
def boundary_round(tr, thr=rm.THR_LINES):
    """The round q of the second phase that case B puts shard_min_K at: of the rounds that start with thr < K < N, the middle
    one (the earlier of two), so that the rounds either side of it are grid-side rounds as well."""
    n = int(tr["Kb"][1:].max())
    rr = [r for r in range(1, tr["total"] + 1) if tr["phase"][r] == 1 and thr < tr["Kb"][r] < n]
    return rr[(len(rr) - 1) // 2]


def caps_b(tr, thr=rm.THR_LINES):
    """q-1, q, q+1, the first tail round of q's phase, the phase's last round, the first round of the next phase."""
    q = boundary_round(tr, thr)
    ph = tr["phase"][q]
    first_tail = next(r for r in range(q, tr["total"] + 1) if tr["phase"][r] == ph and tr["Kb"][r] <= thr)
    last = next(r for r in range(q, tr["total"] + 1) if tr["Ka"][r] == 0)
    return [q - 1, q, q + 1, first_tail, last, last + 1]


# ---- the runner -----------------------------------------------------------------------------------------------------------------
class CountingGroup(ThreadGroup):
    """ThreadGroup that counts each rank's all-reduces by kind.  `reduce_min`, if given, replaces the MIN reduction (the
    mutation runs: a wrong tie rule that is still the same on every rank)."""

    def __init__(self, world, timeout_s=TIMEOUT_S, reduce_min=None):
        super().__init__(world, timeout_s)
        self.calls = [dict(max=0, min=0) for _ in range(self.world)]
        self._reduce_min = reduce_min

    def all_reduce(self, rank, arr, op):
        self.calls[rank][op] += 1
        if op == "min" and self._reduce_min is not None:
            return self._reduce_min(self.all_gather(rank, arr))
        return super().all_reduce(rank, arr, op)


REDUCE_MIN = None  # (hook of the mutation runs; None = numpy minimum)


def run_ranks(loc, val, prob, world, max_iter, okw=None, **gpu_opts):
    """The sharded solve on `world` rank threads, every handle capped at max_iter rounds.  Returns one dict per rank:
    state, meta, gpu, error_bits, the handle's effective shard_min_K and tail_threshold, and the number of MAX and of MIN
    exchanges the rank went through.  A rank that raises aborts the group (the others then raise instead of waiting) and
    the first error is raised here."""
    from sslap_amd import from_sparse
    from sslap_amd.dist import Comm, solve_sharded
    group = CountingGroup(world, TIMEOUT_S, REDUCE_MIN)
    res, errs = [None] * world, []

    def rank_main(rank):
        try:
            comm = Comm.in_process(rank, group)
            s = from_sparse(loc, val.copy(), problem=prob, shard=(rank, world), max_iter=max_iter, cardinality_check=False,
                            **(okw or {}), **gpu_opts)
            solve_sharded(s, comm)
            res[rank] = dict(state=s.state(), meta=s.meta, gpu=s.gpu, error_bits=int(s.status().error_bits),
                             shard_min_K=s.shard_min_K, tail_threshold=s.tail_threshold, exchanges=group.calls[rank])
        except BaseException as e:  # noqa: BLE001
            errs.append((rank, e))
            group.abort()

    threads = [threading.Thread(target=rank_main, args=(k,)) for k in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        # (the ranks that only saw the broken barrier come after the one that failed first)
        errs.sort(key=lambda x: isinstance(x[1], threading.BrokenBarrierError))
        raise RuntimeError("rank %d of %d failed: %r (%d ranks raised)" % (errs[0][0], world, errs[0][1], len(errs))) from errs[0][1]
    return res


def check_ranks(res, want_state, want_edges, tr, r, what, lines=False):
    """Everything a capped sharded solve must satisfy; returns the number of sharded rounds."""
    world = len(res)
    for k, x in enumerate(res):
        d = rm.state_diff(x["state"], want_state)
        assert d is None, "%s: rank %d of %d against the oracle: %s" % (what, k, world, d)
        assert x["error_bits"] == 0, (what, k, x["error_bits"])
    for k, x in enumerate(res[1:], 1):
        d = rm.state_diff(x["state"], res[0]["state"])
        assert d is None, "%s: rank %d differs from rank 0: %s" % (what, k, d)
    s, thr = res[0]["shard_min_K"], res[0]["tail_threshold"]
    want = sharded_rounds(tr, r, s, thr)
    got = [x["gpu"]["sharded_rounds"] for x in res]
    assert got == [want] * world, "%s: sharded_rounds %s, the trace has %d rounds with K >= %d and K > %d" % (what, got, want, s, thr)
    for kind in ("max", "min"):
        got = [x["exchanges"][kind] for x in res]
        assert got == [want] * world, "%s: %s exchanges %s, sharded rounds %d" % (what, kind.upper(), got, want)
    shard = [x["gpu"]["shard_edges"] for x in res]
    repl = [x["gpu"]["edges_scanned"] - x["gpu"]["shard_edges"] for x in res]
    assert repl == [repl[0]] * world, "%s: edges of replicated rounds differ by rank: %s" % (what, repl)
    assert sum(shard) + repl[0] == want_edges, "%s: shard edges %s + replicated %d != %d" % (what, shard, repl[0], want_edges)
    if lines:
        hits = [x["gpu"]["cand_hits"] for x in res]
        assert all(h > 0 for h in hits), "%s: candidate-line hits by rank %s" % (what, hits)
    return want
