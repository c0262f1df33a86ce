"""Shared by test_round_modes.py (GPU) and test_round_modes_nogpu.py: which rounds of a solve sit at the boundaries
between the five code paths that serve a round, and the oracle's state after each of them.

A round is routed by K, the number of unassigned bidders at its start (host_rounds.hpp / host_comm.hpp):
    K > 2048 grid kernels | thr < K <= 2048 small round | 16 < K <= thr block | 3 <= K <= 16 team | K <= 2 pair
with thr the handle's tail threshold.  The oracle is stepped once per input (K before and after every round), the
rounds are selected from that trace for each threshold in use, and a second stepping pass takes the snapshots.  A round
that ends an eps-phase is special: oracle_step applies the eps reduction and resets the list inside that step, while a
solve capped at that round stops in front of the reset -- its expected state comes from a capped oracle solve."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as orc
from sslap_amd import synth

SMALL_MAX = 2048  # kRoundSmallMax
TEAM_MAX = 16     # kTeamMax
HASH_FROM = 64    # block rounds above this resolve through the LDS hash table
THR_LINES, THR_NOLINES = 192, 40  # kDefaultTailThreshold, kDefaultTailThresholdNoLines
LADDER = ("grid", "small", "block", "team", "pair")
STATE_FIELDS = ("K", "U", "p", "p2o", "o2p", "its", "nreductions", "eps")


def default_thr(cand):
    return THR_NOLINES if cand is False or cand == 0 else THR_LINES


def path_of(K, thr):
    """The path that serves a round starting with K bidders (None: K == 0, the phase is over)."""
    if K <= 0:
        return None
    if K > max(thr, 0):
        return "grid" if K > SMALL_MAX else "small"
    return "pair" if K <= 2 else "team" if K <= TEAM_MAX else "block"


def ladder(thr, n):
    """The paths a phase of an n-person problem can walk through at this threshold, top down."""
    t = min(n, max(thr, 0))  # the most bidders a tail round can start with
    have = dict(grid=n > SMALL_MAX, small=min(n, SMALL_MAX) > max(thr, 0), block=t > TEAM_MAX, team=t >= 3, pair=t >= 1)
    return [p for p in LADDER if have[p]]


def boundaries(thr):
    out = []
    for b in (1, 2, 3, TEAM_MAX, TEAM_MAX + 1, HASH_FROM, HASH_FROM + 1, thr, thr + 1, SMALL_MAX, SMALL_MAX + 1):
        if b not in out:
            out.append(b)
    return out


def _is_lower(b, thr):
    return b in (1, 2, TEAM_MAX, HASH_FROM, thr, SMALL_MAX)


def spread(rounds, k):
    if len(rounds) <= k:
        return list(rounds)
    idx = np.unique(np.linspace(0, len(rounds) - 1, k).round().astype(int))
    return [rounds[i] for i in idx]


# ---- inputs ---------------------------------------------------------------------------------------------------------
def f64_values(loc, seed):
    r = np.random.default_rng(seed)
    return r.random(loc.shape[0]) * 10.0 + r.random(loc.shape[0]) * 1e-9  # full 53-bit mantissas


def planted(n, per, seed, hot, groups):
    """gen_sparse rows (values scaled into [0, 1]) plus `hot` objects that every row holds at 100, 100.125, ...; and
    every person's own object of the generator's injection raised to the value of the person's group, `groups` a list of
    (size, value) with the last group taking the rest.  All persons fight over the hot objects at the same prices, so a
    whole group leaves for its own objects in the same round, without conflicts: K falls through several paths in one
    round, and a phase ends when the last group leaves, from whatever path that group's size puts it in.  The price
    war is bounded: (100 - lowest group value) / eps rounds per hot object."""
    m = n + 8  # (spare objects: the hot ones are nobody's own)
    loc, val = synth.gen_sparse(n, m, per / m, seed=seed)
    rng = np.random.default_rng(seed)
    free = np.argsort(synth._stream(seed, 1, m), kind="stable")  # the injection gen_sparse plants: row i holds own[i]
    own, free = free[:n], free[n:]
    group_val = np.empty(n)
    order, at = rng.permutation(n), 0
    for k, (size, value) in enumerate(groups):
        size = n - at if k == len(groups) - 1 else size
        group_val[order[at:at + size]] = value
        at += size
    hot_objs = free[:hot]
    rows = [dict() for _ in range(n)]
    for (i, j), v in zip(loc.tolist(), val.tolist()):
        rows[i][j] = v / 100.0
    for i in range(n):
        assert int(own[i]) in rows[i]
        rows[i][int(own[i])] = group_val[i]
        for k, h in enumerate(hot_objs.tolist()):
            rows[i][h] = 100.0 + 0.125 * k
    out_loc = [(i, j) for i in range(n) for j in sorted(rows[i])]
    out_val = [rows[i][j] for i, j in out_loc]
    return np.array(out_loc, dtype=np.int32), np.array(out_val, dtype=np.float32).astype(np.float64)


def make_input(name):
    """name -> (loc, val, problem, oracle / solver keywords)."""
    if name == "f32max":
        return synth.gen_sparse(2600, 2600, 12.0 / 2600, seed=41) + ("max", {})
    if name == "f32min":
        return synth.gen_sparse(2600, 2600, 12.0 / 2600, seed=41) + ("min", {})
    if name == "ints":
        return synth.gen_sparse(2600, 2600, 12.0 / 2600, seed=42, integer_values=3) + ("max", {})
    if name == "f64":
        loc, _ = synth.gen_sparse(2600, 2600, 12.0 / 2600, seed=43)
        return loc, f64_values(loc, 43), "min", {}
    if name.startswith("planted"):
        spec = PLANTED[name]
        loc, val = planted(spec["n"], spec["per"], spec["seed"], spec["hot"], spec["groups"])
        return loc, val, "max", dict(eps_start=spec["eps_start"])
    if name.startswith("start"):  # start<n><problem>: the first round starts directly in a path
        n, prob = int(name[5:-3]), name[-3:]
        return synth.gen_sparse(n, n, min(6, n) / n, seed=50 + n) + (prob, {})
    raise KeyError(name)


# mode-skipping inputs (see planted); the round counts are asserted in test_round_modes_nogpu.py
PLANTED = {
    "planted_a": dict(n=2600, per=6, seed=61, hot=3, groups=[(100, 40.0), (6, 20.0), (0, 60.0)], eps_start=0.5),
    "planted_b": dict(n=600, per=6, seed=62, hot=2, groups=[(12, 40.0), (0, 60.0)], eps_start=0.25),
}
PLANTED_MAX_ROUNDS = 50_000


# ---- the oracle's trace ---------------------------------------------------------------------------------------------
def _new(loc, val, prob, kw, max_iter, p0=None):
    o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=max_iter, cardinality_check=False, **kw)
    if p0 is not None:  # warm start: the starting prices written into the live price array (tests/test_warm_start.py)
        np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))[:] = p0
    return o


def trace(loc, val, prob, kw=None, p0=None, limit=None):
    """One stepping pass: Kb[r], Ka[r] (K before / after round r, Ka == 0 where the round ends its phase), phase[r]
    (reductions before the round), 1-based (index 0 unused); stops after `limit` rounds if given."""
    o = _new(loc, val, prob, kw or {}, 10**8, p0)
    Kb, Ka, ph = [0], [0], [0]
    m = o.raw_meta()
    while True:
        Kb.append(m.num_unassigned)
        ph.append(m.nreductions)
        done = o.step()
        m = o.raw_meta()  # (behind a step that ends a phase: already the start of the next one)
        Ka.append(0 if m.nreductions != ph[-1] else m.num_unassigned)
        if done or (limit is not None and len(Kb) - 1 >= limit):
            break
    return dict(Kb=np.array(Kb), Ka=np.array(Ka), phase=np.array(ph), total=len(Kb) - 1, finished=bool(done))


def select(tr, thr):
    """The rounds of a trace to check at tail threshold `thr`.  Returns dict(rounds: sorted list, kinds: {kind: rounds},
    nearest: {b: K used instead}, paths: {path: selected rounds that start in it})."""
    Kb, Ka, total = tr["Kb"], tr["Ka"], tr["total"]
    n = int(Kb[1:].max())
    lad = ladder(thr, n)
    rs = np.arange(total + 1)
    kinds, nearest = {}, {}
    # boundary rounds
    for b in boundaries(thr):
        hit = rs[1:][Kb[1:] == b]
        if len(hit) == 0:
            side = Kb[1:] <= b if _is_lower(b, thr) else Kb[1:] >= b
            if not side.any():
                continue
            ks = Kb[1:][side]
            k = int(ks.max() if _is_lower(b, thr) else ks.min())
            nearest[b] = k
            hit = rs[1:][Kb[1:] == k][:1]
        kinds["K=%d" % b] = spread([int(r) for r in hit], 3)
    # crossing and mode-skipping rounds, with the round before and the round after
    cross = {}
    for r in range(1, total + 1):
        if Ka[r] > 0:
            a, b = path_of(Kb[r], thr), path_of(Ka[r], thr)
            if a != b:
                cross.setdefault((a, b), []).append(r)
    for (a, b), rr in cross.items():
        tag = "cross" if lad.index(b) - lad.index(a) == 1 else "skip"
        sel = []
        for r in spread(rr, 3):
            sel += [x for x in (r - 1, r, r + 1) if 1 <= x <= total]
        kinds["%s %s->%s" % (tag, a, b)] = sorted(set(sel))
    # phase ends: the first, a middle and the last phase, plus the first round of the phase that follows
    ends = [r for r in range(1, total + 1) if Ka[r] == 0]
    sel = []
    for r in spread(ends, 3):
        sel += [x for x in (r, r + 1) if x <= total]
    kinds["phase end"] = sorted(set(sel))
    for p in lad[:-1]:  # phases that end from a path other than pair
        rr = [r for r in ends if path_of(Kb[r], thr) == p]
        if rr:
            sel = []
            for r in spread(rr, 3):
                sel += [x for x in (r, r + 1) if x <= total]
            kinds["end from %s" % p] = sorted(set(sel))
    rounds = sorted(set(r for v in kinds.values() for r in v))
    paths = {p: sum(1 for r in rounds if path_of(Kb[r], thr) == p) for p in lad}
    return dict(rounds=rounds, kinds=kinds, nearest=nearest, paths=paths, ladder=lad)


def capped_state(loc, val, prob, kw, r, p0=None):
    o = _new(loc, val, prob, kw or {}, r, p0)
    o.solve()
    return o.state()


def snapshots(loc, val, prob, kw, tr, rounds, p0=None):
    """{r: the oracle's state after r rounds, as a solve capped at r leaves it} for the given rounds: snapshots of one
    stepping pass, capped solves (in threads: the oracle is plain C behind ctypes) for the rounds that end a phase."""
    rounds = sorted(set(rounds))
    stepped = [r for r in rounds if tr["Ka"][r] != 0 or r == tr["total"]]
    capped = [r for r in rounds if not (tr["Ka"][r] != 0 or r == tr["total"])]
    out = {}
    if stepped:
        o = _new(loc, val, prob, kw or {}, 10**8, p0)
        want, r = set(stepped), 0
        while r < stepped[-1]:
            o.step()
            r += 1
            if r in want:
                out[r] = o.state()
    if capped:
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            for r, s in zip(capped, ex.map(lambda x: capped_state(loc, val, prob, kw, x, p0), capped)):
                out[r] = s
    return out


def mode_rounds(tr, thr):
    """Rounds of the whole solve per path."""
    out = dict.fromkeys(LADDER, 0)
    for K in tr["Kb"][1:]:
        out[path_of(int(K), thr)] += 1
    return out


# ---- per input, shared by every test of a session -----------------------------------------------------------------------
# the thresholds each input is checked at (the variants of test_round_modes.py)
THRS = {
    "f32max": (192, 16, 512, 40), "f32min": (192, 40), "ints": (192, 16), "f64": (192, 512, 40),
    "planted_a": (192, 40), "planted_b": (192, 40),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(loc, val, problem, kw, trace, {thr: selection}, {r: state}) of a named input, computed once."""
    loc, val, prob, kw = make_input(name)
    limit = PLANTED_MAX_ROUNDS + 1 if name.startswith("planted") else None
    tr = trace(loc, val, prob, kw, limit=limit)
    if not tr["finished"]:
        return loc, val, prob, kw, tr, {}, {}
    thrs = THRS.get(name, (THR_LINES, THR_NOLINES))
    sels = {thr: select(tr, thr) for thr in thrs}
    snaps = snapshots(loc, val, prob, kw, tr, [r for s in sels.values() for r in s["rounds"]])
    for s in snaps.values():
        for a in s.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return loc, val, prob, kw, tr, sels, snaps


def state_diff(got, want):
    """The first field of two state() dicts that differs (None: equal) -- prices by their bits, eps as fp32."""
    if got["its"] != want["its"]:
        return "its %d != %d" % (got["its"], want["its"])
    if got["K"] != want["K"]:
        return "K %d != %d" % (got["K"], want["K"])
    if not np.array_equal(got["U"], want["U"]):
        return "U (list order)"
    if not np.array_equal(got["p"].view(np.uint64), want["p"].view(np.uint64)):
        return "price bits (%d objects differ)" % int((got["p"].view(np.uint64) != want["p"].view(np.uint64)).sum())
    if not np.array_equal(got["p2o"], want["p2o"]):
        return "p2o"
    if not np.array_equal(got["o2p"], want["o2p"]):
        return "o2p"
    if got["nreductions"] != want["nreductions"]:
        return "nreductions %d != %d" % (got["nreductions"], want["nreductions"])
    if np.float32(got["eps"]) != np.float32(want["eps"]):
        return "eps %r != %r" % (got["eps"], want["eps"])
    return None
