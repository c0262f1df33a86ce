"""Shared by test_single_value_edges.py (GPU) and test_single_value_edges_nogpu.py: the per-handle solve (from_sparse,
from_matrix, AuctionSolver.solve_batch, update_values + resolve) at the edges of the value range.

The graphs, the sign cases, the magnitudes of C, the eps_start cases and the stops are those of tests/_value_edges.py.
Added here are the values that matter to the single solve alone, because only it picks an edge layout from the values
(8 B/edge where every value is fp32-exact, 12 B/edge otherwise), guards its candidate lines by eps against
max_abs * 2^-44, and gates an fp32 filter on 2^-100 < max_abs < 2^60 -- each on the graphs of 70 and of 257 rows:

    f32_subnormal_exact   floor(u * 1000) * 2^-149: fp32-exact subnormals, C and eps subnormal, one phase
    f32_subnormal_mixed   the same on even entries, floor(u * 1000) * 2^-126 on odd ones
    flt_max_f32           u / u.max() * FLT_MAX rounded to float32: C == FLT_MAX, bids and prices beyond the float32 range
    one_not_f32           2 floor(u / 2) + 2^24 (even, hence fp32-exact) with the middle entry one higher: that value alone
                          is not fp32-exact
    all_f32               its twin without that entry
    below_2^-100          u / u.max() * 2^-100    \\ the two ends of the filter's range
    above_2^60            floor(u * 2^20) * 2^34  /

A case is a _value_edges.Case(name, rows, val, opts, stop); here EVERY case has a stop, given to the oracle and to the
handle alike.  The oracle's whole state after the (possibly cut) solve is computed once per (case, problem) and shared.
"""
import functools

import numpy as np

from tests import _round_modes as rm
from tests import _value_edges as ve

FLT_MAX = ve.FLT_MAX
PROBLEMS = ve.PROBLEMS
Case = ve.Case
ENDS_STOP = 1000  # for the _value_edges cases without a stop: test_batch_value_edges_nogpu.py holds them below 1000 rounds


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def _subnormal_exact(u):
    return np.floor(u * 1000) * 2.0 ** -149


def _subnormal_mixed(u):
    k = np.floor(u * 1000)
    return np.where(np.arange(len(u)) % 2 == 0, k * 2.0 ** -149, k * 2.0 ** -126)


def _flt_max_f32(u):
    return (u / u.max() * FLT_MAX).astype(np.float32).astype(np.float64)


def _all_f32(u):
    """Even integers from 2^24 up: between 2^24 and 2^25 a float32 holds the even integers only (floor(u) + 2^24 itself
    would leave every odd one inexact), so these are all fp32-exact."""
    return 2.0 * np.floor(u / 2.0) + 16777216.0


def _one_not_f32(u):
    """... and the middle entry one higher: odd, the one value that is not fp32-exact."""
    v = _all_f32(u)
    v[len(v) // 2] += 1.0
    return v


# (name, f, {rows: stop}).  The stops: rounds of the oracle (min / max) measured by test_single_value_edges_nogpu.py,
# which prints them and holds every solve to its stop --
#   f32_subnormal_exact   70: 20 / 14        257: 71 / 69
#   f32_subnormal_mixed   70: 12 / 10        257: 69 / 23
#   flt_max_f32           70: 325 / 259      257: 1134 / 1216
#   one_not_f32           70: 666 / 730      257: 2938 / 1612
#   all_f32               70: 564 / 518      257: 2482 / 1819
#   below_2^-100          70: 20 / 14        257: 71 / 69
#   above_2^60            70: 325 / 259      257: 1135 / does not end in 5000: cut at 1500
NEW = (
    ("f32_subnormal_exact", _subnormal_exact, {70: 100, 257: 300}),
    ("f32_subnormal_mixed", _subnormal_mixed, {70: 100, 257: 300}),
    ("flt_max_f32", _flt_max_f32, {70: 600, 257: 2000}),
    ("one_not_f32", _one_not_f32, {70: 2000, 257: 5000}),
    ("all_f32", _all_f32, {70: 2000, 257: 5000}),
    ("below_2^-100", lambda u: u / u.max() * 2.0 ** -100, {70: 600, 257: 2000}),
    ("above_2^60", lambda u: np.floor(u * 2.0 ** 20) * 2.0 ** 34, {70: 600, 257: 1500}),
)
NEW_NAMES = tuple(n for n, _, _ in NEW)
CUT = ("above_2^60@257",)  # of the new cases, the ones the stop cuts (under 'max'); every other one ends below its stop
FILTER_ENDS = ("below_2^-100", "above_2^60")


def key_of(name, rows):
    """A case's key: its name on the 70-row graph (and for the _value_edges cases on their own graph), name@257 on the
    other one."""
    return name if rows == ve.ROWS or (name in ve.BIG and name not in NEW_NAMES) else "%s@%d" % (name, rows)


@functools.lru_cache(maxsize=None)
def cases():
    """{key: Case}: every sparse case of _value_edges with a stop of its own, the new cases on both graphs, and
    neg_mixed on the 70-row graph as well (solve_batch takes handles of one row count)."""
    out = {}
    for c in ve.sparse_cases().values():
        out[c.name] = Case(c.name, c.rows, c.val, c.opts, ENDS_STOP if c.stop is None else c.stop)
    for name, f, stops in NEW:
        for rows, stop in stops.items():
            u = ve.graph(rows)[1]
            with np.errstate(over="raise"):
                val = np.ascontiguousarray(f(u.copy()), dtype=np.float64)
            out[key_of(name, rows)] = Case(name, rows, _frozen(val), (), stop)
    out["neg_mixed@70"] = Case("neg_mixed", ve.ROWS, _frozen(ve.graph(ve.ROWS)[1] - 50.0), (), ENDS_STOP)
    return out


def problem_of(case):
    return ve.graph(case.rows)[0], case.val


def is_f32_exact(val):
    """numpy's own float32 round trip: the 8 B/edge layout holds exactly these value sets."""
    with np.errstate(over="ignore"):
        return bool((val.astype(np.float32).astype(np.float64) == val).all())


def layout_of(val, force_f64=False):
    return 8 if is_f32_exact(val) and not force_f64 else 12


# ---- the oracle's whole state ------------------------------------------------------------------------------------------
def oracle_run(loc, val, problem, kw, max_iter, p0=None):
    """The oracle solved with max_iter (from prices p0 if given): dict(sol, state, meta, extra)."""
    with np.errstate(over="ignore"):
        o = rm._new(loc, val, problem, dict(kw), max_iter, p0)
    sol = o.solve()
    return dict(sol=sol, state=o.state(), meta=dict(o.meta), extra=dict(o.extra), max_iter=max_iter)


@functools.lru_cache(maxsize=None)
def want(key, problem, cap=None):
    """The oracle's run of a case, cut at its stop (or at `cap` rounds, for the capped handles)."""
    c = cases()[key]
    loc, val = problem_of(c)
    return oracle_run(loc, val, problem, dict(c.opts), c.stop if cap is None else cap)


def caps_of(key, problem):
    """The rounds a second handle of a CAPPED case is stopped at: round 1 and a middle round of the (cut) solve."""
    its = want(key, problem)["meta"]["its"]
    return sorted({1, max(1, its // 2)})


CAPPED = ("neg_mixed", "flt_max_f32", "f32_subnormal_exact", "ulp_2_53", "above_flt_max")  # one case per family


# ---- the guards ---------------------------------------------------------------------------------------------------------
def eps_schedule(w, n_rows):
    """The fp32 eps of every phase the run entered: eps0, then x 0.15 while eps is not below 1 / N (_warm_cases.eps_schedule
    for a run that may have been cut)."""
    with np.errstate(over="ignore", under="ignore"):
        eps, theta = np.float32(w["extra"]["start_eps_f32"]), np.float32(0.15)
        seq = [eps]
        for _ in range(w["meta"]["nreductions"]):
            eps = np.float32(eps * theta)
            seq.append(eps)
    assert seq[-1].view(np.uint32) == np.float32(w["extra"]["final_eps_f32"]).view(np.uint32)
    return seq


def lines_expected(w, n_rows, val, pmax0=0.0):
    """(phases_with_lines, eps_phases) of a handle with candidate lines: the lines serve the phases whose eps, promoted
    to double, is not below (max |v| + max starting price) * 2^-44; once dropped they stay dropped."""
    bound = (float(np.abs(val).max()) + float(pmax0)) * 2.0 ** -44
    seq = eps_schedule(w, n_rows)
    n = 0
    while n < len(seq) and not float(seq[n]) < bound:
        n += 1
    return n, len(seq)


def filter_range_ok(val, pmax0=0.0):
    m = float(np.abs(val).max())
    return 2.0 ** -100 < m < 2.0 ** 60 and pmax0 < 2.0 ** 60


LINE_CASES = ("ties_2_52", "ulp_2_53", "round_to_f32")  # the cases whose line count the GPU module asserts by name

# ---- the handle variants (the names of tests/test_round_modes.py): (id, handle options, environment) --------------------
VARIANTS = (
    ("default", {}, {}),
    ("cand0", dict(cand=False), {}),
    ("cand2", dict(cand=2), {}),
    ("thr0", dict(tail_threshold=0), {}),       # every round goes to the small / fused path
    ("thr16", dict(tail_threshold=16), {}),
    ("f64", dict(force_f64=True), {}),
    ("tile", dict(tiled_min_k=1, engine=1), {}),
    ("unfused", {}, dict(MISSLAP_ROUND_FUSED="0")),
    ("filter", dict(tiled_min_k=-1), dict(MISSLAP_F32_FILTER="1")),
)


def thr_of(kw):
    return kw.get("tail_threshold", rm.default_thr(kw.get("cand")))


# ---- grid rounds: the cases on the 2600-row graph of _round_modes.make_input("f32max") ----------------------------------
# (name, f, {problem: stop}).  Rounds of the oracle, measured by the nogpu module (min / max): neg_mixed 6110 / 4011,
# f32_subnormal_exact 284 / 1890, flt_max_f32 8830 / 11420; +inf and zero never end (the _value_edges stops); round_to_f32
# and ulp_2_53 under 'max' do not end within 20 000 and are cut a few hundred rounds in, past the first grid -> small ->
# tail descent (asserted from the K trace).
GRID = (
    ("neg_mixed", lambda u: u - 50.0, dict(min=8000, max=8000)),
    ("round_to_f32", lambda u: np.floor(u) + ve._odd_offset(u), dict(min=600, max=600)),
    ("ulp_2_53", lambda u: np.floor(u * 2.0 ** 47), dict(min=600, max=600)),
    ("f32_subnormal_exact", _subnormal_exact, dict(min=3000, max=3000)),
    ("flt_max_f32", _flt_max_f32, dict(min=15000, max=15000)),
    ("above_flt_max", lambda u: u * 1e37, dict(min=60, max=60)),
    ("c_is_zero", lambda u: u * 2.0 ** -160, dict(min=200, max=200)),
)
GRID_NAMES = tuple(n for n, _, _ in GRID)
GRID_CUT_EARLY = ("round_to_f32", "ulp_2_53")
GRID_VARIANTS = (("default", {}), ("cand0", dict(cand=False)), ("tile", dict(tiled_min_k=1, engine=1)))


@functools.lru_cache(maxsize=None)
def grid_graph():
    loc, u = rm.make_input("f32max")[:2]
    return _frozen(loc, u)


@functools.lru_cache(maxsize=None)
def grid_case(name, problem):
    """(loc, val, stop) of a grid case."""
    loc, u = grid_graph()
    f, stops = {n: (f, s) for n, f, s in GRID}[name]
    val = np.ascontiguousarray(f(u.copy()), dtype=np.float64)
    assert np.isfinite(val).all()
    return loc, _frozen(val), stops[problem]


@functools.lru_cache(maxsize=None)
def grid_want(name, problem):
    loc, val, stop = grid_case(name, problem)
    return oracle_run(loc, val, problem, {}, stop)


def grid_paths(name, problem, thr):
    """{path: rounds} of the capped solve, from the oracle's K trace."""
    loc, val, stop = grid_case(name, problem)
    tr = rm.trace(loc, val, problem, {}, limit=stop)
    out = dict.fromkeys(rm.LADDER, 0)
    for K in tr["Kb"][1:]:
        out[rm.path_of(int(K), thr)] += 1
    return out


# ---- near-tie rows for the fp32 filter -----------------------------------------------------------------------------------
# 5200 rows of 12 entries.  The eight rows of a group 8 g .. 8 g + 7 plant their three best costs on the SAME columns 8 g,
# 8 g + 1, 8 g + 2:
#     t1 = 2^-6 * (1 + i % 7),   t2 = t1 - d,   t3 = t2 - d,   d = rel * 64,  rel cycling over NEAR_TIE_REL
# all of them multiples of 2^-24 below 1/8, hence fp32-exact.  Row i also holds column i (a perfect matching exists), at
# -1/8 where it is not one of the three; the other entries are background costs in [-64, -1) on random columns, one of them
# -64 exactly: max |c| = 64 and nothing else comes near it.  With eps_start = 2^-10 (two phases) eight rows fight over
# three columns in steps of eps until five have left for their own: some hundred rounds of more than 2048 bidders each,
# i.e. full scans by k_bid through the filter, with prices that keep the three best values of a row within a few eps.
# At zero prices 2 delta = 2^-21 * 64 = 2^-15: rel = 2^-30 and 2^-23 are inside it, 2^-21 sits ON it (M2 - M3 > 2 delta is
# false: undecided), 2^-20 and 2^-18 are outside.  The 12 B/edge twin multiplies every value by 1 + 2^-30.  The costs are
# those of problem='max'; 'min' is given their negatives.
NEAR_TIE_N, NEAR_TIE_PER, NEAR_TIE_GROUP = 5200, 12, 8
NEAR_TIE_REL = (2.0 ** -30, 2.0 ** -23, 2.0 ** -21, 2.0 ** -20, 2.0 ** -18)
NEAR_TIE_MAG = 64.0
NEAR_TIE_KW = dict(eps_start=2.0 ** -10)
NEAR_TIE_STOP = 20000
NEAR_TIE_CAPS = (1, 2, 3, 6, 14, 30, 70, 160)


@functools.lru_cache(maxsize=None)
def near_tie_costs(layout):
    """(loc, cost): the near-tie graph and its costs (the values of 'max'), fp32-exact for layout 8, x (1 + 2^-30) for 12."""
    n = NEAR_TIE_N
    rng = np.random.default_rng([95])
    rows = []
    cost = []
    for i in range(n):
        top = [NEAR_TIE_GROUP * (i // NEAR_TIE_GROUP) + k for k in range(3)]
        others = [j for j in dict.fromkeys([i] + rng.choice(n, NEAR_TIE_PER, replace=False).tolist()) if j not in top][:NEAR_TIE_PER - 3]
        bg = -(1.0 + np.floor(rng.random(len(others)) * 63 * 1024) / 1024)
        d = NEAR_TIE_REL[i % len(NEAR_TIE_REL)] * NEAR_TIE_MAG
        t1 = 2.0 ** -6 * (1 + i % 7)
        entries = dict(zip(others, bg.tolist()))
        if i not in top:
            entries[i] = -0.125
        entries.update({top[0]: t1, top[1]: t1 - d, top[2]: t1 - 2 * d})
        for j in sorted(entries):
            rows.append((i, j))
            cost.append(entries[j])
    loc = np.array(rows, dtype=np.int32)
    cost = np.array(cost)
    cost[np.argmin(cost)] = -NEAR_TIE_MAG
    if layout == 12:
        cost = cost * (1.0 + 2.0 ** -30)
    return _frozen(loc, cost)


def near_tie_problem(layout, problem):
    loc, cost = near_tie_costs(layout)
    return loc, (cost if problem == "max" else -cost)


def filter_gaps(loc, cost, p=None, per_row=NEAR_TIE_PER):
    """What wave_bid_filter sees of every row (all of `per_row` entries), in numpy float32 arithmetic: (M2 - M3, 2 delta),
    with a = fl32(fl32(c) - fl32(p)) and 2 delta = 2^-21 * (fl32(max |c|) + fl32(max p))."""
    p = np.zeros(int(loc[:, 1].max()) + 1) if p is None else p
    a = (cost.astype(np.float32) - p.astype(np.float32)[loc[:, 1]]).reshape(-1, per_row)
    top = np.sort(a, axis=1)[:, -3:]
    gaps = top[:, 1] - top[:, 0]
    two_delta = np.float32(2.0 ** -21) * (np.float32(np.abs(cost).max()) + np.float32(p.max()))
    return gaps, two_delta


@functools.lru_cache(maxsize=None)
def near_tie_model(layout, problem):
    """(scans, undecided, rounds) summed over the rounds of the whole solve that start with more than 2048 bidders (the
    rounds whose full scans k_bid does): the rows in the list, and those of them that numpy's float32 arithmetic leaves
    undecided at the prices of that round.  A model of the filter, not the oracle's: used as a figure, and for the first
    round -- zero prices -- as the exact count."""
    loc, val = near_tie_problem(layout, problem)
    cost = val if problem == "max" else -val
    o = rm._new(loc, val, problem, NEAR_TIE_KW, NEAR_TIE_STOP)
    scans = undecided = rounds = 0
    done = False
    while not done:
        s = o.state()
        if s["K"] > rm.SMALL_MAX:
            gaps, two_delta = filter_gaps(loc, cost, s["p"])
            scans += s["K"]
            undecided += int((gaps[s["U"]] <= two_delta).sum())
            rounds += 1
        done = o.step()
    return scans, undecided, rounds


@functools.lru_cache(maxsize=None)
def near_tie_want(layout, problem, cap=None):
    loc, val = near_tie_problem(layout, problem)
    return oracle_run(loc, val, problem, NEAR_TIE_KW, NEAR_TIE_STOP if cap is None else cap)


# ---- warm: new values on a live handle ------------------------------------------------------------------------------------
# A force_f64 handle of neg_mixed (257 rows) is solved, given the flt_max_f32 values and re-solved from its own prices, then
# the f32_subnormal_exact values and re-solved again: C, eps0 = C / 2, the line guard (max |v| + max starting price) * 2^-44
# and the filter's range all follow the new values.  A handle's max_iter holds for each of its solves.
WARM_STEPS = ("neg_mixed", "flt_max_f32@257", "f32_subnormal_exact@257")
WARM_STOP = 4000


@functools.lru_cache(maxsize=None)
def warm_chain(problem):
    """[run]: the oracle's run of every step, each started from the prices the one before ended with (`pmax0`: their
    maximum)."""
    loc = ve.graph(ve.BIG_ROWS)[0]
    out, p = [], None
    for key in WARM_STEPS:
        w = oracle_run(loc, cases()[key].val, problem, {}, WARM_STOP, p0=p)
        w["pmax0"] = 0.0 if p is None else float(p.max())
        out.append(w)
        p = w["state"]["p"].copy()
    return out
