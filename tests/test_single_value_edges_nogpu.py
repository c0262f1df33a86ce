"""The cases of tests/_single_value_edges.py on the CPU: the oracle and numpy alone.  test_single_value_edges.py only
compares a handle with the oracle, so this module holds the tests themselves to what they claim: every case constructs
finite values and reaches the edge it is named for (C as a float32, the layout predicate, the eps schedule against the
line guard, the near-tie distances against the filter's bound), every oracle solve ends below its stop or is cut at it,
the capped grid solves walk through every round path, the oracle's results differ between cases (a comparison that
always passes would show), and the oracle time of the whole module stays small.
"""
import time

import numpy as np
import pytest

from tests import _round_modes as rm
from tests import _single_value_edges as sv
from tests import _value_edges as ve
from tests._batch_shapes import bits

F32_TINY = float(np.finfo(np.float32).tiny)
_SPENT = {}


def _timed(what, f, *a, **kw):
    t = time.perf_counter()
    out = f(*a, **kw)
    _SPENT[what] = _SPENT.get(what, 0.0) + time.perf_counter() - t
    return out


@pytest.fixture(autouse=True, scope="module")
def _oracle_loaded():
    """The oracle's library is built on first use: load it, and run one solve, before any test takes a time."""
    rm.orc.lib()
    c = sv.cases()["neg_ints"]
    sv.oracle_run(*sv.problem_of(c), "max", {}, 10)


def _c32(val):
    with np.errstate(over="ignore"):
        return np.float32(np.abs(val).max())


def test_the_case_list():
    cs = sv.cases()
    assert set(ve.sparse_cases()) <= set(cs) and all(c.stop is not None and c.stop < 10000 for c in cs.values())
    for name in sv.NEW_NAMES:
        assert cs[name].rows == ve.ROWS and cs[name + "@257"].rows == ve.BIG_ROWS
    assert len(cs) == len(ve.sparse_cases()) + 2 * len(sv.NEW) + 1 == 34
    assert set(ve.SIGN_NAMES) <= set(cs) and set(sv.LINE_CASES) <= set(cs)
    for c in cs.values():
        assert np.isfinite(c.val).all() and c.val.shape == (c.rows * ve.PER_ROW,), c.name
    assert set(sv.CAPPED) <= set(cs) and {v[0] for v in sv.VARIANTS} == {
        "default", "cand0", "cand2", "thr0", "thr16", "f64", "tile", "unfused", "filter"}


def test_every_oracle_solve_ends_below_its_stop_or_is_cut_at_it():
    """A NEVER_ENDS case (and above_2^60 on 257 rows under 'max') is cut; every new case and every case without a stop in
    _value_edges ends on its own below the stop; the others either."""
    worst = 0.0
    for key, c in sv.cases().items():
        for problem in sv.PROBLEMS:
            t = time.perf_counter()
            w = _timed("small", sv.want, key, problem)
            worst = max(worst, time.perf_counter() - t)
            its, ece = w["meta"]["its"], w["meta"]["eCE"]
            print(key, problem, "its", its, "eCE", ece, "stop", c.stop)
            assert w["state"]["its"] == its <= c.stop
            if c.name in ve.NEVER_ENDS or (key in sv.CUT and problem == "max"):
                assert its == c.stop and ece == 0, (key, problem)
            elif c.name in sv.NEW_NAMES or c.name in ve.ENDS_LATE or ve.sparse_cases()[c.name].stop is None:
                assert ece == 1 and its < c.stop, (key, problem, its)
            else:
                assert (its == c.stop and ece == 0) or (its < c.stop and ece == 1), (key, problem)
    print("slowest oracle solve on the 70 / 257-row graphs: %.4f s" % worst)
    assert worst < 0.25  # (measured: under 5 ms each)


def test_every_new_case_reaches_the_edge_it_is_named_for():
    cs = sv.cases()
    for rows in (70, 257):
        at = (lambda n: n) if rows == 70 else (lambda n: n + "@257")
        k = np.floor(ve.graph(rows)[1] * 1000)
        # fp32-exact subnormals: C and eps are subnormal float32, one phase (eps0 is far below 1 / N already)
        c = cs[at("f32_subnormal_exact")]
        assert sv.is_f32_exact(c.val) and 0 < c.val.max() < F32_TINY and np.array_equal(c.val, k * 2.0 ** -149)
        for problem in sv.PROBLEMS:
            w = sv.want(at("f32_subnormal_exact"), problem)
            start = np.float32(w["extra"]["start_eps_f32"])
            assert 0 < float(_c32(c.val)) < F32_TINY and 0 < float(start) < F32_TINY
            assert start.view(np.uint32) == np.float32(np.float64(_c32(c.val)) / 2.0).view(np.uint32)
            assert w["meta"]["nreductions"] == 0 and w["meta"]["eCE"] == 1
        # mixed: subnormal on even entries, multiples of 2^-126 (normal) on odd ones, all fp32-exact
        c = cs[at("f32_subnormal_mixed")]
        assert sv.is_f32_exact(c.val) and (c.val[0::2] < F32_TINY).all() and (c.val[1::2][k[1::2] > 0] >= F32_TINY).all()
        assert float(_c32(c.val)) >= F32_TINY
        # FLT_MAX: C narrows exactly, the costs stay in the float32 range, bids and prices leave it
        c = cs[at("flt_max_f32")]
        assert sv.is_f32_exact(c.val) and c.val.max() == sv.FLT_MAX == float(_c32(c.val))
        for problem in sv.PROBLEMS:
            w = sv.want(at("flt_max_f32"), problem)
            assert w["extra"]["start_eps_f32"] == sv.FLT_MAX / 2
            assert np.isfinite(w["state"]["p"]).all() and w["state"]["p"].max() > sv.FLT_MAX
        # exactly one value is not fp32-exact; the twin has none
        a, b = cs[at("one_not_f32")].val, cs[at("all_f32")].val
        with np.errstate(over="ignore"):
            inexact = a.astype(np.float32).astype(np.float64) != a
        assert inexact.sum() == 1 and inexact[len(a) // 2] and sv.is_f32_exact(b)
        assert (a != b).sum() == 1 and a[len(a) // 2] == b[len(a) // 2] + 1 and a[len(a) // 2] % 2 == 1
        assert sv.layout_of(a) == 12 and sv.layout_of(b) == 8
        # the two ends of the filter's range (2^-100 < max_abs < 2^60), each on the outside
        lo, hi = cs[at("below_2^-100")].val, cs[at("above_2^60")].val
        assert lo.max() == 2.0 ** -100 and not sv.filter_range_ok(lo) and sv.filter_range_ok(lo * 1.0001)
        assert 2.0 ** 60 <= hi.max() < 2.0 ** 61 and not sv.filter_range_ok(hi) and sv.filter_range_ok(hi / 4)
        assert not sv.is_f32_exact(hi) and not sv.is_f32_exact(lo)  # (27-bit integers times 2^34; full mantissas)
    # the layouts: subnormals and FLT_MAX are fp32-exact; a value above FLT_MAX is not
    want8 = {"f32_subnormal_exact", "f32_subnormal_mixed", "flt_max_f32", "all_f32", "zeros", "neg_ints",
             "neg_zero", "ties_2_52"}
    for key, c in cs.items():
        print(key, "layout", sv.layout_of(c.val))
        if c.name in want8:
            assert sv.layout_of(c.val) == 8, key
        if c.name in ("above_flt_max", "dbl_max", "one_not_f32", "round_to_f32", "c_is_zero", "below_2^-100", "above_2^60"):
            assert sv.layout_of(c.val) == 12, key
        assert sv.layout_of(c.val, force_f64=True) == 12
    assert {sv.layout_of(c.val) for c in cs.values()} == {8, 12}


def test_the_line_guard_is_crossed_where_the_gpu_module_says_so():
    """phases_with_lines as the handle must report it: the phases whose eps is not below max_abs * 2^-44.  Of the three
    cases named for it, the ones whose schedule crosses the guard inside the stop report fewer phases with lines than
    phases; those that stay above it report all of them."""
    crossed = {}
    for key, c in sv.cases().items():
        for problem in sv.PROBLEMS:
            w = sv.want(key, problem)
            with_lines, phases = sv.lines_expected(w, c.rows, c.val)
            assert phases == w["meta"]["nreductions"] + 1 and 0 <= with_lines <= phases
            if c.name in sv.LINE_CASES:
                print(key, problem, "phases with lines", with_lines, "of", phases)
                crossed[(key, problem)] = with_lines < phases
    # eps falls below the guard where the values are 2^53 wide and the solve runs 16 phases; the cut ties_2_52 solve (3
    # or 4 phases in 300 rounds) and the integers near 2^24 stay above it
    assert crossed == {(k, p): k == "ulp_2_53" for k in sv.LINE_CASES for p in sv.PROBLEMS}
    # C == 0 with positive values: eps == 0 is below the guard from the first phase; all zeros: 0 is not below 0
    for problem in sv.PROBLEMS:
        c = sv.cases()["c_is_zero"]
        assert sv.lines_expected(sv.want("c_is_zero", problem), c.rows, c.val)[0] == 0
        c = sv.cases()["zeros"]
        assert sv.lines_expected(sv.want("zeros", problem), c.rows, c.val) == (1, 1)


def test_the_oracle_tells_the_cases_apart():
    """sol and price bits differ between sign cases and between magnitude cases on one graph."""
    for problem in sv.PROBLEMS:
        for a, b in (("all_neg", "c_from_negative"), ("flt_max_f32", "f32_subnormal_exact"), ("one_not_f32", "ulp_2_53"),
                     ("neg_mixed@70", "all_neg"), ("above_2^60", "below_2^-100")):
            wa, wb = sv.want(a, problem), sv.want(b, problem)
            assert not np.array_equal(bits(wa["state"]["p"]), bits(wb["state"]["p"])), (a, b)
        sols = {sv.want(k, problem)["sol"].tobytes() for k in ("all_neg", "c_from_negative", "flt_max_f32", "one_not_f32",
                                                               "f32_subnormal_exact", "neg_mixed@70")}
        assert len(sols) >= 3
    # the one inexact value changes the layout, and the solve with it
    assert any(not np.array_equal(bits(sv.want("one_not_f32", p)["state"]["p"]), bits(sv.want("all_f32", p)["state"]["p"]))
               for p in sv.PROBLEMS)


def test_both_zero_cases_give_the_solver_a_negative_zero_cost():
    """The solver maximises cost = v for 'max' and cost = -v for 'min': neg_zero holds -0.0 under 'max', and the +0.0 of
    neg_ints becomes -0.0 under 'min'.  cost - p is then -0.0 at a zero price while another entry's c - p with c == p is
    +0.0: equal values, a tie that the later stored index wins -- the oracle gives both cases the same solve."""
    cs = sv.cases()
    assert np.signbit(cs["neg_zero"].val[cs["neg_zero"].val == 0]).all()
    z = -cs["neg_ints"].val
    assert (z == 0).any() and np.signbit(z[z == 0]).all()
    for problem in sv.PROBLEMS:
        a, b = sv.want("neg_ints", problem), sv.want("neg_zero", problem)
        assert np.array_equal(a["sol"], b["sol"]) and np.array_equal(bits(a["state"]["p"]), bits(b["state"]["p"]))
        assert a["meta"]["its"] == b["meta"]["its"] and a["meta"]["eCE"] == 1
    # ... and such ties do decide bids: in some round a bidder's best value is zero and is held by a -0.0 and a +0.0 at once
    for key, problem in (("neg_zero", "max"), ("neg_ints", "min")):
        c = cs[key]
        loc, val = sv.problem_of(c)
        cost = (val if problem == "max" else -val).reshape(c.rows, ve.PER_ROW)
        cols = loc[:, 1].reshape(c.rows, ve.PER_ROW)
        o = rm._new(loc, val, problem, {}, c.stop)
        mixed, done = 0, False
        while not done:
            st = o.state()
            v = cost[st["U"]] - st["p"][cols[st["U"]]]
            top = v == v.max(axis=1, keepdims=True)
            mixed += int(((v.max(axis=1) == 0) & (top & np.signbit(v)).any(1) & (top & ~np.signbit(v)).any(1)).sum())
            done = o.step()
        print(key, problem, "bids whose best value is held by a -0.0 and a +0.0:", mixed)
        assert mixed > 0


def test_the_capped_handles_stop_at_round_1_and_in_the_middle():
    for key in sv.CAPPED:
        for problem in sv.PROBLEMS:
            caps = sv.caps_of(key, problem)
            assert caps[0] == 1 and caps[-1] <= sv.want(key, problem)["meta"]["its"]
            for r in caps:
                w = _timed("small", sv.want, key, problem, r)
                assert w["state"]["its"] == r


@pytest.mark.parametrize("problem", sv.PROBLEMS)
def test_the_grid_cases_walk_through_every_round_path(problem):
    n = sv.grid_graph()[0][:, 0].max() + 1
    assert n == 2600 > rm.SMALL_MAX
    for name in sv.GRID_NAMES:
        loc, val, stop = sv.grid_case(name, problem)
        t = time.perf_counter()
        w = _timed("grid", sv.grid_want, name, problem)
        dt = time.perf_counter() - t
        its, ece = w["meta"]["its"], w["meta"]["eCE"]
        print(name, problem, "its", its, "eCE", ece, "stop", stop, "%.3f s" % dt)
        assert stop <= 20000 and dt < 2.0  # (measured: under 0.2 s)
        if name in ("above_flt_max", "c_is_zero") or name in sv.GRID_CUT_EARLY:
            assert its == stop or (ece == 1 and its < stop)
        else:
            assert ece == 1 and its < stop, (name, its)
        if name in sv.GRID_CUT_EARLY or its == stop and name not in ("above_flt_max", "c_is_zero"):
            # cut: the solve still passes through every path, at the default threshold with and without lines
            for thr in (rm.THR_LINES, rm.THR_NOLINES):
                paths = _timed("grid", sv.grid_paths, name, problem, thr)
                print(name, problem, "thr", thr, paths)
                assert all(paths[p] > 0 for p in rm.ladder(thr, n)), (name, thr, paths)
    # the first round of every case is a grid round, whatever the stop
    assert rm.path_of(n, rm.THR_LINES) == "grid"


def test_near_tie_rows_sit_on_both_sides_of_the_filter_bound():
    for layout in (8, 12):
        loc, cost = sv.near_tie_costs(layout)
        n = int(loc[:, 0].max()) + 1
        assert n == sv.NEAR_TIE_N >= 2500 and len(cost) == n * sv.NEAR_TIE_PER and np.unique(loc, axis=0).shape[0] == len(loc)
        assert (np.bincount(loc[:, 0]) == sv.NEAR_TIE_PER).all() and (loc[:, 1].reshape(n, -1) == np.arange(n)[:, None]).any(1).all()
        assert sv.layout_of(cost) == layout and np.abs(cost).max() == sv.NEAR_TIE_MAG * (1 if layout == 8 else 1 + 2.0 ** -30)
        assert sv.filter_range_ok(cost)
        gaps, two_delta = sv.filter_gaps(loc, cost)
        assert two_delta == np.float32(2.0 ** -21 * 64)
        rel = np.array([sv.NEAR_TIE_REL[i % 5] for i in range(n)])
        # in float32 arithmetic M2 - M3 is the planted distance exactly
        assert np.array_equal(gaps.astype(np.float64), rel * sv.NEAR_TIE_MAG)
        undecided = gaps <= two_delta
        print("layout", layout, "undecided at zero prices:", int(undecided.sum()), "of", n)
        assert np.array_equal(undecided, rel <= 2.0 ** -21) and undecided.sum() == n * 3 // 5
        # a bound four times smaller would decide the rows at 2^-21: they are what tells the two bounds apart
        assert ((gaps > two_delta / 4) & undecided).sum() == (rel == 2.0 ** -21).sum() == n // 5
        for problem in sv.PROBLEMS:
            t = time.perf_counter()
            w = _timed("grid", sv.near_tie_want, layout, problem)
            scans, und, rounds = _timed("grid", sv.near_tie_model, layout, problem)
            print("near ties", layout, problem, "its", w["meta"]["its"], "eCE", w["meta"]["eCE"], "rounds with K > 2048:", rounds,
                  "scans", scans, "undecided by the numpy model", und, "%.3f s" % (time.perf_counter() - t))
            assert w["meta"]["eCE"] == 1 and w["meta"]["its"] < sv.NEAR_TIE_STOP and w["meta"]["nreductions"] == 1
            # many rounds of full scans, and at their prices too rows sit on both sides of the bound
            assert rounds >= 100 and n * 3 // 5 < und < scans - (n - n * 3 // 5)
            assert max(sv.NEAR_TIE_CAPS) < w["meta"]["its"]
    # 'min' is given the negated costs: the same solve
    a, b = sv.near_tie_want(8, "max"), sv.near_tie_want(8, "min")
    assert np.array_equal(a["sol"], b["sol"]) and np.array_equal(bits(a["state"]["p"]), bits(b["state"]["p"]))


def test_the_warm_chain_moves_every_guard():
    for problem in sv.PROBLEMS:
        chain = _timed("small", sv.warm_chain, problem)
        vals = [sv.cases()[k].val for k in sv.WARM_STEPS]
        for k, (w, val) in enumerate(zip(chain, vals)):
            with_lines, phases = sv.lines_expected(w, ve.BIG_ROWS, val, w["pmax0"])
            print(sv.WARM_STEPS[k], problem, "its", w["meta"]["its"], "eCE", w["meta"]["eCE"], "pmax0 %.3g" % w["pmax0"],
                  "lines", with_lines, "of", phases)
            assert w["meta"]["its"] <= sv.WARM_STOP
            assert np.float32(w["extra"]["start_eps_f32"]) == np.float32(np.float64(_c32(val)) / 2.0)  # the new C / 2
        assert chain[0]["meta"]["eCE"] == 1 and chain[1]["meta"]["eCE"] == 1
        # from prices near FLT_MAX a subnormal eps is below the guard: no phase of the last solve has lines
        assert chain[2]["pmax0"] > sv.FLT_MAX / 2
        assert sv.lines_expected(chain[2], ve.BIG_ROWS, vals[2], chain[2]["pmax0"])[0] == 0
        assert sv.lines_expected(chain[1], ve.BIG_ROWS, vals[1], chain[1]["pmax0"])[0] >= 1


def test_the_dense_cases_have_small_stops():
    for name, c in ve.dense_cases().items():
        for problem in sv.PROBLEMS:
            its = ve.dense_want(name, problem)["meta"]["its"]
            assert its <= (sv.ENDS_STOP if c.stop is None else c.stop) < 10000


def test_zz_the_oracle_time_of_this_module_stays_small():
    print({k: round(v, 3) for k, v in _SPENT.items()})
    assert sum(_SPENT.values()) < 60.0
