"""The per-handle solve on the GPU at the edges of the value range (the cases of tests/_single_value_edges.py): the sign
cases, the magnitudes of C and the eps_start cases of the batch tests, fp32-exact subnormals and FLT_MAX in the 8 B/edge
layout, one value that alone flips the layout to 12 B/edge, the two ends of the fp32 filter's range, eps against the
line guard max_abs * 2^-44, and rows whose three best values lie within and beyond the filter's bound.

Every case runs for both problems through nine handle variants (the options of test_round_modes.py, MISSLAP_ROUND_FUSED=0
and the forced fp32 filter), and the WHOLE state is compared with the oracle's with `==` on bits: its, K, the list in
order, prices, p2o, o2p, nreductions, fp32 eps, error_bits == 0, eCE, soln_found, n_assigned, obj_f64, the fp32 bits of
start_eps and final_eps, and the layout against numpy's own float32 round trip of the values.  Every solve has an explicit
max_iter, the same as the oracle's (test_single_value_edges_nogpu.py holds each oracle solve to it).
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import AuctionSolver, from_matrix, from_sparse
from tests import _round_modes as rm
from tests import _single_value_edges as sv
from tests import _value_edges as ve
from tests._batch_shapes import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _quiet_narrowing():
    """eps_start = 1e39 narrows to +inf as a float32, which numpy reports: that is the case."""
    with np.errstate(over="ignore"):
        yield


def _f32_bits(x):
    return np.float32(x).view(np.uint32)


def _same_float(a, b):
    return a == b or (a != a and b != b)


def _same(g, sol, w, what, layout=None):
    """Handle `g` after solve() / resolve() -> sol, against an oracle run of _single_value_edges.oracle_run."""
    sg, so = g.state(), w["state"]
    assert sg["its"] == so["its"] and sg["K"] == so["K"], (what, sg["its"], so["its"], sg["K"], so["K"])
    assert np.array_equal(sg["U"], so["U"]), what
    assert np.array_equal(bits(sg["p"]), bits(so["p"])), (what, int((bits(sg["p"]) != bits(so["p"])).sum()))
    assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), what
    assert sg["nreductions"] == so["nreductions"] and _f32_bits(sg["eps"]) == _f32_bits(so["eps"]), what
    assert g.status().error_bits == 0, (what, g.status().error_bits)
    assert np.array_equal(sol, w["sol"]), what
    for k in ("its", "eCE", "soln_found", "n_assigned", "nreductions"):
        assert g.meta[k] == w["meta"][k], (what, k, g.meta[k], w["meta"][k])
    assert _same_float(g.gpu["obj_f64"], w["extra"]["obj_f64"]), (what, g.gpu["obj_f64"], w["extra"]["obj_f64"])
    for k in ("start_eps_f32", "final_eps_f32"):
        assert _f32_bits(g.gpu[k]) == _f32_bits(w["extra"][k]), (what, k, g.gpu[k], w["extra"][k])
    assert g.gpu["eps_phases"] == w["meta"]["nreductions"] + 1, what
    if layout is not None:
        assert g.gpu["bytes_per_edge"] == layout, (what, g.gpu["bytes_per_edge"], layout)


def _handle(loc, val, problem, max_iter, opts=(), **kw):
    return from_sparse(loc, val.copy(), problem=problem, max_iter=max_iter, cardinality_check=False, **dict(opts), **kw)


def _lines(g, w, rows, val, kw, what, pmax0=0.0):
    """phases_with_lines: the phases whose eps is not below the guard, where the handle keeps lines at all."""
    with_lines, phases = sv.lines_expected(w, rows, val, pmax0)
    want = 0 if kw.get("cand") is False else with_lines
    assert (g.gpu["phases_with_lines"], g.gpu["eps_phases"]) == (want, phases), (what, g.gpu["phases_with_lines"], want, phases)
    return with_lines, phases


# ---- every case through every variant ------------------------------------------------------------------------------------

@pytest.mark.parametrize("problem", sv.PROBLEMS)
@pytest.mark.parametrize("variant", sv.VARIANTS, ids=[v[0] for v in sv.VARIANTS])
def test_every_case_ends_in_the_oracle_state(variant, problem, gpu_lib, monkeypatch):
    vid, kw, env = variant
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = set()
    for key, c in sv.cases().items():
        loc, val = sv.problem_of(c)
        what = "%s %s %s" % (key, problem, vid)
        g = _handle(loc, val, problem, c.stop, c.opts, **kw)
        assert g.tail_threshold == sv.thr_of(kw), what
        sol = g.solve()
        w = sv.want(key, problem)
        _same(g, sol, w, what, sv.layout_of(val, kw.get("force_f64", False)))
        with_lines, phases = _lines(g, w, c.rows, val, kw, what)
        if c.name in sv.LINE_CASES and kw.get("cand") is not False:
            # eps falls below max_abs * 2^-44 inside the stop for ulp_2_53 only (the nogpu module holds this)
            if c.name == "ulp_2_53":
                assert 0 < g.gpu["phases_with_lines"] < g.gpu["eps_phases"] and g.gpu["lines_active"] == 0, what
            else:
                assert g.gpu["phases_with_lines"] == g.gpu["eps_phases"] and g.gpu["lines_active"] == 1, what
        if vid == "filter":
            # the handle has the filter's mirror exactly where max_abs is inside (2^-100, 2^60)
            assert (g.gpu["filter_undecided"] >= 0) == sv.filter_range_ok(val), (what, g.gpu["filter_undecided"])
        else:
            assert g.gpu["filter_undecided"] == -1, what
        seen.add(c.name)
    assert seen >= set(ve.SIGN_NAMES) | set(sv.NEW_NAMES) | set(sv.LINE_CASES)


@pytest.mark.parametrize("problem", sv.PROBLEMS)
@pytest.mark.parametrize("key", sv.CAPPED)
def test_capped_at_round_1_and_at_a_middle_round(key, problem, gpu_lib, monkeypatch):
    """One case per family: a second handle stopped after round 1 and after a middle round, in every variant."""
    c = sv.cases()[key]
    loc, val = sv.problem_of(c)
    for vid, kw, env in sv.VARIANTS:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            for r in sv.caps_of(key, problem):
                g = _handle(loc, val, problem, r, c.opts, **kw)
                sol = g.solve()
                _same(g, sol, sv.want(key, problem, r), "%s %s %s capped at round %d" % (key, problem, vid, r),
                      sv.layout_of(val, kw.get("force_f64", False)))


def test_one_inexact_value_flips_the_layout(gpu_lib):
    for rows in (ve.ROWS, ve.BIG_ROWS):
        a, b = sv.cases()[sv.key_of("one_not_f32", rows)], sv.cases()[sv.key_of("all_f32", rows)]
        loc = ve.graph(rows)[0]
        ga, gb = _handle(loc, a.val, "max", a.stop), _handle(loc, b.val, "max", b.stop)
        ga.solve(), gb.solve()
        assert ga.gpu["bytes_per_edge"] == 12 and gb.gpu["bytes_per_edge"] == 8
    for name in ("f32_subnormal_exact", "f32_subnormal_mixed", "flt_max_f32"):  # fp32-exact: subnormals and FLT_MAX are
        c = sv.cases()[name]
        g = _handle(ve.graph(c.rows)[0], c.val, "min", c.stop)
        g.solve()
        assert g.gpu["bytes_per_edge"] == 8, name


# ---- grid rounds: 2600 rows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("problem", sv.PROBLEMS)
@pytest.mark.parametrize("name", sv.GRID_NAMES)
def test_grid_rounds_on_2600_rows(name, problem, gpu_lib):
    loc, val, stop = sv.grid_case(name, problem)
    w = sv.grid_want(name, problem)
    for vid, kw in sv.GRID_VARIANTS:
        what = "%s %s %s (2600 rows)" % (name, problem, vid)
        g = _handle(loc, val, problem, stop, **kw)
        sol = g.solve()
        _same(g, sol, w, what, sv.layout_of(val))
        _lines(g, w, 2600, val, kw, what)
        assert g.gpu["grid_rounds"] > 0 and g.gpu["grid_rounds"] + g.gpu["tail_rounds"] == w["meta"]["its"], what
        if vid == "tile":
            assert g.gpu["tiled_active"] == 1, what
    g = _handle(loc, val, problem, 1)  # the first round alone: 2600 bidders, a grid round
    sol = g.solve()
    _same(g, sol, sv.oracle_run(loc, val, problem, {}, 1), "%s %s round 1 (2600 rows)" % (name, problem), sv.layout_of(val))
    assert g.gpu["grid_rounds"] == 1 and g.gpu["tail_rounds"] == 0


# ---- the fp32 filter on near-tie rows --------------------------------------------------------------------------------------

@pytest.mark.parametrize("problem", sv.PROBLEMS)
@pytest.mark.parametrize("layout", [8, 12])
def test_near_tie_rows_through_the_fp32_filter(layout, problem, gpu_lib, monkeypatch):
    """Rows whose three best values lie 2^-30 .. 2^-18 of the magnitude apart, through the forced filter where k_bid does
    the full scans (tiled_min_k=-1): bit parity with the oracle after the first rounds and at the end, with and without
    candidate lines.  The rows the filter cannot decide go to the exact scan and are counted: after round 1 (zero prices)
    they are exactly the rows planted at 2^-30, 2^-23 and 2^-21 -- three in five; a bound of 2^-23 instead of 2^-21 would
    decide the rows at 2^-21 and count two in five -- and over the whole solve some but not all scans.
    Measured: 3120 after round 1; 14 845 of 1 004 936 scans over the whole solve without lines, 14 317 with lines (numpy's
    float32 model of the filter at the oracle's prices, printed beside it: 14 474).  With 2^-23 in place of 2^-21 the count
    after round 1 is 2080 while every state still equals the oracle's: that bound is still sufficient for three roundings,
    so the count is what tells the two apart."""
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")
    loc, val = sv.near_tie_problem(layout, problem)
    n = sv.NEAR_TIE_N
    scans, model, rounds = sv.near_tie_model(layout, problem)
    # without lines every full scan of k_bid goes through the filter; with lines those of the rounds above
    # cand_build_max_k do (below it k_bid builds a line from the scan and reads the row exactly), set to 2048 here: the
    # default, max(0.3 N, 8192), would leave this graph's rounds without a single filter scan
    for cand in (rm.SMALL_MAX, False):
        kw = dict(sv.NEAR_TIE_KW, tiled_min_k=-1, **(dict(cand=False) if cand is False else dict(cand_build_max_k=cand)))
        for r in sv.NEAR_TIE_CAPS + (sv.NEAR_TIE_STOP,):
            what = "near ties, layout %d, %s, %s, max_iter=%d" % (layout, problem, "no lines" if cand is False else "lines", r)
            g = _handle(loc, val, problem, r, **kw)
            sol = g.solve()
            _same(g, sol, sv.near_tie_want(layout, problem, None if r == sv.NEAR_TIE_STOP else r), what, layout)
            assert g.gpu["tiled_active"] == 0, what
            und = g.gpu["filter_undecided"]
            print(what, "filter_undecided", und, "numpy model of the whole solve", model, "of", scans, "scans in", rounds, "rounds")
            if r == 1:
                assert und == n * 3 // 5, (what, und)
            assert 0 < und, (what, und)
            if r == sv.NEAR_TIE_STOP:
                # a sanity bound only: `scans` is the sum of the bidders of all rounds with K > 2048, which is the number
                # of filter scans without lines and above it with them (a line that hits answers without a scan); what
                # pins the bound is the exact count after round 1
                assert und < scans, (what, und, scans)
                assert g.gpu["grid_rounds"] >= rounds


# ---- the dense entry point -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("problem", sv.PROBLEMS)
def test_dense_cases_through_from_matrix(problem, gpu_lib):
    N, M = ve.DENSE_SHAPE
    for name, c in ve.dense_cases().items():
        stop = sv.ENDS_STOP if c.stop is None else c.stop
        w = ve.dense_want(name, problem)
        mat = c.val.copy()
        g = from_matrix(mat, problem=problem, max_iter=stop, cardinality_check=False, **dict(c.opts))
        sol = g.solve()
        what = "dense %s %s" % (name, problem)
        with np.errstate(invalid="ignore"):
            valid = c.val >= 0
        assert mat.tobytes() == c.val.tobytes(), what  # the caller's matrix is not written
        assert g.nnz == int(valid.sum()) and g.num_rows == N and g.num_cols == w["M"], what
        assert g.gpu["bytes_per_edge"] == sv.layout_of(c.val[valid]), what
        assert np.array_equal(sol, w["sol"]), what
        for k in ("its", "eCE", "soln_found", "n_assigned", "nreductions"):
            assert g.meta[k] == w["meta"][k], (what, k, g.meta[k], w["meta"][k])
        assert _same_float(g.gpu["obj_f64"], w["extra"]["obj_f64"]), what
        for k in ("start_eps_f32", "final_eps_f32"):
            assert _f32_bits(g.gpu[k]) == _f32_bits(w["extra"][k]), (what, k)
        assert np.array_equal(bits(g.prices), bits(w["p"])), what
        assert g.status().error_bits == 0, what


# ---- lockstep ----------------------------------------------------------------------------------------------------------------

LOCKSTEP = ("neg_mixed@70", "above_flt_max", "zeros", "f32_subnormal_exact", "flt_max_f32", "one_not_f32", "ulp_2_53", "eps_1e39")


@pytest.mark.parametrize("problem", sv.PROBLEMS)
def test_lockstep_batch_of_eight_cases(problem, gpu_lib):
    """One solve_batch call: every handle has its own stop, so spinning problems (C = +inf, all zeros, eps = +inf) run beside
    converging ones, and each ends in its own oracle state."""
    cs = [sv.cases()[k] for k in LOCKSTEP]
    assert {c.rows for c in cs} == {ve.ROWS}
    loc = ve.graph(ve.ROWS)[0]
    solvers = [_handle(loc, c.val, problem, c.stop, c.opts) for c in cs]
    sols, info = AuctionSolver.solve_batch(solvers)
    assert info["groups"] >= 1
    for key, c, g, sol in zip(LOCKSTEP, cs, solvers, sols):
        _same(g, sol, sv.want(key, problem), "%s %s in a lockstep batch" % (key, problem), sv.layout_of(c.val))


# ---- warm ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("problem", sv.PROBLEMS)
def test_new_values_on_a_live_handle_move_every_guard(problem, gpu_lib, monkeypatch):
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")  # the handle gets the filter's mirror; whether a solve uses it follows
    loc = ve.graph(ve.BIG_ROWS)[0]                 # the values and starting prices of that solve (filter_undecided == -1: no)
    chain = sv.warm_chain(problem)
    vals = [sv.cases()[k].val for k in sv.WARM_STEPS]
    g = _handle(loc, vals[0], problem, sv.WARM_STOP, force_f64=True, tiled_min_k=-1)
    sol = g.solve()
    _same(g, sol, chain[0], "cold %s" % problem, 12)
    assert g.gpu["filter_undecided"] >= 0 and sv.filter_range_ok(vals[0])
    for k in (1, 2):
        what = "%s: values of %s, resolve from the prices of step %d" % (problem, sv.WARM_STEPS[k], k - 1)
        before = vals[k].copy()
        g.update_values(before)
        assert np.array_equal(bits(before), bits(vals[k])), what  # the caller's values are not written
        sol = g.resolve()
        _same(g, sol, chain[k], what, 12)
        with np.errstate(over="ignore"):
            c32 = np.float32(np.abs(vals[k]).max())
        assert _f32_bits(g.gpu["start_eps_f32"]) == _f32_bits(np.float32(np.float64(c32) / 2.0)), what  # the new C / 2
        _lines(g, chain[k], ve.BIG_ROWS, vals[k], {}, what, chain[k]["pmax0"])
        assert not sv.filter_range_ok(vals[k], chain[k]["pmax0"]) and g.gpu["filter_undecided"] == -1, what
    # ... and back inside the range, from zero prices: the filter serves the solve again
    g.update_values(vals[0].copy())
    sol = g.resolve(prices=np.zeros(g.num_cols))
    _same(g, sol, chain[0], "%s: the first values again, from zero prices" % problem, 12)
    assert g.gpu["filter_undecided"] >= 0


@pytest.mark.parametrize("problem", sv.PROBLEMS)
def test_an_inexact_value_is_refused_by_an_8_byte_handle(problem, gpu_lib):
    """update_values of the one_not_f32 values on the 8 B/edge handle of its twin: refused, the handle unchanged -- its
    solve equals that of a handle that never saw the update."""
    a, b = sv.cases()["all_f32"], sv.cases()["one_not_f32"]
    loc = ve.graph(ve.ROWS)[0]
    g, twin = _handle(loc, a.val, problem, a.stop), _handle(loc, a.val, problem, a.stop)
    with pytest.raises(ValueError):
        g.update_values(b.val.copy())
    sg, st = g.solve(), twin.solve()
    w = sv.want("all_f32", problem)
    _same(g, sg, w, "after the refused update", 8)
    _same(twin, st, w, "twin", 8)
    for k, v in twin.state().items():
        assert np.array_equal(np.asarray(g.state()[k]), np.asarray(v)), k
    # ... and after a solve: refused again, and the warm resolve equals the twin's
    with pytest.raises(ValueError):
        g.update_values(b.val.copy())
    sg, st = g.resolve(), twin.resolve()
    assert np.array_equal(sg, st) and np.array_equal(bits(g.prices), bits(twin.prices))
    assert g.meta["its"] == twin.meta["its"] and g.gpu["bytes_per_edge"] == twin.gpu["bytes_per_edge"] == 8
