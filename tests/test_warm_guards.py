"""Warm re-solves (misslap_resolve / misslap_update_values / misslap_update_dense) against the oracle
where starting prices and new values move the guards: lines_safe_eps = (C + P0) x 2^-44 driven by P0 and by a new C, the
fp32 filter under prices far above the costs and on both sides of set_filter's 2^60 and 2^-100, the edges of what
k_check_prices accepts, and value updates on the tile-major layouts the older cases miss (overflow lists that are known to
be non-empty, 8 and 16 lanes per person, the column split, T = 3 with empty segments, repeated columns, long rows, fewer
rows than a layout block, dense handles at the edges of the gather, two updates in a row).

Everything bit for bit against the oracle started from the same prices; inputs, starting prices and the oracle's runs
come from tests/_warm_cases.py (pinned without a GPU by tests/test_warm_guards_nogpu.py).  A whole solve is one the oracle
ends within ROUNDS_FACTOR x its cold rounds; every other solve carries max_iter <= 160 and its state after that round is
compared.  Which side of set_filter a solve took is not observable through the API: parity is asserted on both sides."""
import numpy as np
import pytest

import _warm_cases as wc
from sslap_amd import from_matrix, from_sparse

pytestmark = pytest.mark.gpu

WAVE = dict(tiled_min_k=-1)
TILED = dict(tiled_min_k=1, engine=1)


def _solver(name, vals, prob, max_iter, **kw):
    loc, _ = wc.inputs(name)
    return from_sparse(loc, wc.values(name, vals).copy(), problem=prob, max_iter=max_iter, cardinality_check=False, **kw)


def _zeros(g):
    return np.zeros(g.num_cols)


def _lines(g):
    return g.gpu["phases_with_lines"], g.gpu["eps_phases"], g.gpu["lines_active"]


# ---- A. starting prices that move the guards ----------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [None, 0])
@pytest.mark.parametrize("engine", ["wave", "tiled"])
@pytest.mark.parametrize("prob", wc.PROBLEMS)
def test_lines_guard_driven_by_the_starting_prices(prob, engine, thr, gpu_lib):
    """A1.  Converged prices (and half of them) plus a uniform shift S: the same equilibrium under other rounding.  The
    lines serve exactly the phases whose eps is >= (C + max P0) x 2^-44, computed here from the oracle's eps schedule:
    all 7 up to S = 2^33, 6 at 2^34, 5 at 2^36, 4 at 2^40.  A resolve from zeros on the same handle is again the cold
    solve with every phase on lines: the bound went back down."""
    g = _solver("g800", "A", prob, wc.max_rounds("g800", prob), tail_threshold=thr, **(WAVE if engine == "wave" else TILED))
    cold = wc.want("g800", prob, "A", "zero", None)
    seen = set()
    for st in wc.GUARD_STARTS:
        what = "%s %s thr=%s start=%s + 2^%d" % (prob, engine, thr, st[0], int(np.log2(st[1])))
        sol = g.resolve(prices=wc.start("g800", prob, st))
        wc.same_result(g, sol, wc.want("g800", prob, "A", st, None), what)
        expect = wc.lines_expected("g800", prob, "A", st)
        assert _lines(g) == expect, (what, _lines(g), expect)
        assert g.gpu["tiled_active"] == (engine == "tiled"), what
        seen.add(expect[0] == expect[1])
        sol = g.resolve(prices=_zeros(g))
        wc.same_result(g, sol, cold, what + ", then from zeros")
        assert _lines(g) == (cold["meta"]["nreductions"] + 1,) * 2 + (1,), (what, _lines(g))
    assert seen == {True, False}  # both sides of the bound


@pytest.mark.parametrize("cand", [True, False])
@pytest.mark.parametrize("name", wc.FILTER_INPUTS)
def test_f32_filter_under_prices_far_above_the_costs(name, cand, gpu_lib, monkeypatch):
    """A2.  wave_bid_filter with pmax >> cmax from round 1 (two_delta = 2^-21 (cmax + pmax) exceeds every gap of a row, so
    every row must fall through to the exact scan): the state after r rounds, and one whole solve."""
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")
    prob = wc.PROBLEM[name]
    kw = dict(tail_threshold=0, cand=cand, **WAVE)
    for s in wc.FILTER_SHIFTS:
        p0 = wc.start(name, prob, ("cold", s))
        for r in wc.FILTER_ROUNDS:
            g = _solver(name, "A", prob, r, **kw)
            g.resolve(prices=p0)
            assert g.gpu["tiled_active"] == 0 and g.gpu["bytes_per_edge"] == (12 if name == "f_f64" else 8)
            wc.same_state(g, wc.want(name, prob, "A", ("cold", s), r), "%s cand=%s shift 2^%d r=%d" % (name, cand, int(np.log2(s)), r))
    st = ("cold", wc.FILTER_SHIFTS[0])
    g = _solver(name, "A", prob, wc.max_rounds(name, prob), **kw)
    sol = g.resolve(prices=wc.start(name, prob, st))
    wc.same_result(g, sol, wc.want(name, prob, "A", st, None), "%s cand=%s whole solve" % (name, cand))


@pytest.mark.parametrize("name", wc.FILTER_INPUTS)
def test_starting_prices_on_both_sides_of_two_to_the_sixty(name, gpu_lib, monkeypatch):
    """A3.  Largest starting price = the last double below 2^60 (the filter's bound holds), 2^60 and 2^62 (it does not: the
    exact scan): all accepted, state after r rounds (these solves do not end, so they are always capped)."""
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")
    prob = wc.PROBLEM[name]
    for p in wc.TOP_PRICES:
        p0 = wc.start(name, prob, ("top", p))
        for r in wc.TOP_ROUNDS:
            g = _solver(name, "A", prob, r, tail_threshold=0, **WAVE)
            g.resolve(prices=p0)
            wc.same_state(g, wc.want(name, prob, "A", ("top", p), r), "%s P0=%r r=%d" % (name, p, r))


@pytest.mark.parametrize("engine", ["wave", "tiled"])
@pytest.mark.parametrize("prob", wc.PROBLEMS)
def test_accepted_edge_prices_and_rejected_ones(prob, engine, gpu_lib):
    """A4.  +0.0 everywhere but a subnormal, the smallest normal and, at an object no row lists, the largest finite double:
    accepted, solved like the cold solve, and with P0 ~ 1.8e308 no phase runs on lines.  A rejected vector (NaN, inf,
    negative, -0.0) leaves the handle equal to a twin that never saw it."""
    kw = WAVE if engine == "wave" else TILED
    g, twin = (_solver("rect", "A", prob, wc.max_rounds("rect", prob), **kw) for _ in range(2))
    p0 = wc.start("rect", prob, "edge")
    w = wc.want("rect", prob, "A", "edge", None)
    sol = g.resolve(prices=p0)
    wc.same_result(g, sol, w, "edge prices")
    assert _lines(g) == wc.lines_expected("rect", prob, "A", "edge") == (0, w["meta"]["nreductions"] + 1, 0)
    sol_t = twin.resolve(prices=p0)
    for bad in (np.nan, np.inf, -1.0, -0.0):
        p = p0.copy()
        p[7] = bad
        with pytest.raises(ValueError):
            g.resolve(prices=p)
    wc.same_handles(g, sol, twin, sol_t, "after the rejected vectors")
    assert np.array_equal(wc.bits(g.state()["p"]), wc.bits(twin.state()["p"])) and g.state()["its"] == twin.state()["its"]
    sol, sol_t = g.resolve(prices=p0), twin.resolve(prices=p0)
    wc.same_handles(g, sol, twin, sol_t, "a resolve after the rejected vectors")
    wc.same_result(g, sol, w, "and the oracle")


# ---- B. updates that change the cost range --------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(wc.RANGE_CONFIGS))
@pytest.mark.parametrize("prob", wc.PROBLEMS)
def test_update_raises_the_cost_range_and_lowers_it_again(prob, config, gpu_lib):
    """B5 / B6.  Values <= 100 replaced by float32(1e10) + 1024 v: eps0 = C / 2 of the NEW values, 17 phases of which the
    last is below the new bound (16 on lines), on a handle nothing has run on (solve) and on a used one (resolve from
    zeros); then back to the old values: the cold solve again, every phase on lines."""
    kw, big = wc.RANGE_CONFIGS[config]
    A, B = wc.values("g800", "A"), wc.values("g800", big)
    delta = float(np.abs(B - A).max())
    cold, w = wc.want("g800", prob, "A", "zero", None), wc.want("g800", prob, big, "zero", None)
    expect = wc.lines_expected("g800", prob, big, "zero")
    assert 0 < expect[0] < expect[1]
    fresh_h = _solver("g800", "A", prob, wc.max_rounds("g800", prob), **kw)
    assert fresh_h.update_values(B.copy()) == delta
    sol = fresh_h.solve()
    wc.same_result(fresh_h, sol, w, "update on an untouched handle, solve")
    assert _lines(fresh_h) == expect and fresh_h.gpu["start_eps_f32"] == w["extra"]["start_eps_f32"] > 1e9
    used = _solver("g800", "A", prob, wc.max_rounds("g800", prob), **kw)
    wc.same_result(used, used.solve(), cold, "cold")
    assert used.update_values(B.copy()) == delta
    sol = used.resolve(prices=_zeros(used))
    wc.same_result(used, sol, w, "update on a used handle, resolve from zeros")
    assert _lines(used) == expect
    if "engine" in kw:
        assert used.gpu["tiled_active"] == 1 and used.gpu["tiled_format"] == int(bool(kw.get("force_f64")))
    # B6
    assert used.update_values(A.copy()) == delta
    sol = used.resolve(prices=_zeros(used))
    wc.same_result(used, sol, cold, "back to the old values")
    assert _lines(used) == (cold["meta"]["nreductions"] + 1,) * 2 + (1,)
    twin = _solver("g800", "A", prob, wc.max_rounds("g800", prob), **kw)
    wc.same_handles(used, sol, twin, twin.solve(), "a fresh handle's cold solve")


@pytest.mark.parametrize("config", list(wc.TINY_CONFIGS))
@pytest.mark.parametrize("prob", wc.PROBLEMS)
def test_update_to_a_range_below_the_filters(prob, config, gpu_lib, monkeypatch):
    """B7.  New values v x 2^-110: max |v| below set_filter's 2^-100, filter forced.  eps0 = C / 2 is below 1 / N, so the
    oracle runs one phase and ends (69 / 80 rounds)."""
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")
    kw = dict(wc.TINY_CONFIGS[config], tail_threshold=0)
    A, B = wc.values("g800", "A"), wc.values("g800", "tiny")
    w = wc.want("g800", prob, "tiny", "zero", None)
    fresh_h = _solver("g800", "A", prob, wc.max_rounds("g800", prob), **kw)
    assert fresh_h.update_values(B.copy()) == float(np.abs(B - A).max())
    wc.same_result(fresh_h, fresh_h.solve(), w, "untouched handle")
    assert fresh_h.gpu["bytes_per_edge"] == 12
    used = _solver("g800", "A", prob, wc.max_rounds("g800", prob), **kw)
    cold = wc.want("g800", prob, "A", "zero", None)
    wc.same_result(used, used.solve(), cold, "cold")
    used.update_values(B.copy())
    wc.same_result(used, used.resolve(prices=_zeros(used)), w, "used handle, from zeros")
    assert _lines(used) == wc.lines_expected("g800", prob, "tiny", "zero")
    used.update_values(A.copy())
    wc.same_result(used, used.resolve(prices=_zeros(used)), cold, "back to the old values")


# ---- C. updates on the layouts ----------------------------------------------------------------------------------------------
def _update_flow(name, prob, kw, fmt=None, thr_capped=0):
    """Old values -> the same values rotated by one place within every row (every edge changes, C stays), then a warm
    resolve from the old prices: stopped after r rounds on a handle nothing has run on, whole on a handle that has
    solved the old values, and equal to a fresh handle on the new values."""
    A, B = wc.values(name, "A"), wc.values(name, "rot")
    delta = float(np.abs(B - A).max())
    pA = wc.start(name, prob, "old")

    def check(g):
        if "engine" in kw:
            assert g.gpu["tiled_active"] == 1
            if fmt is not None:
                assert g.gpu["tiled_format"] == fmt
    for r in wc.UPDATE_ROUNDS:
        g = _solver(name, "A", prob, r, tail_threshold=thr_capped, **kw)
        assert g.update_values(B.copy()) == delta
        g.resolve(prices=pA)
        wc.same_state(g, wc.want(name, prob, "rot", "old", r), "%s %s %s r=%d" % (name, prob, kw, r))
        check(g)
    g = _solver(name, "A", prob, wc.max_rounds(name, prob), **kw)
    wc.same_result(g, g.solve(), wc.want(name, prob, "A", "zero", None), "cold")
    assert g.update_values(B.copy()) == delta
    sol = g.resolve(prices=pA)
    wc.same_result(g, sol, wc.want(name, prob, "rot", "old", None), "%s %s %s whole" % (name, prob, kw))
    check(g)
    fresh_h = _solver(name, "rot", prob, wc.max_rounds(name, prob), **kw)
    wc.same_handles(g, sol, fresh_h, fresh_h.resolve(prices=pA), "fresh handle on the new values")


@pytest.mark.parametrize("inp", wc.LAYOUT_INPUTS)
@pytest.mark.parametrize("shape,fmt", wc.LAYOUT_SHAPES)
def test_update_on_every_launch_shape_and_record_format(shape, fmt, inp, gpu_lib):
    """C8 / C9.  4, 8 and 16 lanes per person (overflow caps 16, 32, 64) and the column split, record formats 0..3, T = 3
    tiles with empty segments: `mid` puts edges on the overflow lists at every cap (k_ovf_revalue on non-empty lists),
    `short` none at any."""
    name, prob = wc.layout_case(inp, fmt)
    over = wc.overflow_edges(wc.inputs(name)[0], shape)
    assert over > 0 if inp == "mid" else over == 0
    _update_flow(name, prob, dict(TILED, tiled_shape=shape, force_f64=bool(fmt & 1)), fmt)


@pytest.mark.parametrize("shape", [0, 8])
@pytest.mark.parametrize("f64", [False, True])
def test_update_on_rows_with_repeated_columns(f64, shape, gpu_lib):
    """C10.  Entries stored twice under one column with different values, fp32 and force_f64.  The ingest sends such
    rows to the stored-index formats (2 / 3), as test_repeated_entries_on_the_engine_round_by_round pins, so the
    rewritten value must come from the stored index and not from a search by column.  The oracle does not end these
    inputs with soln_found, so every solve here is capped."""
    kw = dict(TILED, tiled_shape=shape, force_f64=f64, tail_threshold=0)
    over = wc.overflow_edges(wc.inputs("dups")[0], shape)
    assert over > 0 if shape == 0 else over == 0
    A, B = wc.values("dups", "A"), wc.values("dups", "rot")
    delta = float(np.abs(B - A).max())
    pA = wc.start("dups", "max", "old")
    for r in wc.DUPS_ROUNDS:
        g = _solver("dups", "A", "max", r, **kw)
        if r == wc.ROUND_CAP:  # a used handle
            g.solve()
            wc.same_state(g, wc.want("dups", "max", "A", "zero", r), "cold, r=%d" % r)
        assert g.update_values(B.copy()) == delta
        g.resolve(prices=pA)
        wc.same_state(g, wc.want("dups", "max", "rot", "old", r), "f64=%s shape=%d r=%d" % (f64, shape, r))
        assert g.gpu["tiled_active"] == 1 and g.gpu["tiled_format"] == (3 if f64 else 2)
    fresh_h = _solver("dups", "rot", "max", wc.ROUND_CAP, **kw)
    fresh_h.resolve(prices=pA)
    wc.same_state(fresh_h, wc.want("dups", "max", "rot", "old", wc.ROUND_CAP), "fresh handle")
    assert np.array_equal(wc.bits(fresh_h.state()["p"]), wc.bits(g.state()["p"]))


@pytest.mark.parametrize("engine", ["wave", "tiled"])
def test_update_on_rows_of_600_edges(engine, gpu_lib):
    """C11.  cases.LONG_CASES['dense600_max_mat'] as loc / val: the engine's long-segment loop with nearly every edge on an
    overflow list, and the wave-per-row kernel with the lines of long rows."""
    assert wc.overflow_edges(wc.inputs("long")[0], 0) > 0
    if engine == "tiled":
        _update_flow("long", "max", dict(TILED))
    else:
        _update_flow("long", "max", dict(WAVE), thr_capped=None)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("prob", wc.PROBLEMS)
@pytest.mark.parametrize("name", wc.SMALL_N)
def test_update_with_fewer_rows_than_a_layout_block(name, prob, f64, gpu_lib):
    """C12.  100 rows (one partial layout block of 128) and 129 (a full one and one row of the next)."""
    _update_flow(name, prob, dict(TILED, force_f64=f64), int(f64))


@pytest.mark.parametrize("prob", wc.PROBLEMS)
@pytest.mark.parametrize("name", wc.DENSE_PARITY)
def test_dense_handle_update_at_the_edges_of_the_gather(name, prob, gpu_lib):
    """C13.  from_matrix + update_values / update_values_device(dense=True): 1 x 1, 3 x 64, 5 x 65, 130 x 191 and
    257 x 1000 with rows of one entry between rows of 1000.  Pattern kept, values rotated within every row."""
    import torch
    A, B = wc.dense_values(name, "A"), wc.dense_values(name, "rot")
    delta = float(np.abs(wc.values(name, "rot") - wc.values(name, "A")).max())
    cap = wc.max_rounds(name, prob)
    h, d = (from_matrix(A.copy(), problem=prob, max_iter=cap, cardinality_check=False) for _ in range(2))
    wc.same_result(h, h.solve(), wc.want(name, prob, "A", "zero", None), "cold")
    assert h.update_values(B.copy()) == delta
    tB = torch.tensor(B, device="cuda")
    torch.cuda.synchronize()
    assert d.update_values_device(tB.data_ptr(), dense=True) == delta  # (on a handle nothing has run on)
    w = wc.want(name, prob, "rot", "zero", None)
    sol_h, sol_d = h.resolve(prices=_zeros(h)), d.solve()
    wc.same_result(h, sol_h, w, "host matrix")
    wc.same_result(d, sol_d, w, "device matrix")
    wc.same_handles(h, sol_h, d, sol_d, "host and device variants")


def test_dense_handle_update_with_more_persons_than_objects(gpu_lib):
    """C13, 130 x 63.  No oracle here: with more persons than objects the reference's push_all_left writes out of bounds
    from the first round on (its bound is num_cols), so there is nothing to compare with.  What is defined is checked
    between handles after a few rounds: an updated handle against a fresh one on the new values, host against device."""
    import torch
    A, B = wc.dense_values("d130x63", "A"), wc.dense_values("d130x63", "rot")
    delta = float(np.abs(wc.values("d130x63", "rot") - wc.values("d130x63", "A")).max())
    h, d, fresh_h = (from_matrix(m.copy(), max_iter=wc.UNCOMPARED_ROUNDS, cardinality_check=False) for m in (A, A, B))
    assert h.update_values(B.copy()) == delta
    tB = torch.tensor(B, device="cuda")
    torch.cuda.synchronize()
    assert d.update_values_device(tB.data_ptr(), dense=True) == delta
    states = []
    for g in (h, d, fresh_h):
        g.solve()
        states.append(g.state())
        assert g.status().error_bits == 0
    for s in states[:2]:
        assert s["its"] == states[2]["its"] == wc.UNCOMPARED_ROUNDS and s["K"] == states[2]["K"]
        assert np.array_equal(s["U"], states[2]["U"]) and np.array_equal(wc.bits(s["p"]), wc.bits(states[2]["p"]))
        assert np.array_equal(s["p2o"], states[2]["p2o"]) and np.array_equal(s["o2p"], states[2]["o2p"])


def test_dense_pattern_changes_that_keep_the_count_or_sit_in_the_last_cell(gpu_lib):
    """C13.  A swap inside one row (one entry leaves, one arrives: the count stays) and a change in the last row's last
    column are both refused, and the handle then equals a twin that never saw them."""
    D = wc.dense_values("d130x191", "A")
    g, twin = (from_matrix(D.copy(), max_iter=wc.max_rounds("d130x191", "min"), cardinality_check=False) for _ in range(2))
    swap = D.copy()
    row = 77
    gone, new = np.flatnonzero(D[row] >= 0)[5], np.flatnonzero(D[row] < 0)[2]
    swap[row, new], swap[row, gone] = D[row, gone], -1.0
    assert ((swap >= 0).sum(axis=1) == (D >= 0).sum(axis=1)).all()
    last = D.copy()
    last[-1, -1] = -1.0 if D[-1, -1] >= 0 else 1.0
    for bad in (swap, last):
        with pytest.raises(ValueError, match="pattern"):
            g.update_values(bad)
    wc.same_handles(g, g.solve(), twin, twin.solve(), "after the refused updates")
    wc.same_result(g, g.resolve(prices=_zeros(g)), wc.want("d130x191", "min", "A", "zero", None), "and the oracle")


@pytest.mark.parametrize("name,prob,shape,fmt", [("mid", "max", 8, 0), ("mid_sh", "min", 9, 3)])
def test_two_updates_in_a_row(name, prob, shape, fmt, gpu_lib):
    """C14.  A -> B -> A' without a solve between: a fresh handle on A' (and the oracle), cold on a handle nothing has run
    on, warm from the old prices on a used one."""
    kw = dict(TILED, tiled_shape=shape, force_f64=bool(fmt & 1))
    A, B, A2 = (wc.values(name, v) for v in ("A", "rot", "rot2"))
    cap = wc.max_rounds(name, prob)
    g, used = _solver(name, "A", prob, cap, **kw), _solver(name, "A", prob, cap, **kw)
    used.solve()
    for h in (g, used):
        assert h.update_values(B.copy()) == float(np.abs(B - A).max())
        assert h.update_values(A2.copy()) == float(np.abs(A2 - B).max())
    sol = g.solve()
    wc.same_result(g, sol, wc.want(name, prob, "rot2", "zero", None), "untouched")
    fresh_h = _solver(name, "rot2", prob, cap, **kw)
    wc.same_handles(g, sol, fresh_h, fresh_h.solve(), "fresh handle on A'")
    pA = wc.start(name, prob, "old")
    sol = used.resolve(prices=pA)
    wc.same_result(used, sol, wc.want(name, prob, "rot2", "old", None), "used")
    wc.same_handles(used, sol, fresh_h, fresh_h.resolve(prices=pA), "fresh handle on A', warm")
    assert used.gpu["tiled_active"] == 1 and used.gpu["tiled_format"] == fmt
