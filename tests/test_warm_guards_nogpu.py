"""What tests/test_warm_guards.py rests on, pinned without a GPU: every whole solve it runs ends on the oracle within the
bound, every other solve is capped, the guard positions it asserts really change sides, the overflow lists are empty or
not as each case says, a rotated value set moves every edge, and the oracle's results follow from the seeds alone."""
import hashlib

import numpy as np

import _warm_cases as wc


def test_every_whole_solve_ends_with_soln_found_within_twenty_times_the_cold_rounds():
    """ROUNDS_FACTOR is a cap against price wars, not a measurement: the largest ratio among these runs is printed."""
    runs = wc.whole_runs()
    assert len(set(runs)) == len(runs)
    worst = 0.0
    for name, prob, vals, st in runs:
        w = wc.want(name, prob, vals, st, None)
        cold = wc.want(name, prob, "A", "zero", None)["meta"]["its"]
        assert w["meta"]["soln_found"] == 1, (name, prob, vals, st)
        assert w["meta"]["its"] <= wc.ROUNDS_FACTOR * cold and w["meta"]["its"] < w["max_iter"], (name, prob, vals, st)
        worst = max(worst, w["meta"]["its"] / cold)
    print("whole solves: %d, largest rounds / cold rounds: %.2f" % (len(runs), worst))
    assert worst < wc.ROUNDS_FACTOR


def test_every_other_solve_is_capped():
    """The capped runs, listed: none of them is given more than ROUND_CAP rounds, and the oracle stops where it is told
    (or earlier, where the solve ends inside the cap)."""
    runs = wc.capped_runs()
    assert len(set(runs)) == len(runs)
    for name, prob, vals, st, cap in runs:
        assert cap <= wc.ROUND_CAP == 160
        w = wc.want(name, prob, vals, st, cap)
        assert w["max_iter"] == cap and w["state"]["its"] <= cap, (name, prob, vals, st, cap)
    # the runs that are capped because they do not end: the 2^60 prices and the repeated-entry input
    for name in wc.FILTER_INPUTS:
        for p in wc.TOP_PRICES:
            w = wc.want(name, wc.PROBLEM[name], "A", ("top", p), max(wc.TOP_ROUNDS))
            assert w["state"]["its"] == max(wc.TOP_ROUNDS) and w["state"]["K"] > 0
    w = wc.want("dups", "max", "rot", "old", wc.ROUND_CAP)
    assert w["state"]["its"] == wc.ROUND_CAP and w["state"]["K"] > 0
    assert "d130x63" in wc.NEVER_ENDS and wc.UNCOMPARED_ROUNDS <= wc.ROUND_CAP


def test_the_measured_shifts_of_the_800_row_input():
    """The figures the cases were chosen by: cold 2315 rounds and 6 reductions, final price max 203.9, C = 99.995;
    cold prices + 2^20 and + 2^33: 2689 rounds, 6 reductions, final eps 5.695e-4."""
    cold = wc.want("g800", "max", "A", "zero", None)
    assert (cold["meta"]["its"], cold["meta"]["nreductions"]) == (2315, 6)
    assert round(float(cold["p"].max()), 1) == 203.9 and round(float(wc.values("g800", "A").max()), 3) == 99.995
    a, b = (wc.want("g800", "max", "A", ("cold", 2.0 ** e), None) for e in (20, 33))
    assert (a["meta"]["its"], a["meta"]["nreductions"]) == (b["meta"]["its"], b["meta"]["nreductions"]) == (2689, 6)
    assert abs(a["extra"]["final_eps_f32"] - 5.695e-4) < 1e-7
    assert np.array_equal(a["sol"], b["sol"])


def test_guard_positions_straddle():
    """A1: (C + P0) x 2^-44 against the seven eps of the schedule, 49.998 x 0.15^k = ..., 3.797e-3, 5.695e-4.
    P0 ~ 2^33: bound 4.88e-4, below the last eps: 7 of 7 phases on lines.  2^34: 9.77e-4: 6 of 7.  2^36: 3.9e-3: 5 of 7.
    2^40: 6.25e-2: 4 of 7.  B5: C = 1.00001e10: bound 5.68e-4 against 17 eps down to 1.6e-4 (5.0e9 x 0.15^16): 16 of 17."""
    for prob in wc.PROBLEMS:
        for base in ("cold", "half"):
            got = {e: wc.lines_expected("g800", prob, "A", (base, 2.0 ** e)) for e in (20, 33, 34, 36, 40)}
            assert got == {20: (7, 7, 1), 33: (7, 7, 1), 34: (6, 7, 0), 36: (5, 7, 0), 40: (4, 7, 0)}, (prob, base, got)
        bound33, bound34 = (wc.lines_bound("g800", prob, "A", ("cold", 2.0 ** e)) for e in (33, 34))
        last = float(wc.eps_schedule(wc.want("g800", prob, "A", ("cold", 2.0 ** 33), None), 800)[-1])
        assert bound33 < last < bound34 and abs(bound33 - 4.88e-4) < 1e-6 and abs(last - 5.695e-4) < 1e-7
        assert wc.lines_expected("g800", prob, "A", "zero") == (7, 7, 1)
        for vals in ("big32", "big64"):
            assert wc.lines_expected("g800", prob, vals, "zero") == (16, 17, 0), (prob, vals)
            w = wc.want("g800", prob, vals, "zero", None)
            assert w["extra"]["start_eps_f32"] == float(np.float32(np.float32(np.abs(wc.values("g800", vals)).max()) / 2.0))
        # B7: eps0 = C / 2 = 3.85e-32 is below 1 / N: one phase, far above the bound of 4.4e-45
        assert wc.lines_expected("g800", prob, "tiny", "zero") == (1, 1, 1)
        assert float(np.abs(wc.values("g800", "tiny")).max()) < 2.0 ** -100
        # A4: the largest finite double as P0: the bound is ~1e295 and no phase runs on lines
        assert wc.lines_expected("rect", prob, "A", "edge") == (0, 7, 0)


def test_starting_prices_are_what_the_cases_say():
    for name in wc.FILTER_INPUTS:
        prob = wc.PROBLEM[name]
        cold = wc.want(name, prob, "A", "zero", None)["p"]
        assert cold.max() < 256.0  # below the ulp at 2^60: the shifted vector is flat there (a uniform shift all the same)
        for p in wc.TOP_PRICES:
            p0 = wc.start(name, prob, ("top", p))
            assert p0.max() == p and p0.min() >= p - 256.0
        assert wc.TOP_PRICES[0] < 2.0 ** 60 == wc.TOP_PRICES[1] < wc.TOP_PRICES[2]
        for s in wc.FILTER_SHIFTS:  # prices far above the costs: P0 / C >= 2^13
            assert wc.start(name, prob, ("cold", s)).min() >= s > 2.0 ** 13 * np.abs(wc.values(name, "A")).max()
    loc, _ = wc.inputs("rect")
    n, m = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    assert m > n
    for prob in wc.PROBLEMS:
        p0 = wc.start("rect", prob, "edge")
        nz = np.flatnonzero(p0)
        assert sorted(p0[nz].tolist()) == sorted(wc.EDGE_PRICES) and not np.signbit(p0).any() and np.isfinite(p0).all()
        huge = int(np.argmax(p0))
        assert p0[huge] == np.finfo(np.float64).max and huge not in set(loc[:, 1].tolist())
        assert all(int(j) in set(loc[:, 1].tolist()) for j in nz if j != huge)  # the two small ones are read by bids
        assert wc.want("rect", prob, "A", "edge", None)["p"][huge] == p0[huge]


def test_overflow_counts_have_the_asserted_sign():
    """Edges beyond the cap (16 / 32 / 64 for tiled_shape 0 and 4 / 8 / 9) of their (row, tile) segment, from loc alone."""
    for name in ("mid", "mid_sh"):
        loc, _ = wc.inputs(name)
        cnt, empty, T = wc.segment_counts(loc)
        rows = np.bincount(loc[:, 0])
        assert T == 3 and empty > 0 and 20 <= rows.min() and rows.max() <= 200
        assert wc.overflow_edges(loc, 0) == wc.overflow_edges(loc, 4) > wc.overflow_edges(loc, 8) > wc.overflow_edges(loc, 9) > 0
    for name in ("short", "short_sh"):
        loc, _ = wc.inputs(name)
        assert wc.segment_counts(loc)[2] == 3 and np.bincount(loc[:, 0]).max() <= 16
        assert all(wc.overflow_edges(loc, s) == 0 for s in wc.OVF_CAP)
    loc, _ = wc.inputs("dups")
    key = loc[:, 0].astype(np.int64) << 32 | loc[:, 1]
    assert (key[1:] == key[:-1]).sum() > 1000 and (key[1:] >= key[:-1]).all()  # repeated columns, ascending
    assert wc.overflow_edges(loc, 0) > 0 and wc.overflow_edges(loc, 8) == 0
    loc, _ = wc.inputs("long")
    assert np.bincount(loc[:, 0]).min() >= 600 and all(wc.overflow_edges(loc, s) > 0 for s in (0, 8, 9))
    for name, n in (("n100", 100), ("n129", 129)):
        loc, _ = wc.inputs(name)
        assert int(loc[:, 0].max()) + 1 == n and wc.overflow_edges(loc, 0) == 0


def test_rotated_values_differ_at_every_edge():
    names = [n for n in wc.INPUTS if n not in wc.FILTER_INPUTS + ("g800", "rect")]
    assert len(names) == 14
    for name in names:
        loc, val = wc.inputs(name)
        rot, rot2 = wc.values(name, "rot"), wc.values(name, "rot2")
        assert (rot != val).all() and (rot2 != rot).all() and (rot2 != val).all(), name
        if name not in wc.DENSE_SHAPES:  # the same values per row, so the same C
            order = np.lexsort((val, loc[:, 0])), np.lexsort((rot, loc[:, 0]))
            assert np.array_equal(val[order[0]], rot[order[1]]), name
        assert np.array_equal(rot.astype(np.float32).astype(np.float64), rot)  # fp32-exact: every layout takes them
    loc, val = wc.inputs("dups")
    same_col = np.flatnonzero((loc[1:, 0] == loc[:-1, 0]) & (loc[1:, 1] == loc[:-1, 1]))
    assert (val[same_col] != val[same_col + 1]).all()  # different values under one column
    for d in wc.DENSE_SHAPES:  # the pattern is kept
        assert np.array_equal(wc.dense_values(d, "rot") >= 0, wc.dense_matrix(d) >= 0)
        assert np.array_equal(wc.dense_values(d, "A"), wc.dense_matrix(d))
    one = wc.dense_matrix("d257x1000")
    assert set((one >= 0).sum(axis=1).tolist()) == {1, 1000}


def _digest(w):
    h = hashlib.sha256()
    for a in (w["sol"], w["p"], w["state"]["U"], w["state"]["p2o"], w["state"]["o2p"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(repr(sorted((k, v) for k, v in w["meta"].items() if k != "timer")).encode())
    h.update(repr((w["extra"]["obj_f64"], w["extra"]["edges_scanned"], w["extra"]["final_eps_f32"])).encode())
    return h.hexdigest()


def test_oracle_results_are_reproducible_from_the_seed():
    """A second computation that shares nothing with the cached one (inputs, values, starting prices and the oracle run
    all made again) gives the same bits."""
    picks = [("g800", "max", "A", ("cold", 2.0 ** 34), None), ("g800", "min", "big32", "zero", None),
             ("f_f64", "min", "A", ("cold", 2.0 ** 30), 70), ("f_plain", "max", "A", ("top", 2.0 ** 60), 20),
             ("mid_sh", "min", "rot", "old", None), ("dups", "max", "rot", "old", 160), ("rect", "min", "A", "edge", None),
             ("d257x1000", "max", "rot", "zero", None)]
    first = [_digest(wc.want(*k)) for k in picks]
    for f in (wc.inputs, wc.values, wc.start, wc.want):
        f.cache_clear()
    assert [_digest(wc.want(*k)) for k in picks] == first
    assert wc.inputs("mid")[0].shape == (167646, 2) and wc.inputs("short")[0].shape == (15503, 2)
