"""The cases of tests/_value_edges.py on the CPU: the oracle alone.  Every case must reach the edge it is named for --
otherwise test_batch_value_edges.py, which only compares the library with the oracle, would pass without the batch loop
ever seeing that edge -- and every oracle solve must end within its stop, so that no workgroup is sent into a solve that
only the default max_iter would end.

What the oracle (oracle/auction_oracle.c, pinned to the reference by tests/golden) does at the float32 limits:
  a value above FLT_MAX      C, eps, every bid and every price of a column that was bid for are +inf; only max_iter ends it
  every value below 2^-150   C == 0 and eps == 0: bids equal to the price; distinct values may still end, zeros never do
  eps_start = 1e-46          narrows to 0.0f and means "default": eps = C / 2
  eps_start = 1e-45          the smallest float32 subnormal; it holds, the solve is one phase
  eps_start = 1e39           +inf
"""
import numpy as np
import pytest

from sslap_amd import dense_to_augmented, ell_to_packed, sparse_to_augmented
from tests import _sparse_outside_fixture as sof
from tests import _value_edges as ve
from tests._batch_shapes import META_KEYS, bits

F32_TINY = float(np.finfo(np.float32).tiny)  # the smallest normal float32
ALL_SPARSE = ve.SIGN_NAMES + tuple(n for n, _, _ in ve.MAGNITUDES + ve.EPS_STARTS)
ALL_DENSE = tuple(n for n, _, _ in ve.MAGNITUDES + ve.EPS_STARTS)


def _f32(x):
    return np.float32(x)


def test_no_case_is_left_out():
    assert tuple(ve.sparse_cases()) == ALL_SPARSE and len(set(ALL_SPARSE)) == 19
    assert tuple(ve.dense_cases()) == ALL_DENSE and len(ALL_DENSE) == 14
    assert {c.rows for c in ve.sparse_cases().values() if c.name in ve.BIG} == {ve.BIG_ROWS}
    assert {c.rows for c in ve.sparse_cases().values() if c.name not in ve.BIG} == {ve.ROWS}
    for rows in (ve.ROWS, ve.BIG_ROWS):
        loc = ve.graph(rows)[0]
        assert loc.shape == (rows * ve.PER_ROW, 2) and np.unique(loc, axis=0).shape[0] == loc.shape[0]
    # the cases that have no float32 are exactly those with a value above FLT_MAX
    assert {n for n, c in ve.sparse_cases().items() if not ve.has_f32(c)} == {"above_flt_max", "dbl_max"}
    assert {n for n, c in ve.dense_cases().items() if ve.dense_rounded_f32(c.val) is None} == {"above_flt_max", "dbl_max"}
    # every stop is explicit and small; None is left to the cases that the test below holds to fewer than 1000 rounds
    assert set(ve.STOPPED) == {"above_flt_max", "dbl_max", "flt_max_exact", "c_is_zero", "zeros", "round_to_f32", "ulp_2_53",
                               "ties_2_52", "eps_1e-45", "eps_3e38", "eps_1e39"}
    assert all(s <= 300 for n, s in ve.STOPPED.items() if n not in ve.ENDS_LATE)
    assert set(ve.ENDS_LATE) <= set(ve.STOPPED) and set(ve.NEVER_ENDS) <= set(ve.STOPPED)
    # one batch per (rows, eps_start, stop): a spinning eps == 0 workgroup sits beside others in its batch
    groups = ve.groups(ve.sparse_cases().values())
    assert sum(len(cs) for _, _, _, cs in groups) == 19 and max(len(cs) for _, _, _, cs in groups) <= 20
    assert any({"c_is_zero", "zeros"} <= {c.name for c in cs} for _, _, _, cs in groups)


def _variants():
    for problem in ve.PROBLEMS:
        for name, case in ve.sparse_cases().items():
            for f32 in (False, True):
                if not f32 or ve.has_f32(case):
                    yield "sparse", name, problem, f32, case, ve.sparse_want(name, problem, f32)
        for name, case in ve.dense_cases().items():
            for f32 in (False, True):
                if not f32 or ve.dense_rounded_f32(case.val) is not None:
                    yield "dense", name, problem, f32, case, ve.dense_want(name, problem, f32)


def test_every_oracle_solve_ends_within_its_stop():
    """its == stop for a case that is cut, eCE == 1 below the stop for one that ends; never a solve that ran into the
    default max_iter.  A case of NEVER_ENDS is cut in every variant, one of ENDS_LATE or without a stop ends in every
    variant, each of the others is cut in at least one."""
    cut = {}
    for layout, name, problem, f32, case, want in _variants():
        its, ece = want["meta"]["its"], want["meta"]["eCE"]
        key = (layout, name, problem, f32)
        print(key, "its", its, "eCE", ece, "stop", case.stop)
        if case.stop is None:
            assert ece == 1 and its < 1000, key
        elif name in ve.NEVER_ENDS:
            assert its == case.stop and ece == 0, key
        elif name in ve.ENDS_LATE:
            assert ece == 1 and its < case.stop, key
        else:
            assert (its == case.stop and ece == 0) or (its < case.stop and ece == 1), key
            cut[name] = cut.get(name, False) or its == case.stop
    assert cut == dict.fromkeys(("flt_max_exact", "c_is_zero", "ulp_2_53", "ties_2_52", "eps_3e38"), True)
    for problem in ve.PROBLEMS:
        for want in ve.fast_want(problem):
            assert want["meta"]["eCE"] == 1 and want["meta"]["its"] < 1000
        for name, _, dense in ve.OUTSIDE:
            wants = [ve.outside_sparse_want(name, problem), ve.outside_sparse_want(name, problem, True) if
                     ve.has_f32(ve.sparse_cases()[name]) else None, ve.outside_dense_want(name, problem) if dense else None]
            for w in wants:
                if w is not None:
                    its, ece = w[0]["meta"]["its"], w[0]["meta"]["eCE"]
                    print("outside", name, problem, "its", its, "eCE", ece)
                    assert its == ve.outside_stop(name) or (ece == 1 and its < ve.outside_stop(name))


def _best(case, problem):
    """Every row's best value (the one its first bid goes to): the largest for 'max', the smallest for 'min'."""
    v = case.val.reshape(case.rows, ve.PER_ROW)
    return v.max(axis=1) if problem == "max" else v.min(axis=1)


def _best_cost(case, problem):
    """The same in the solver's terms, where 'min' maximises cost = -v (auction_.pyx:236-237)."""
    return _best(case, problem) if problem == "max" else -_best(case, problem)


def test_the_sign_cases_hold_negative_best_values_and_ties_at_zero():
    cases = ve.sparse_cases()
    for name in ve.SIGN_NAMES:  # some row's best value is negative
        assert any((_best(cases[name], problem) < 0).any() for problem in ve.PROBLEMS), name
    # all_neg: every best value is negative; under 'max' every cost is negative, under 'min' every cost is positive (the
    # non-negative values of the other batch tests give 'min' negative costs only and 'max' positive ones only)
    for problem in ve.PROBLEMS:
        assert (_best(cases["all_neg"], problem) < 0).all()
    assert (_best_cost(cases["all_neg"], "max") < 0).all() and (_best_cost(cases["all_neg"], "min") > 0).all()
    v = cases["neg_mixed"].val.reshape(ve.BIG_ROWS, ve.PER_ROW)
    assert ((v < 0).any(axis=1) & (v > 0).any(axis=1)).any()  # rows of mixed signs
    assert (cases["all_neg"].val < 0).all()
    # C comes from a negative entry alone: eps = 1000 / 2 against values below 100
    v = cases["c_from_negative"].val
    assert (v == -1000.0).sum() == 1 and np.abs(np.delete(v, np.argmin(v))).max() < 100
    for problem in ve.PROBLEMS:
        assert ve.sparse_want("c_from_negative", problem)["extra"]["start_eps_f32"] == 500.0
        c = float(_f32(np.abs(cases["all_neg"].val).max()))
        assert ve.sparse_want("all_neg", problem)["extra"]["start_eps_f32"] == c / 2
    # ties that involve a zero: rows that hold 0 twice, among -2 .. 2; in neg_zero every one of them is -0.0
    for name in ("neg_ints", "neg_zero"):
        v = cases[name].val.reshape(ve.ROWS, ve.PER_ROW)
        assert set(np.unique(v)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert ((v == 0).sum(axis=1) >= 2).any()
        zero_tied_best = [(v == 0).sum(axis=1)[(_best(cases[name], p) == 0)] for p in ve.PROBLEMS]
        print(name, "rows whose best value is a zero:", [len(z) for z in zero_tied_best])
    z = cases["neg_zero"].val[cases["neg_zero"].val == 0]
    assert len(z) > 0 and np.signbit(z).all() and not np.signbit(cases["neg_ints"].val[cases["neg_ints"].val == 0]).any()
    for problem in ve.PROBLEMS:  # -0.0 is a value like +0.0: the same solve, bit for bit
        a, b = ve.sparse_want("neg_ints", problem), ve.sparse_want("neg_zero", problem)
        assert np.array_equal(a["sol"], b["sol"]) and np.array_equal(bits(a["p"]), bits(b["p"]))
        assert all(a["meta"][k] == b["meta"][k] for k in META_KEYS)
        assert not np.signbit(b["p"]).any()


def _values_of(layout, case, f32):
    if layout == "sparse":
        return ve.sparse_problem_of(case, f32)[1]
    mat = ve.dense_rounded_f32(case.val).astype(np.float64) if f32 else case.val
    with np.errstate(invalid="ignore"):
        return mat[mat >= 0]


def test_every_case_reaches_the_edge_it_is_named_for():
    seen, below_ulp = set(), set()
    for layout, name, problem, f32, case, want in _variants():
        key = (layout, name, problem, f32)
        v = _values_of(layout, case, f32)
        c64 = float(np.abs(v).max())
        with np.errstate(over="ignore"):
            c32 = _f32(c64)
        start, final, p = _f32(want["extra"]["start_eps_f32"]), _f32(want["extra"]["final_eps_f32"]), want["p"]
        assert not np.isnan(p).any() and not np.signbit(p).any(), key  # bids stay >= +0.0: no key ever holds a sign
        if "eps_start" not in dict(case.opts) or name == "eps_1e-46":
            with np.errstate(over="ignore"):
                assert start.view(np.uint32) == _f32(np.float64(c32) / 2.0).view(np.uint32), key  # eps = (float)(C / 2)
        if name in ("above_flt_max", "dbl_max"):
            assert c64 > ve.FLT_MAX and np.isinf(c32) and np.isinf(start) and np.isinf(final), key
            assert np.isinf(p).any() and set(np.unique(p)) <= {0.0, np.inf}, key
            if name == "dbl_max":
                assert c64 > ve.DBL_MAX / 2 and np.isinf(want["extra"]["obj_f64"]), key
        elif name == "flt_max_exact":
            assert c64 == ve.FLT_MAX and float(c32) == c64 and float(start) == ve.FLT_MAX / 2, key
            assert np.isfinite(p).all() and p.max() > ve.FLT_MAX / 2, key  # finite prices at the top of the float32 range
        elif name == "c_is_zero":
            assert c32 == 0 and start == 0 and final == 0, key
            if not f32:
                assert 0 < c64 < 2.0 ** -150, key
        elif name == "zeros":
            assert (v == 0).all() and start == 0 and (p == 0).all(), key
        elif name == "c_subnormal_f32":
            assert 0 < float(c32) < F32_TINY and 0 < float(start) < F32_TINY and want["meta"]["eCE"] == 1, key
        elif name == "c_subnormal_tie":
            assert float(c32) == 25601 * 2.0 ** -149 and float(start) == 12800 * 2.0 ** -149, key
            if not f32:  # the order of the two steps shows: halved first, C would narrow to the odd neighbour
                assert float(_f32(c64 / 2.0)) == 12801 * 2.0 ** -149, key
        elif name == "round_to_f32":
            if not f32:  # C is a tie between two float32 values and goes to the even mantissa, below the true maximum
                assert c64 % 2 == 1 and 2.0 ** 24 < c64 < 2.0 ** 25 and float(c32) == c64 - 1 and (c64 - 1) % 4 == 0, key
            assert float(start) == float(c32) / 2, key
        elif name == "ulp_2_53":
            assert c64 > 2.0 ** 53 and want["meta"]["nreductions"] >= 17 and p.max() > 2.0 ** 53, key
            if float(final) < np.spacing(p.max()):  # eps below one ulp of a price: costbest - w + eps rounds
                below_ulp.add(layout)
        elif name == "ties_2_52":
            assert set(np.unique(v)) <= {k * 2.0 ** 52 for k in range(5)} and c64 == 2.0 ** 54, key
        elif name == "eps_1e-46":
            assert _f32(1e-46) == 0 and float(start) > 1 and want["meta"]["nreductions"] >= 2, key
        elif name == "eps_1e-45":
            assert start.view(np.uint32) == 1 and final.view(np.uint32) == 1 and want["meta"]["nreductions"] == 0, key
        elif name == "eps_3e38":
            assert start == _f32(3e38) and np.isfinite(p).all() and p.max() > ve.FLT_MAX, key
        elif name == "eps_1e39":
            assert np.isinf(start) and np.isinf(final) and np.isinf(p).any(), key
        seen.add(name)
    assert seen == set(ALL_SPARSE) and below_ulp == {"sparse", "dense"}


def test_fast_forms_one_over_n_per_problem():
    probs, sizes = ve.fast_mix()
    assert [int(lo[-1, 0]) + 1 for lo, _ in probs] == list(ve.FAST_ROWS) == [int(n) for n in sizes[:, 1]]
    for problem in ve.PROBLEMS:
        for n, want in zip(ve.FAST_ROWS, ve.fast_want(problem)):
            assert _f32(want["extra"]["start_eps_f32"]).view(np.uint32) == _f32(1.0 / n).view(np.uint32)
            assert want["meta"]["nreductions"] == 0
    assert float(_f32(1.0 / 3)) != 1.0 / 3 and float(_f32(1.0 / 7)) != 1.0 / 7  # (inexact: the narrowing is visible)


def _densified(loc, val):
    n, m = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    mat = np.full((n, m), -1.0)
    mat[loc[:, 0], loc[:, 1]] = val
    return mat


def test_the_three_augmentations_give_one_problem():
    """sparse_to_augmented, ell_to_packed(outside=) and dense_to_augmented on the outside values of the GPU module,
    negative and huge ones included: the same entries (the sparse and ELL forms in the same stored order)."""
    for name, value, dense in ve.OUTSIDE:
        loc, val = ve.sparse_problem_of(ve.sparse_cases()[name])
        assert value < 0 and abs(value) > np.abs(val).max() if name in ("neg_mixed", "all_neg") else value >= 0
        (lo, va, m, n), = sparse_to_augmented(loc, val, np.array([0, len(val)]), None, value)
        assert n == ve.sparse_cases()[name].rows and lo.shape[0] == len(val) + n
        assert np.array_equal(va[lo[:, 1] >= m], np.full(n, value))
        cols, vals, rows = sof.to_ell([(loc, val)], [n], n)
        (elo, eva), = ell_to_packed(cols, vals, rows, outside=np.array([value]))
        assert np.array_equal(elo, lo) and np.array_equal(bits(eva), bits(va)), name
        aug, = dense_to_augmented(_densified(loc, val)[None], None, outside=value)
        assert aug.shape == (n, m + n)
        if not dense:  # a negative dense entry is absent: the dense call does not take these
            assert (np.diag(aug[:, m:]) < 0).all()
            continue
        i, j = np.nonzero(aug >= 0)
        order = np.lexsort((lo[:, 1], lo[:, 0]))
        assert np.array_equal(np.stack([i, j], axis=1), lo[order]) and np.array_equal(bits(aug[i, j]), bits(va[order])), name
    # -0.0, the dense form of an outside value of zero, is a valid entry there
    aug, = dense_to_augmented(ve.dense_cases()["c_is_zero"].val[None], None, outside=-0.0)
    assert np.signbit(np.diag(aug[:, ve.DENSE_SHAPE[1]:])).all() and (np.diag(aug[:, ve.DENSE_SHAPE[1]:]) >= 0).all()


@pytest.mark.parametrize("problem", ve.PROBLEMS)
def test_the_outside_value_alone_sets_c(problem):
    for name in ("neg_mixed", "all_neg"):
        want, m, n = ve.outside_sparse_want(name, problem)
        value = dict((k, v) for k, v, _ in ve.OUTSIDE)[name]
        assert want["extra"]["start_eps_f32"] == -value / 2
    want, _, _ = ve.outside_sparse_want("above_flt_max", problem)
    assert np.isinf(want["extra"]["start_eps_f32"]) and np.isinf(want["p"]).any()
    want, _, _ = ve.outside_sparse_want("c_is_zero", problem)
    assert want["extra"]["start_eps_f32"] == 0.0
