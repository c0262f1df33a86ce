"""The reverse finish of the dense batch without a GPU: sslap_amd.dense_reverse_finish, the numpy statement that defines
auction_solve_batch(finish="reverse"), against scipy's optimum and against eps-CS stated directly, on random integer
problems behind a plain forward auction from arbitrary prices and on the CPU oracle's own final states; the hand-built
situations of the GPU test (the forward solve there is the oracle's, bit for bit, so they can be shown here); and the
front end's keyword.
"""
import ctypes as C

import numpy as np
import pytest

import sslap_amd
from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_batch, dense_reverse_finish
from tests import _dense_finish as df

DRAWS = 400


def test_the_model_is_public():
    assert "dense_reverse_finish" in sslap_amd.__all__ and sslap_amd.dense_reverse_finish is dense_reverse_finish


def test_integer_draws_reach_scipys_optimum_and_keep_the_structure():
    """Every draw, none left out: behind a forward phase from arbitrary non-negative integer prices (eps = 0.9 / n, so
    n * eps < 1 and integer values leave no room below the optimum) the finish reaches scipy's optimum exactly, the
    assignment is an injection onto entries, eps-CS holds and no unassigned object is priced above lambda."""
    missed_before, finished = 0, 0
    for d in df.integer_draws(DRAWS):
        n, m = d["n"], d["m"]
        a, valid = df.maximised(d["mat"], d["problem"], d["outside"])
        eps32 = np.float32(0.9 / n)
        p, p2o = df.forward_auction(a, valid, d["p0"], float(eps32))
        best = df.optimum(a, valid)
        missed_before += a[np.arange(n), p2o].sum() != best
        lam = p[p2o].min()
        res, q, q2o = df.finish_one(d["mat"], d["problem"], p, p2o, eps32, d["outside"])
        assert res["ran"][0] and res["reverse"]["left"][0] == 0 and res["reverse"]["its"][0] >= 0, d["k"]
        df.assert_structure(a, valid, q, q2o, float(eps32), lam)
        assert a[np.arange(n), q2o].sum() == best, d["k"]
        want_obj = best if d["problem"] == "max" else -best
        assert res["obj_f64"][0] == want_obj and res["eCE"][0] == 1, d["k"]
        finished += 1
    assert finished == DRAWS
    assert missed_before > DRAWS // 2  # (what the finish is for: the forward phase alone misses most of them)


ORACLE_CASES = [(n, extra, kind, problem, out, seed)
                for seed, (n, extra) in enumerate([(3, 1), (5, 4), (8, 8), (12, 3), (16, 20), (24, 9)])
                for kind in ("int", "float") for problem in ("min", "max") for out in (False, True)]


@pytest.mark.parametrize("n,extra,kind,problem,out,seed", ORACLE_CASES)
def test_the_oracles_final_states_become_optimal(n, extra, kind, problem, out, seed):
    """The reference's default eps-scaling on a rectangular problem, then the finish: the optimum (exact for integers,
    within n * final_eps for floats), and oracle.ece_satisfied at 1 / n stays true."""
    rng = np.random.default_rng(1000 + seed)
    m = n + extra
    mat = rng.integers(0, 50, (n, m)).astype(np.float64) if kind == "int" else rng.uniform(0, 100, (n, m))
    outside = None
    if out:
        outside = rng.integers(0, 50, n).astype(np.float64) if kind == "int" else rng.uniform(0, 100, n)
    st = df.oracle_state(mat, problem, outside)
    assert st["n_assigned"] == n
    a, valid = df.maximised(mat, problem, outside)
    lam = st["p"][st["p2o"]].min()
    res, q, q2o = df.finish_one(mat, problem, st["p"].copy(), st["p2o"].copy(), st["eps32"], outside)
    eps = float(st["eps32"])
    df.assert_structure(a, valid, q, q2o, eps, lam)
    got, best = a[np.arange(n), q2o].sum(), df.optimum(a, valid)
    if kind == "int":
        assert got == best
    else:
        assert best - n * eps - 1e-9 <= got <= best + 1e-9
    assert orc.ece_satisfied(st["loc"], st["val"], problem, q, q2o, 1.0 / n)
    assert res["eCE"][0] == 1 and res["reverse"]["left"][0] == 0


def test_the_budget_cuts_the_finish_where_the_model_says():
    d = next(x for x in df.integer_draws(40) if x["m"] - x["n"] > 20 and x["outside"] is None)
    a, valid = df.maximised(d["mat"], d["problem"])
    eps32 = np.float32(0.9 / d["n"])
    p, p2o = df.forward_auction(a, valid, d["p0"], float(eps32))
    full, _, _ = df.finish_one(d["mat"], d["problem"], p, p2o, eps32)
    assert full["reverse"]["its"][0] > 3
    cut, _, _ = df.finish_one(d["mat"], d["problem"], p, p2o, eps32, max_iter=3)
    assert cut["reverse"]["its"][0] == 3 and cut["reverse"]["left"][0] > 0


def test_a_problem_that_is_not_to_run_is_untouched():
    mats = np.array([[[1.0, 2.0, 3.0], [3.0, 1.0, 2.0]]] * 2)
    sol = np.array([[0, 1], [0, -1]], dtype=np.int32)  # problem 1: a row without an object
    prices = np.array([[1.0, 1.0, 9.0], [1.0, 1.0, 9.0]])
    res = dense_reverse_finish(mats, sol, prices, np.full(2, 0.5, dtype=np.float32), problem="max")
    assert res["ran"].tolist() == [True, False] and res["reverse"]["its"].tolist()[1] == -1
    assert res["reverse"]["left"].tolist() == [0, -1] and np.array_equal(res["prices"][1], prices[1])
    res = dense_reverse_finish(mats, sol, prices, np.full(2, 0.5, dtype=np.float32), problem="max", run=[False, False])
    assert not res["ran"].any() and np.array_equal(res["sol"], sol) and np.array_equal(res["prices"], prices)


@pytest.mark.parametrize("name", list(df.situations()))
def test_the_hand_built_situations_occur(name):
    """On the reference's forward state (the GPU's, bit for bit) each situation of the GPU test is met by the model."""
    case = df.situations()[name]
    mats, kw = case["mats"], dict(case["kw"])
    p0, problem = kw.pop("prices"), kw.pop("problem")
    B, N, M = mats.shape
    sol, prices, eps = np.empty((B, N), dtype=np.int32), np.empty((B, M)), np.empty(B, dtype=np.float32)
    for b in range(B):
        st = df.oracle_state(mats[b], problem, p0=p0[b], **kw)
        sol[b], prices[b], eps[b] = st["p2o"], st["p"], st["eps32"]
    trace = []
    model = dense_reverse_finish(mats, sol, prices, eps, problem=problem, trace=trace)
    assert model["ran"].all() and (model["reverse"]["left"] == 0).all()
    assert df.situation_holds(case, dict(prices=prices), model, trace), trace[:8]


# ---- the front end ------------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for the library: records every entry point that is called with its arguments and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("misslap_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, len(args)))
            if name.endswith(("_status", "_outside")):  # ..., status, matching_size, meta, info: every problem is solved
                status = args[-4]
                address = status.value if isinstance(status, C.c_void_p) else int(status)
                np.ctypeslib.as_array(C.cast(address, C.POINTER(C.c_int32)), (MATS.shape[0],))[...] = 0
            return 0
        return call


MATS = np.array([[[1.0, -1.0, 3.0], [2.0, 5.0, -1.0]], [[4.0, 2.0, -1.0], [0.0, 1.0, 2.0]]])


@pytest.mark.parametrize("finish", ["forward", "Reverse", "", 1, True, b"reverse"])
@pytest.mark.parametrize("errors", ["raise", "status"])
def test_a_bad_finish_raises_before_the_library_is_reached(monkeypatch, finish, errors):
    spy = _Spy()
    monkeypatch.setattr(_lib, "load", lambda: spy)
    with pytest.raises(ValueError, match="finish must be None or 'reverse'"):
        auction_solve_batch(MATS, errors=errors, finish=finish)
    assert spy.calls == []


@pytest.mark.parametrize("kw", [dict(), dict(errors="status"), dict(outside=1.0), dict(errors="status", entries="finite"),
                                dict(errors="status", outside=np.array([2.0, 3.0]), fast=True)])
def test_finish_none_is_todays_call(monkeypatch, kw):
    """finish=None reaches the library through exactly the calls of a call without the keyword, and never through the
    finish's entry point."""
    seen = []
    for extra in (dict(), dict(finish=None)):
        spy = _Spy()
        monkeypatch.setattr(_lib, "load", lambda spy=spy: spy)
        res = auction_solve_batch(MATS, **kw, **extra)
        assert "reverse" not in res
        seen.append((spy.calls, sorted(res)))
    assert seen[0] == seen[1] and len(seen[0][0]) == 1
    assert seen[0][0][0][0] in ("misslap_solve_dense_batch", "misslap_solve_dense_batch_status",
                                "misslap_solve_dense_batch_outside")
