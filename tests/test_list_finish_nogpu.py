"""The reverse finish of the list batches without a GPU: sslap_amd.sparse_reverse_finish, the numpy statement that defines
auction_solve_sparse_batch / auction_solve_ell_batch(finish="reverse"), against scipy's optimum and eps-CS stated
directly on random gated problems behind a plain forward auction from arbitrary prices, against the dense model on the
densified stack, on the ELL form, with duplicates, where it must not run and under a budget; and the front ends'
keyword.
"""
import ctypes as C

import numpy as np
import pytest

import sslap_amd
from sslap_amd import (_lib, auction_solve_ell_batch, auction_solve_sparse_batch, dense_reverse_finish, ell_to_packed,
                       sparse_reverse_finish)
from tests import _dense_finish as df
from tests import _list_finish as lf

DRAWS = 400


def test_the_model_is_public():
    assert "sparse_reverse_finish" in sslap_amd.__all__ and sslap_amd.sparse_reverse_finish is sparse_reverse_finish


def _forward(d):
    n, m = d["n"], d["m"]
    a, valid = df.maximised(lf.densify(d["loc"], d["val"], n, m), d["problem"], d["outside"], entries="finite")
    eps32 = np.float32(0.9 / n)
    p, p2o = df.forward_auction(a, valid, d["p0"], float(eps32))
    return a, valid, eps32, p, p2o


def test_gated_draws_reach_scipys_optimum_and_keep_the_structure():
    """Every draw, none left out: behind a forward phase from arbitrary integer prices below 60 (eps = 0.9 / n, so
    n * eps < 1 and integer values leave no room below the optimum) the finish reaches scipy's optimum exactly, the
    assignment is an injection onto entries, eps-CS holds, no unassigned object is priced above lambda and left == 0."""
    missed_before, finished = 0, 0
    for d in lf.gated_draws(DRAWS):
        n, m = d["n"], d["m"]
        a, valid, eps32, p, p2o = _forward(d)
        best = df.optimum(a, valid)
        missed_before += a[np.arange(n), p2o].sum() != best
        lam = p[p2o].min()
        res, q, q2o = lf.finish_one(d["loc"], d["val"], n, m, d["problem"], p, p2o, eps32, d["outside"])
        assert res["ran"][0] and res["reverse"]["left"][0] == 0 and res["reverse"]["its"][0] >= 0, d["k"]
        df.assert_structure(a, valid, q, q2o, float(eps32), lam)
        assert a[np.arange(n), q2o].sum() == best, d["k"]
        assert res["obj_f64"][0] == (best if d["problem"] == "max" else -best) and res["eCE"][0] == 1, d["k"]
        finished += 1
    assert finished == DRAWS
    assert missed_before > DRAWS // 2  # (what the finish is for: the forward phase alone misses most of them)


@pytest.mark.parametrize("shuffle", [False, True])
def test_the_list_model_is_the_dense_model(shuffle):
    """Duplicate-free problems, rows stored in ascending or in shuffled column order: sparse_reverse_finish and
    dense_reverse_finish(entries="finite") on the NaN-gated densified stack agree bit for bit in sol, prices,
    outside_prices, its, left and the trace.  The finish does not depend on the stored order."""
    rng = np.random.default_rng(5)
    draws = list(lf.gated_draws(48, seed=99))
    B, N, M = len(draws), max(d["n"] for d in draws), max(d["m"] for d in draws)
    mats, out = np.full((B, N, M), np.nan), np.zeros((B, N))
    sol, prices, oprices = np.full((B, N), -1, dtype=np.int32), np.zeros((B, M)), np.zeros((B, N))
    eps, shapes, problems = np.zeros(B, dtype=np.float32), np.zeros((B, 2), dtype=np.int64), []
    problem = "max"
    for b, d in enumerate(draws):
        d["problem"] = problem
        n, m = d["n"], d["m"]
        _, _, eps[b], p, p2o = _forward(d)
        mats[b, :n, :m], out[b, :n], shapes[b] = lf.densify(d["loc"], d["val"], n, m), d["outside"], (n, m)
        sol[b, :n], prices[b, :m], oprices[b, :n] = np.where(p2o < m, p2o, -1), p[:m], p[m:]
        problems.append(lf.shuffled_rows(d["loc"], d["val"], rng) if shuffle else (d["loc"], d["val"]))
    t_list, t_dense = [], []
    got = sparse_reverse_finish(*lf.pack(problems), sol, prices, eps, shapes, problem=problem, outside=out,
                                outside_prices=oprices, trace=t_list)
    want = dense_reverse_finish(mats, sol, prices, eps, problem=problem, shapes=shapes, outside=out, outside_prices=oprices,
                                entries="finite", trace=t_dense)
    assert got["ran"].all() and want["ran"].all() and t_list == t_dense and len(t_list) > B
    assert np.array_equal(got["sol"], want["sol"])
    for key in ("prices", "outside_prices"):
        assert np.array_equal(df.bits(got[key]), df.bits(want[key])), key
    for key in ("its", "left"):
        assert np.array_equal(got["reverse"][key], want["reverse"][key]), key
    # (duplicate-free: the last stored entry is the only one, so eCE and the objective agree too)
    assert np.array_equal(got["eCE"], want["eCE"]) and np.array_equal(df.bits(got["obj_f64"]), df.bits(want["obj_f64"]))


def test_ell_is_packed_and_the_holes_may_move():
    rng = np.random.default_rng(6)
    draws = list(lf.gated_draws(16, seed=7))
    ns = [d["n"] for d in draws]
    problems = [(d["loc"], d["val"]) for d in draws]
    B, N, M = len(draws), max(ns), max(d["m"] for d in draws)
    sol, prices, oprices = np.full((B, N), -1, dtype=np.int32), np.zeros((B, M)), np.zeros((B, N))
    eps, shapes, out = np.zeros(B, dtype=np.float32), np.zeros((B, 2), dtype=np.int64), np.zeros((B, N))
    for b, d in enumerate(draws):
        d["problem"] = "min"
        n, m = d["n"], d["m"]
        _, _, eps[b], p, p2o = _forward(d)
        sol[b, :n], prices[b, :m], oprices[b, :n], shapes[b], out[b, :n] = np.where(p2o < m, p2o, -1), p[:m], p[m:], (n, m), d["outside"]
    kw = dict(problem="min", outside=out, outside_prices=oprices)
    want = sparse_reverse_finish(*lf.pack(problems), sol, prices, eps, shapes, **kw)
    for move in (None, rng):
        cols, vals = lf.to_ell(problems, ns, 6, move)
        got = sparse_reverse_finish(ell_to_packed(cols, vals, np.array(ns)), None, None, sol, prices, eps, shapes, **kw)
        for key in ("sol", "prices", "outside_prices", "obj_f64", "eCE"):
            assert got[key].tobytes() == want[key].tobytes(), key
        assert np.array_equal(got["reverse"]["its"], want["reverse"]["its"]) and (got["reverse"]["left"] == 0).all()
    assert want["reverse"]["its"].sum() > B


def test_duplicates_use_the_largest_value_and_the_list_rules():
    d = lf.duplicates_case()
    trace = []
    res = sparse_reverse_finish(d["loc"], d["val"], d["offsets"], d["sol"], d["prices"], d["eps"], d["shapes"], problem="max",
                                trace=trace)
    # object 2 starts above lambda = 0 and unassigned; row 0 holds (0, 2) twice, 5.0 and then 9.0 and then 7.0: the image
    # has 9.0, so row 0 (profit 3) wins it over row 1 (8.0, profit 4: w = 4) with w = 6, at omega - eps = 3.5
    assert trace == [(0, 2, 0, 0, False)] and res["sol"][0].tolist() == [2, 1]
    assert res["prices"][0].tolist() == [0.0, 0.0, 3.5]
    # the list rules: the choice is the LAST stored copy (7.0), and the objective counts all three copies
    assert res["obj_f64"][0] == 5.0 + 9.0 + 7.0 + 4.0
    # eCE: LHS = 7 - 3.5 + 1e-7 against the copy worth 9 - 3.5 at target eps 0.5: 3.5 < 5.0 -> violated
    assert res["eCE"][0] == 0 and res["reverse"]["its"][0] == 1 and res["reverse"]["left"][0] == 0


def test_a_problem_that_is_not_to_run_is_untouched():
    loc = np.array([[0, 0], [0, 2], [1, 1], [1, 2]] * 2, dtype=np.int32)
    val = np.array([1.0, 3.0, 1.0, 2.0] * 2)
    off = np.array([0, 4, 8])
    sol = np.array([[0, 1], [0, -1]], dtype=np.int32)  # problem 1: a row without an object
    prices = np.array([[1.0, 1.0, 9.0], [1.0, 1.0, 9.0]])
    args = (loc, val, off, sol, prices, np.full(2, 0.5, dtype=np.float32), np.array([[2, 3], [2, 3]]))
    res = sparse_reverse_finish(*args, problem="max")
    assert res["ran"].tolist() == [True, False] and res["reverse"]["its"].tolist()[1] == -1
    assert res["reverse"]["left"].tolist() == [0, -1] and np.array_equal(res["prices"][1], prices[1])
    assert res["reverse"]["its"][0] >= 1 and not np.array_equal(res["prices"][0], prices[0])
    res = sparse_reverse_finish(*args, problem="max", run=[False, False])
    assert not res["ran"].any() and np.array_equal(res["sol"], sol) and np.array_equal(res["prices"], prices)
    assert np.isnan(res["obj_f64"]).all() and (res["reverse"]["its"] == -1).all()


def test_the_budget_cuts_the_finish_where_the_model_says():
    d = next(x for x in lf.gated_draws(60) if x["n"] > 20)
    _, _, eps32, p, p2o = _forward(d)
    one = lambda **kw: lf.finish_one(d["loc"], d["val"], d["n"], d["m"], d["problem"], p, p2o, eps32, d["outside"], **kw)[0]
    trace = []
    full = one(trace=trace)
    assert full["reverse"]["its"][0] > 3
    cut = one(max_iter=3)
    assert cut["reverse"]["its"][0] == 3 and cut["reverse"]["left"][0] > 0
    # left: the unassigned objects priced above lambda once the first three iterations are made, the next one included
    replay = one(max_iter=3, trace=(t3 := []))
    assert t3 == trace[:3] and replay["reverse"]["left"][0] == cut["reverse"]["left"][0]
    m = d["m"]
    q = np.concatenate([cut["prices"][0], cut["outside_prices"][0]])
    held = np.zeros(q.size, dtype=bool)
    held[df.augmented_p2o(cut["sol"][0], m)] = True
    assert cut["reverse"]["left"][0] == np.count_nonzero(~held & (q > p[p2o].min()))


# ---- the front ends -----------------------------------------------------------------------------------------------------
class _Spy:
    """Stands in for the library: records every entry point that is called with the number of its arguments, names a
    workspace of 256 bytes and returns 0 with every status 0."""

    def __init__(self, B):
        self.calls, self.B = [], B

    def __getattr__(self, name):
        if not name.startswith("misslap_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, len(args)))
            if name.endswith("_bytes"):
                return 256
            if name.endswith(("_status", "_outside", "_ell_batch")):  # ..., status, matching_size, meta, info
                status = args[-4]
                address = status.value if isinstance(status, C.c_void_p) else int(status)
                np.ctypeslib.as_array(C.cast(address, C.POINTER(C.c_int32)), (self.B,))[...] = 0
            return 0
        return call


LOC = np.array([[0, 0], [0, 2], [1, 0], [1, 1], [0, 1], [1, 2]], dtype=np.int32)
VAL = np.array([1.0, 3.0, 2.0, 5.0, 4.0, 2.0])
OFF = np.array([0, 4, 6])
COLS = np.array([[[0, 2], [0, 1]], [[1, -1], [2, -1]]], dtype=np.int32)
VALS = np.array([[[1.0, 3.0], [2.0, 5.0]], [[4.0, 0.0], [2.0, 0.0]]])
CALLS = {"sparse": lambda **kw: auction_solve_sparse_batch(LOC, VAL, OFF, **kw),
         "ell": lambda **kw: auction_solve_ell_batch(COLS, VALS, **kw)}


@pytest.mark.parametrize("finish", ["forward", "Reverse", "", 1, True, b"reverse"])
@pytest.mark.parametrize("errors", ["raise", "status"])
@pytest.mark.parametrize("which", list(CALLS))
def test_a_bad_finish_raises_before_the_library_is_reached(monkeypatch, which, finish, errors):
    spy = _Spy(2)
    monkeypatch.setattr(_lib, "load", lambda: spy)
    with pytest.raises(ValueError, match="finish must be None or 'reverse'"):
        CALLS[which](errors=errors, finish=finish)
    assert spy.calls == []


@pytest.mark.parametrize("which,kw", [("sparse", dict()), ("sparse", dict(errors="status")), ("sparse", dict(outside=1.0)),
                                      ("sparse", dict(errors="status", outside=np.array([2.0, 3.0]), dims=(2, 3))),
                                      ("ell", dict()), ("ell", dict(errors="status", n_cols=3)),
                                      ("ell", dict(outside=np.array([2.0, 3.0]), rows=np.array([2, 2])))])
def test_finish_none_is_todays_call(monkeypatch, which, kw):
    """finish=None reaches the library through exactly the calls of a call without the keyword, with as many arguments,
    never through a finish's entry point, and returns the same keys."""
    seen = []
    for extra in (dict(), dict(finish=None)):
        spy = _Spy(2)
        monkeypatch.setattr(_lib, "load", lambda spy=spy: spy)
        res = CALLS[which](**kw, **extra)
        assert "reverse" not in res
        seen.append((spy.calls, sorted(res)))
    assert seen[0] == seen[1] and len(seen[0][0]) == 1
    assert seen[0][0][0][0] in ("misslap_solve_sparse_batch", "misslap_solve_sparse_batch_status",
                                "misslap_solve_sparse_batch_outside", "misslap_solve_ell_batch",
                                "misslap_solve_ell_batch_outside")
