"""The reverse finish of the points batch without a GPU: sslap_amd.points_reverse_finish, the numpy statement that
defines auction_solve_points_batch(finish="reverse"), against dense_reverse_finish on points_to_dense (bit for bit),
against scipy's optimum and eps-CS stated directly on integer-grid problems behind a plain forward auction from
arbitrary prices; and the front end's keyword.
"""
import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, auction_solve_points_batch, dense_reverse_finish, points_reverse_finish, points_to_dense
from tests import _dense_finish as df
from tests import _points_finish as pf
from tests import _points_fixture as fx

DRAWS = 400


def test_the_model_is_public():
    assert "points_reverse_finish" in sslap_amd.__all__ and sslap_amd.points_reverse_finish is points_reverse_finish


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("dtype", fx.DTYPES)
@pytest.mark.parametrize("D", pf.DIMS)
def test_the_model_is_the_dense_model_on_points_to_dense(D, dtype, outside):
    """Cropped shapes, both coordinate types, with and without outside: every returned array, bit for bit."""
    rng = np.random.default_rng(100 * D + 10 * outside + (dtype == "float32"))
    B, N, M = 4, 9, 14
    x, y = fx.draw("uniform", (B, N, D), dtype, rng), fx.draw("uniform", (B, M, D), dtype, rng)
    shapes = np.array([[9, 14], [1, 14], [5, 6], [9, 10]], dtype=np.int32)
    x[2, 5:], y[2, 6:] = np.nan, np.inf  # (beyond the shape: never read)
    problem = ("min", "max")[D % 2]
    o = rng.uniform(0.5, 3.0, (B, N)) if outside else None
    mats = points_to_dense(x, y, shapes)
    sol, prices, oprices = np.full((B, N), -1, dtype=np.int32), np.zeros((B, M)), np.zeros((B, N))
    eps = np.empty(B, dtype=np.float32)
    for b, (n, m) in enumerate(shapes):
        a, valid = df.maximised(mats[b, :n, :m], problem, None if o is None else o[b, :n])
        eps[b] = np.float32(0.01 / n)
        p, p2o = df.forward_auction(a, valid, rng.uniform(0, 6, a.shape[1]), float(eps[b]))
        sol[b, :n], prices[b, :m], oprices[b, :n] = np.where(p2o < m, p2o, -1), p[:m], p[m:] if outside else 0.0
    kw = dict(problem=problem, shapes=shapes, outside=o, outside_prices=oprices if outside else None, max_iter=1000)
    t0, t1 = [], []
    want = dense_reverse_finish(mats, sol, prices, eps, trace=t0, **kw)
    got = points_reverse_finish(x, y, sol, prices, eps, trace=t1, **kw)
    assert want["ran"].all() and (want["reverse"]["its"] > 0).any() and t0 == t1
    assert sorted(got) == sorted(want)
    for key in want:
        if key == "reverse":
            assert all(np.array_equal(got[key][f], want[key][f]) and got[key][f].dtype == want[key][f].dtype for f in ("its", "left"))
        else:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key


def test_integer_grid_draws_reach_scipys_optimum_and_keep_the_structure():
    """Every draw, none left out: behind a forward phase from arbitrary non-negative integer prices (eps = 1 / (n + 1),
    so n * eps < 1 and integer costs leave no room below the optimum) the finish reaches scipy's optimum exactly with
    left == 0, the assignment is an injection, eps-CS holds and no unassigned object is priced above lambda.  The forward
    state alone misses the optimum on at least 300 of the 400."""
    missed_before, finished = 0, 0
    for d in pf.grid_draws(DRAWS):
        n, m = d["n"], d["m"]
        mat = points_to_dense(d["x"][None], d["y"][None])[0]
        assert mat.max() <= 49 * d["D"] and (mat == np.round(mat)).all()
        a, valid = df.maximised(mat, d["problem"], d["outside"])
        eps32 = np.float32(1.0 / (n + 1))
        p, p2o = df.forward_auction(a, valid, d["p0"], float(eps32))
        best = df.optimum(a, valid)
        missed_before += a[np.arange(n), p2o].sum() != best
        lam = p[p2o].min()
        res, q, q2o = pf.finish_one(d["x"], d["y"], d["problem"], p, p2o, eps32, d["outside"])
        assert res["ran"][0] and res["reverse"]["left"][0] == 0 and res["reverse"]["its"][0] >= 0, d["k"]
        df.assert_structure(a, valid, q, q2o, float(eps32), lam)
        assert a[np.arange(n), q2o].sum() == best, d["k"]
        assert res["obj_f64"][0] == (best if d["problem"] == "max" else -best) and res["eCE"][0] == 1, d["k"]
        finished += 1
    print("the forward state alone missed the optimum on", missed_before, "of", DRAWS)
    assert finished == DRAWS
    assert missed_before >= 300


# ---- the situations of the GPU test, on the oracle's forward state (the GPU's, bit for bit) ------------------------------
def _on_the_oracle(case, eps=None, max_iter=1000000):
    kw = dict(case["kw"])
    problem, outside, prices = kw.pop("problem"), kw.pop("outside", None), kw.pop("prices")
    kw.setdefault("fast", True)
    fwd = pf.oracle_forward(case["x"], case["y"], problem=problem, outside=outside, prices=prices, **kw)
    trace = []
    res = points_reverse_finish(case["x"], case["y"], fwd["sol"], fwd["prices"],
                                fwd["final_eps"] if eps is None else np.full(len(fwd["sol"]), eps, dtype=np.float32),
                                problem=problem, outside=outside, outside_prices=fwd["outside_prices"], max_iter=max_iter,
                                trace=trace)
    return fwd, res, trace


def test_the_ties_case_has_moves_whose_beta_two_rows_share():
    case = pf.ties_case()
    fwd, res, trace = _on_the_oracle(case)
    assert res["ran"].all() and (res["reverse"]["left"] == 0).all()
    ties = sum(pf.beta_ties(case["x"], case["y"], case["kw"]["problem"], None, fwd, b, [t[1:] for t in trace if t[0] == b])
               for b in range(case["x"].shape[0]))
    assert ties >= 1


def test_the_chains_case_has_a_chained_pick_and_a_drop():
    _, res, trace = _on_the_oracle(pf.chains_case())
    assert res["ran"].all() and pf.holds_chain_and_drop(trace)


def test_the_stall_case_stalls_at_the_rewritten_eps():
    _, res, trace = _on_the_oracle(pf.stall_case(), eps=pf.STALL_EPS, max_iter=5000)
    assert res["ran"].all() and pf.holds_stall(trace)
    stalled = sorted({t[0] for t in trace if t[2] >= 0 and t[3] == -1})
    assert (res["reverse"]["left"][stalled] > 0).all() and (res["reverse"]["its"][stalled] < 5000).all()


# ---- the front end ------------------------------------------------------------------------------------------------------
X = np.zeros((2, 3, 2))
Y = np.ones((2, 4, 2))


@pytest.mark.parametrize("finish", ["forward", 1, "Reverse", "", True, b"reverse"])
@pytest.mark.parametrize("errors", ["raise", "status"])
def test_a_bad_finish_raises_before_the_library_is_reached(monkeypatch, finish, errors):
    def load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", load)
    with pytest.raises(ValueError, match="finish must be left out or 'reverse'"):
        auction_solve_points_batch(X, Y, errors=errors, finish=finish)
    with pytest.raises(ValueError, match="finish must be left out or 'reverse'"):
        auction_solve_points_batch(X, Y, outside=1.0, prices=np.zeros((2, 4)), errors=errors, finish=finish)


def test_finish_none_stays_the_type_error_it_was(monkeypatch):
    """Before the keyword existed finish=None was an unexpected keyword (tests/test_points_batch_nogpu.py pins the
    TypeError); the call without a finish is the call with the keyword left out."""
    def load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", load)
    with pytest.raises(TypeError, match="finish"):
        auction_solve_points_batch(X, Y, finish=None)


def test_the_entry_point_is_bound():
    assert "misslap_points_batch_reverse_finish" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["misslap_points_batch_reverse_finish"][1]) == 24
