"""Shared cases of the reverse finish of the points batch (auction_solve_points_batch(finish="reverse"),
sslap_amd.points_reverse_finish): the integer-grid draws of the CPU test, the numpy model on the forward outputs of a
GPU call, and the two calls of a GPU case with their comparison.

What is compared with what is tests/_dense_finish.py's rule: on the CPU the model is judged by scipy's optimum and by
eps-CS stated directly; on the GPU the yardstick is always the model on the forward outputs of the same call with
finish left out, bit for bit (assert_is_the_model's field list).
"""
import numpy as np

from sslap_amd import auction_solve_points_batch, points_reverse_finish, points_to_dense
from tests import _dense_finish as df
from tests import _points_fixture as fx

DIMS = (1, 2, 3, 8)


def grid_draws(count=400, seed=20261021):
    """count problems on integer coordinates 0 .. 7 (costs are exact integers <= 49 D <= 392): n <= 32, m - n < 40, D
    cycling through 1, 2, 3, 8, every second one with an integer outside value per row, min and max in turn, arbitrary
    non-negative integer starting prices below 60."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(1, 33))
        m = n + int(rng.integers(0, 40))
        D = DIMS[k % 4]
        out, problem = k % 2 == 1, ("min", "max")[(k // 2) % 2]
        x = rng.integers(0, 8, (n, D)).astype(np.float64)
        y = rng.integers(0, 8, (m, D)).astype(np.float64)
        outside = rng.integers(0, 50, n).astype(np.float64) if out else None
        p0 = rng.integers(0, 60, m + (n if out else 0)).astype(np.float64)
        yield dict(k=k, n=n, m=m, D=D, x=x, y=y, problem=problem, outside=outside, p0=p0)


def finish_one(x, y, problem, p, p2o, eps32, outside=None, **kw):
    """points_reverse_finish on one problem in the state (p, p2o) of its augmented form; returns (result, p, p2o) with the
    prices and the assignment in the augmented form again."""
    n, m = x.shape[0], y.shape[0]
    sol = np.where(p2o < m, p2o, -1).astype(np.int32)[None]
    res = points_reverse_finish(x[None], y[None], sol, p[None, :m], np.array([eps32], dtype=np.float32), problem=problem,
                                outside=None if outside is None else outside[None],
                                outside_prices=None if outside is None else p[None, m:], **kw)
    q = res["prices"][0] if outside is None else np.concatenate([res["prices"][0], res["outside_prices"][0]])
    return res, q, df.augmented_p2o(res["sol"][0], m)


def oracle_forward(x, y, problem="min", outside=None, prices=None, **kw):
    """The reference's forward solve of every problem of the full shape on points_to_dense(x, y), from `prices` (B, M):
    the state the GPU call ends its forward solve in, bit for bit (pinned elsewhere).  kw: eps_start, max_iter, fast of
    oracle.from_matrix.  Returns dict(sol, prices, outside_prices or None, final_eps)."""
    mats = points_to_dense(x, y)
    B, N, M = mats.shape
    o = None if outside is None else fx.outside_rows(outside, B, N)
    sol, p, eps = np.empty((B, N), dtype=np.int32), np.empty((B, M)), np.empty(B, dtype=np.float32)
    op = None if o is None else np.empty((B, N))
    for b in range(B):
        p0 = None if prices is None else np.concatenate([prices[b], np.zeros(0 if o is None else N)])
        st = df.oracle_state(mats[b], problem, None if o is None else o[b], p0=p0, **kw)
        assert st["n_assigned"] == N
        sol[b], p[b], eps[b] = np.where(st["p2o"] < M, st["p2o"], -1), st["p"][:M], st["eps32"]
        if o is not None:
            op[b] = st["p"][M:]
    return dict(sol=sol, prices=p, outside_prices=op, final_eps=eps)


def beta_ties(x, y, problem, outside, fwd, b, steps):
    """Replays the model's trace `steps` of problem b ((j, i*, freed object, chained) per iteration) from the forward
    state fwd (oracle_forward's, or host copies of a call's outputs with final_eps) and returns the number of moves
    whose beta was shared by two or more rows; asserts on the way that the replay and the trace agree on i*."""
    n, m = x.shape[1], y.shape[1]
    a, valid = df.maximised(points_to_dense(x[b:b + 1], y[b:b + 1])[0], problem,
                            None if outside is None else fx.outside_rows(outside, x.shape[0], n)[b])
    p = fwd["prices"][b].copy() if outside is None else np.concatenate([fwd["prices"][b], fwd["outside_prices"][b]])
    p2o = df.augmented_p2o(fwd["sol"][b], m)
    eps, lam = float(fwd["final_eps"][b]), p[p2o].min()
    pi = a[np.arange(n), p2o] - p[p2o]
    ties = 0
    for j, istar, jo, _ in steps:
        if istar < 0:
            p[j] = lam
            continue
        rows = np.flatnonzero(valid[:, j])
        w = a[rows, j] - pi[rows]
        k = int(np.argmax(w))
        assert rows[k] == istar
        ties += int(np.count_nonzero(w == w[k]) >= 2)
        if jo < 0:  # the stalled iteration: the last one
            break
        omega = np.delete(w, k).max() if rows.size > 1 else -np.inf
        p[j] = max(lam, omega - eps)
        pi[istar] = a[istar, j] - p[j]
        p2o[istar] = j
    return ties


# ---- the situations of the GPU test; tests/test_points_finish_nogpu.py holds each to its claim on the oracle's state ------
def ties_case():
    """Integer-grid coordinates 0 .. 3: many bit-equal costs and profits."""
    rng = np.random.default_rng(41)
    B, n, m, D = 3, 24, 40, 2
    return dict(x=rng.integers(0, 4, (B, n, D)).astype(np.float64), y=rng.integers(0, 4, (B, m, D)).astype(np.float64),
                kw=dict(problem="max", fast=True, prices=rng.integers(0, 30, (B, m)).astype(np.float64)))


def chains_case():
    """Many objects start far above the prices in use: a freed object is taken up at once, others drop to lambda."""
    rng = np.random.default_rng(43)
    B, n, m, D = 2, 40, 56, 3
    return dict(x=rng.uniform(0, 10, (B, n, D)), y=rng.uniform(0, 10, (B, m, D)),
                kw=dict(problem="max", fast=True, prices=rng.integers(0, 300, (B, m)).astype(np.float64)))


STALL_EPS = 2.0 ** -60


def stall_case():
    """Integer-grid problems with outside; the finish is given eps = 2**-60, below one ulp of the profits."""
    rng = np.random.default_rng(47)
    B, n, m, D = 4, 12, 20, 2
    return dict(x=rng.integers(0, 8, (B, n, D)).astype(np.float64), y=rng.integers(0, 8, (B, m, D)).astype(np.float64),
                kw=dict(problem="min", outside=rng.integers(5, 50, (B, n)).astype(np.float64),
                        prices=rng.integers(0, 60, (B, m)).astype(np.float64)))


def holds_chain_and_drop(trace):
    """a chained pick (the object freed by one iteration is processed by the next) and an object that drops to lambda
    without a row"""
    chained = any(t[4] and trace[k - 1][0] == t[0] and trace[k - 1][3] == t[1] for k, t in enumerate(trace) if k)
    return chained and any(t[2] == -1 for t in trace)


def holds_stall(trace):
    """some problem's trace ends in a stalled iteration: a row and no freed object"""
    return any(t[2] >= 0 and t[3] == -1 for t in trace)


def model_of(x, y, res0, problem="min", shapes=None, outside=None, max_iter=1000000, trace=None, final_eps=None, **_):
    """The numpy model on the outputs res0 of the call without the finish (device result): what finish="reverse" must
    give.  final_eps: instead of the records' (the stall test rewrites them)."""
    rec = df.records(res0)
    run = (df.host(res0["status"]) == 0) & (rec["n_assigned"] == rec["n_rows"])
    return points_reverse_finish(x, y, df.host(res0["sol"]), df.host(res0["prices"]),
                                 rec["final_eps"] if final_eps is None else final_eps, problem=problem,
                                 shapes=None if shapes is None else df.host(shapes), outside=outside,
                                 outside_prices=df.host(res0["outside_prices"]) if "outside_prices" in res0 else None,
                                 max_iter=max_iter, run=run, trace=trace)


def check(x, y, trace=None, **kw):
    """Both calls on the device point sets, the model on the first one's outputs, the comparison.  Returns (forward
    result, finished result, model)."""
    r0 = auction_solve_points_batch(x, y, errors="status", **kw)
    r1 = auction_solve_points_batch(x, y, errors="status", finish="reverse", **kw)
    want = model_of(x, y, r0, trace=trace, **kw)
    df.assert_is_the_model(r1, r0, want)
    return r0, r1, want
