"""Shared cases of the reverse finish of the dense batch (auction_solve_batch(finish="reverse"),
sslap_amd.dense_reverse_finish): the random draws, a plain forward auction, the optimum by scipy, the structure a
finished state must have, the hand-built situations, and the comparison of a GPU result with the numpy model applied to
the outputs of the same call without the finish.

What is compared with what.  On the CPU the model is judged by scipy's optimum and by eps-CS stated directly.  On the
GPU the yardstick is always the model on the forward outputs of the same call (the forward solve is pinned to the oracle
elsewhere), bit for bit.
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from sslap_amd import _lib, dense_reverse_finish, dense_to_augmented, dense_to_packed

BIG = 1.0e7  # what an absent entry costs scipy: above every sum of 32 values below 50 (and of 1024 below 100)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# ---- one problem as the model sees it ----------------------------------------------------------------------------------
def maximised(mat, problem, outside=None, entries="nonneg"):
    """(a, valid) of one problem: the maximised values over the m real objects and, with outside (n,), the n outside
    objects; valid marks the entries."""
    v = np.asarray(mat, dtype=np.float64)
    n = v.shape[0]
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(v) if entries == "finite" else v >= 0
    if outside is not None:
        d = np.zeros((n, n))
        d[np.arange(n), np.arange(n)] = outside
        v, valid = np.hstack([v, d]), np.hstack([valid, np.eye(n, dtype=bool)])
    return (v if problem == "max" else v * -1.0), valid


def forward_auction(a, valid, p0, eps):
    """A Gauss-Seidel forward auction from prices p0: every row ends on an object within eps of its best net value
    (eps-CS).  A row with one entry raises its price by 100 + eps.  Returns (p, p2o)."""
    n, mo = a.shape
    p = np.array(p0, dtype=np.float64)
    p2o, o2p = np.full(n, -1), np.full(mo, -1)
    todo = list(range(n))
    while todo:
        i = todo.pop()
        js = np.flatnonzero(valid[i])
        net = a[i, js] - p[js]
        k = int(np.argmax(net))
        gap = net[k] - np.delete(net, k).max() if js.size > 1 else 100.0
        j = int(js[k])
        p[j] += gap + eps
        if o2p[j] >= 0:
            p2o[o2p[j]] = -1
            todo.append(int(o2p[j]))
        p2o[i], o2p[j] = j, i
    return p, p2o


def optimum(a, valid):
    """The largest total of a over the complete assignments onto entries (scipy)."""
    from scipy.optimize import linear_sum_assignment
    w = np.where(valid, a, -BIG)
    r, c = linear_sum_assignment(w, maximize=True)
    assert valid[r, c].all()
    return float(a[r, c].sum())


def assert_structure(a, valid, p, p2o, eps, lam, slack=1e-9):
    """A finished state: an injection onto entries, eps-CS (slack: the rounding of a few thousand float64 operations on
    values below 1e4, each within 2e-12), and no unassigned object priced above lam."""
    n, mo = a.shape
    assert len(set(p2o.tolist())) == n and (p2o >= 0).all() and (p2o < mo).all()
    assert valid[np.arange(n), p2o].all()
    with np.errstate(invalid="ignore"):
        net = np.where(valid, a - p[None, :], -np.inf)
    own = net[np.arange(n), p2o]
    assert (own >= net.max(axis=1) - eps - slack).all()
    free = np.ones(mo, dtype=bool)
    free[p2o] = False
    assert (p[free] <= lam).all()
    assert (p[~free] >= lam).all()


def augmented_p2o(sol, m):
    sol = np.asarray(sol).astype(np.int64)
    return np.where(sol < 0, m + np.arange(sol.shape[0]), sol)


# ---- the random integer draws of the CPU test -----------------------------------------------------------------------------
def integer_draws(count=400, seed=20261020):
    """count problems: n <= 32, m - n <= 39, every second one with an outside value per row, gates of 0 / 50 / 90 %,
    integer values below 50, min and max in turn, arbitrary non-negative integer starting prices.  Without outside a
    random injection is kept free of gates, so that a complete assignment exists."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(1, 33))
        m = n + int(rng.integers(0, 40))
        out, problem, gate = k % 2 == 1, ("min", "max")[(k // 2) % 2], (0.0, 0.5, 0.9)[(k // 4) % 3]
        vals = rng.integers(0, 50, (n, m)).astype(np.float64)
        gated = rng.random((n, m)) < gate
        if not out:
            gated[np.arange(n), rng.permutation(m)[:n]] = False
        mat = np.where(gated, -1.0, vals)
        outside = rng.integers(0, 50, n).astype(np.float64) if out else None
        p0 = rng.integers(0, 60, m + (n if out else 0)).astype(np.float64)
        yield dict(k=k, n=n, m=m, mat=mat, problem=problem, outside=outside, p0=p0)


def finish_one(mat, problem, p, p2o, eps32, outside=None, entries="nonneg", **kw):
    """dense_reverse_finish on one problem in the state (p, p2o) of its augmented form; returns (result, p, p2o) with the
    prices and the assignment in the augmented form again."""
    n, m = mat.shape
    sol = np.where(p2o < m, p2o, -1).astype(np.int32)[None]
    res = dense_reverse_finish(mat[None], sol, p[None, :m], np.array([eps32], dtype=np.float32), problem=problem,
                               outside=None if outside is None else outside[None],
                               outside_prices=None if outside is None else p[None, m:], entries=entries, **kw)
    q = res["prices"][0] if outside is None else np.concatenate([res["prices"][0], res["outside_prices"][0]])
    return res, q, augmented_p2o(res["sol"][0], m)


# ---- the oracle's final state of one dense problem ------------------------------------------------------------------------
def oracle_state(mat, problem, outside=None, p0=None, **kw):
    """The reference's solve of one problem (with outside: of dense_to_augmented's matrix), optionally from prices p0:
    dict(p (mo,), p2o, eps32, loc, val) -- loc / val the entries in the caller's sign, for oracle.ece_satisfied."""
    n, m = mat.shape
    full = mat if outside is None else dense_to_augmented(mat[None], outside=outside[None])[0]
    o = orc.from_matrix(full, problem=problem, **kw)
    if p0 is not None:
        np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))[:] = np.asarray(p0, dtype=np.float64)[:o.M]
    p2o = o.solve()
    st = o.state()
    p = np.zeros(full.shape[1])
    p[:o.M] = st["p"]
    loc, val = dense_to_packed(full[None])[0]
    return dict(p=p, p2o=p2o.astype(np.int64), eps32=np.float32(st["eps"]), loc=loc, val=val, n_assigned=o.meta["n_assigned"])


# ---- hand-built situations (n <= 40): the forward solve is the reference's, so its final state is known on the CPU ---------
def situations():
    """name -> dict(mats (B, N, M) float64, kw of auction_solve_batch, expect): each built so that the finish meets the
    named situation; `expect` is checked on the model's trace by situation_holds."""
    rng = np.random.default_rng(77)
    out = {}
    # a column without any entry, priced above everything: it drops to lambda without a row
    mat = rng.integers(1, 40, (5, 9)).astype(np.float64)
    mat[:, 6] = -1.0
    p0 = np.zeros((1, 9))
    p0[0, 6] = 500.0
    out["empty_column"] = dict(mats=mat[None], kw=dict(problem="max", fast=True, prices=p0), expect="empty_column", col=6)
    # a row with a single entry bids +inf: its object is priced +inf, its profit is -inf
    mat = rng.integers(1, 40, (6, 11)).astype(np.float64)
    mat[2, :] = -1.0
    mat[2, 4] = 7.0
    out["single_entry_row"] = dict(mats=mat[None], kw=dict(problem="max", fast=True, prices=rng.integers(0, 90, (1, 11)).astype(np.float64)),
                                   expect="inf_price")
    # chains: many objects start far above the prices in use, so a freed object is taken up at once, and again
    mat = rng.integers(0, 100, (4, 40, 56)).astype(np.float64)
    out["chain"] = dict(mats=mat, kw=dict(problem="max", fast=True, prices=rng.integers(0, 300, (4, 56)).astype(np.float64)),
                        expect="chain")
    # two rows tie for beta: rows 0 and 1 value object 2 alike and hold the same profit; the smaller row must move
    mat = np.array([[10.0, 0.0, 30.0], [0.0, 10.0, 30.0]])
    out["beta_tie"] = dict(mats=mat[None], kw=dict(problem="max", eps_start=0.5, prices=np.array([[0.0, 0.0, 100.0]])),
                           expect="tie")
    # lambda == beta - eps exactly: one row, eps = 1 (fast at n = 1).  The row bids 10 - 0 + 1 = 11 for object 0 (profit
    # -1), object 1 is worth 11 + 1 = 12 to it: 12 - 1 == 11 == lambda, so the object drops to lambda and nothing moves
    mat = np.array([[10.0, 11.0, 0.0]])
    out["lambda_equals_beta_minus_eps"] = dict(mats=mat[None], kw=dict(problem="max", fast=True, prices=np.array([[0.0, 100.0, 0.0]])),
                                               expect="equality")
    return out


def situation_holds(case, res0, model, trace):
    """Whether the finish of `case` met its situation: judged on the forward outputs res0 (host arrays), the model's
    result and its trace."""
    kind = case["expect"]
    if kind == "empty_column":
        return any(j == case["col"] and i == -1 for _, j, i, _, _ in trace) and model["reverse"]["its"][0] >= 1
    if kind == "inf_price":
        return bool(np.isinf(host(res0["prices"])).any()) and model["reverse"]["its"][0] >= 1
    if kind == "chain":  # an object freed by an iteration is processed next and frees an object that is processed next
        return any(trace[t][4] and trace[t + 1][4] and trace[t][0] == trace[t + 1][0] for t in range(len(trace) - 1))
    if kind == "tie":
        return trace == [(0, 2, 0, 0, False)] and model["sol"][0].tolist() == [2, 1]
    if kind == "equality":
        return trace == [(0, 1, -1, -1, False)] and model["sol"][0].tolist() == [0]
    raise KeyError(kind)


# ---- a GPU result against the model ------------------------------------------------------------------------------------
_FIELDS = [f[0] for f in _lib.DenseBatchMeta._fields_]


def records(res):
    """The meta records of a device result as a structured array (waits for the call's stream)."""
    res["stream"].synchronize()
    raw = res["records"].cpu().numpy()
    metas = (_lib.DenseBatchMeta * raw.shape[0]).from_buffer_copy(raw.tobytes())
    return np.ctypeslib.as_array(metas).copy()


def model_of(mats, res0, problem="min", shapes=None, outside=None, entries="nonneg", max_iter=1000000, trace=None, **_):
    """The numpy model on the outputs res0 of the call without the finish (device result): what finish="reverse" must give."""
    rec = records(res0)
    run = (host(res0["status"]) == 0) & (rec["n_assigned"] == rec["n_rows"])
    return dense_reverse_finish(mats, host(res0["sol"]), host(res0["prices"]), rec["final_eps"], problem=problem,
                                shapes=None if shapes is None else host(shapes), outside=outside,
                                outside_prices=host(res0["outside_prices"]) if "outside_prices" in res0 else None,
                                entries=entries, max_iter=max_iter, run=run, trace=trace)


def assert_is_the_model(res1, res0, want):
    """res1 (finish="reverse") against the model `want` of res0 (finish=None), bit for bit: sol, prices, outside_prices,
    reverse.its / left, meta.obj_f64 / obj_f32 / eCE, every other meta field and status / matching_size unchanged."""
    rec0, rec1 = records(res0), records(res1)
    ran = want["ran"]
    for key in ("status", "matching_size"):
        assert np.array_equal(host(res1[key]), host(res0[key])), key
    assert np.array_equal(host(res1["sol"]), want["sol"])
    assert np.array_equal(bits(host(res1["prices"])), bits(want["prices"]))
    assert ("outside_prices" in res1) == ("outside_prices" in want)
    if "outside_prices" in want:
        assert np.array_equal(bits(host(res1["outside_prices"])), bits(want["outside_prices"]))
    its, left = host(res1["reverse"]["its"]), host(res1["reverse"]["left"])
    assert its.dtype == np.int64 and left.dtype == np.int32 and its.shape == left.shape == ran.shape
    assert np.array_equal(its, want["reverse"]["its"]) and np.array_equal(left, want["reverse"]["left"])
    assert np.array_equal((its >= 0), ran)
    for f in _FIELDS:
        if f in ("obj_f64", "obj_f32", "eCE"):
            assert rec1[f][~ran].tobytes() == rec0[f][~ran].tobytes(), f
        else:
            assert rec1[f].tobytes() == rec0[f].tobytes(), f
    assert np.array_equal(bits(rec1["obj_f64"][ran]), bits(want["obj_f64"][ran]))
    assert rec1["obj_f32"][ran].tobytes() == want["obj_f32"][ran].tobytes()
    assert np.array_equal(rec1["eCE"][ran], want["eCE"][ran])
    # where the finish did not run nothing of the problem was touched
    for key in ("sol", "prices", "outside_prices"):
        if key in res0:
            assert host(res1[key])[~ran].tobytes() == host(res0[key])[~ran].tobytes(), key
