"""Shared cases of the reverse finish of the list batches (auction_solve_sparse_batch / auction_solve_ell_batch with
finish="reverse", sslap_amd.sparse_reverse_finish): the random gated draws, packing and densifying, the ELL form of a
packed batch, and the model applied to the outputs of the same call without the finish.

What is compared with what is said in tests/_dense_finish.py, whose helpers are used as they are: on the CPU the model
is judged by scipy's optimum, by eps-CS stated directly and by the dense model on the densified stack; on the GPU the
yardstick is the model on the forward outputs of the same call, bit for bit (assert_is_the_model).
"""
import numpy as np

from sslap_amd import sparse_reverse_finish
from tests import _dense_finish as df

host, bits, records, assert_is_the_model = df.host, df.bits, df.records, df.assert_is_the_model


# ---- one problem: (loc int32 (k, 2), val float64 (k,)), rows ascending ---------------------------------------------------
def densify(loc, val, n, m):
    """The NaN-gated (n, m) matrix of a duplicate-free problem: what entries="finite" reads."""
    mat = np.full((n, m), np.nan)
    mat[loc[:, 0], loc[:, 1]] = val
    return mat


def pack(problems):
    """[(loc_b, val_b)] -> packed loc int32 (nnz, 2), val float64 (nnz,), offsets int64 (B + 1,)."""
    loc = np.concatenate([p[0].reshape(-1, 2) for p in problems]).astype(np.int32)
    val = np.concatenate([p[1] for p in problems]).astype(np.float64)
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in problems])]).astype(np.int64)
    return np.ascontiguousarray(loc), np.ascontiguousarray(val), off


def shuffled_rows(loc, val, rng):
    """The same entries with every row's stored order permuted (rows stay ascending)."""
    order = np.lexsort((rng.random(len(val)), loc[:, 0]))
    return np.ascontiguousarray(loc[order]), np.ascontiguousarray(val[order])


def to_ell(problems, ns, K, rng=None, cols_dtype=np.int32, vals_dtype=np.float64):
    """[(loc_b, val_b)] with ns rows each -> cols / vals (B, max ns, K): the entries of a row in stored order, the holes
    (-1, value 1e300 or inf: never interpreted) behind them or, with rng, moved to random slots of the row."""
    B, N = len(problems), int(max(ns))
    cols = np.full((B, N, K), -1, dtype=cols_dtype)
    vals = np.full((B, N, K), np.inf if vals_dtype == np.float32 else 1e300, dtype=vals_dtype)
    for b, (loc, val) in enumerate(problems):
        for i in range(int(ns[b])):
            at = np.flatnonzero(loc[:, 0] == i)
            assert at.size <= K
            slots = np.arange(at.size) if rng is None else np.sort(rng.permutation(K)[:at.size])
            cols[b, i, slots], vals[b, i, slots] = loc[at, 1], val[at]
    return cols, vals


def gated_problem(rng, n, m, kmax=4, empty=0.1, ints=True, high=50):
    """n rows, 0 .. kmax distinct candidates per row among m columns (a row in `empty` of the cases has none), in
    ascending column order; integer values below `high` (or float32-exact multiples of 1 / 8)."""
    rows, cols = [], []
    for i in range(n):
        k = 0 if rng.random() < empty else int(rng.integers(0, min(kmax, m) + 1))
        c = np.sort(rng.permutation(m)[:k])
        rows.append(np.full(k, i))
        cols.append(c)
    loc = np.stack([np.concatenate(rows), np.concatenate(cols)], axis=1).astype(np.int32).reshape(-1, 2)
    val = rng.integers(0, high, len(loc)).astype(np.float64)
    if not ints:
        val = val + rng.integers(0, 8, len(loc)) / 8.0
    return loc, val


def gated_draws(count=400, seed=20261021):
    """count sparse gated integer problems: n <= 40, m <= 60, 0 - 4 distinct candidates per row, one row in ten empty,
    an outside value per row, min and max in turn, arbitrary integer starting prices below 60."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n, m = int(rng.integers(1, 41)), int(rng.integers(1, 61))
        loc, val = gated_problem(rng, n, m)
        yield dict(k=k, n=n, m=m, loc=loc, val=val, problem=("min", "max")[k % 2],
                   outside=rng.integers(0, 50, n).astype(np.float64), p0=rng.integers(0, 60, m + n).astype(np.float64))


def finish_one(loc, val, n, m, problem, p, p2o, eps32, outside, **kw):
    """sparse_reverse_finish on one problem in the state (p, p2o) of its augmented form; returns (result, p, p2o) in the
    augmented form again."""
    sol = np.where(p2o < m, p2o, -1).astype(np.int32)[None]
    res = sparse_reverse_finish(loc, val, np.array([0, len(val)]), sol, p[None, :m], np.array([eps32], dtype=np.float32),
                                np.array([[n, m]]), problem=problem, outside=outside[None], outside_prices=p[None, m:], **kw)
    q = np.concatenate([res["prices"][0], res["outside_prices"][0]])
    return res, q, df.augmented_p2o(res["sol"][0], m)


def duplicates_case():
    """One 2 x 3 problem ("max") whose row 0 holds (0, 2) three times -- 5.0, 9.0, 7.0 in stored order -- in the state
    sol = [0, 1], prices = [0, 0, 20], eps = 0.5: object 2 is unassigned above lambda = 0."""
    loc = np.array([[0, 0], [0, 2], [0, 2], [0, 2], [1, 1], [1, 2]], dtype=np.int32)
    val = np.array([3.0, 5.0, 9.0, 7.0, 4.0, 8.0])
    return dict(loc=loc, val=val, offsets=np.array([0, 6], dtype=np.int64), sol=np.array([[0, 1]], dtype=np.int32),
                prices=np.array([[0.0, 0.0, 20.0]]), eps=np.array([0.5], dtype=np.float32), shapes=np.array([[2, 3]]))


# ---- a GPU result against the model ------------------------------------------------------------------------------------
def shapes_of(res0):
    """(n_b, m_b) of every problem from the records of a device result: n_rows, and n_cols (minus n_rows with outside)."""
    rec = records(res0)
    n = rec["n_rows"].astype(np.int64)
    m = rec["n_cols"].astype(np.int64) - (n if "outside_prices" in res0 else 0)
    return np.stack([n, m], axis=1)


def model_of(packed, res0, problem="min", outside=None, max_iter=1000000, trace=None):
    """The numpy model on the outputs res0 of the call without the finish (device result): what finish="reverse" must
    give.  packed: (loc, val, offsets) on the host, or a list of (loc_b, val_b) pairs."""
    rec = records(res0)
    run = (host(res0["status"]) == 0) & (rec["n_assigned"] == rec["n_rows"])
    loc, val, off = packed if isinstance(packed, tuple) else (packed, None, None)
    return sparse_reverse_finish(loc, val, off, host(res0["sol"]), host(res0["prices"]), rec["final_eps"], shapes_of(res0),
                                 problem=problem, outside=outside.cpu().numpy() if hasattr(outside, "cpu") else outside,
                                 outside_prices=host(res0["outside_prices"]) if "outside_prices" in res0 else None,
                                 max_iter=max_iter, run=run, trace=trace)
