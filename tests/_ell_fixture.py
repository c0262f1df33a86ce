"""Shared by test_ell_batch.py (GPU) and test_ell_batch_nogpu.py: padded candidate lists (cols, vals of shape (B, N, K))
built from the sparse draws of tests/_batch_shapes.py, the plain-Python definition of their packed form, the status each
problem must get -- derived here on the CPU from the definition in include/misslap.h, not from the library -- and the
mixed batch that holds a problem of every status code of misslap_solve_ell_batch.
"""
import functools

import numpy as np

from tests._batch_shapes import sparse_problem, sparse_problem_distinct

INT_MAX = 2**31 - 1
CAP = 2048  # MISSLAP_SPARSE_BATCH_MAX_DIM
(OK, TOO_FEW_VALUES, EMPTY_ROW, INFINITE_VALUE, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE) = range(8)
TOO_LARGE, PRICES_TOO_NARROW = 13, 14
ORDER = (BAD_SHAPE, EMPTY_ROW, INFINITE_VALUE, TOO_LARGE, PRICES_TOO_NARROW, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE)
# what a hole may hold: its column is any negative number, its value is never interpreted
HOLE_COLS = (-1, -2, -(2**31))
HOLE_VALS = (np.nan, np.inf, -np.inf, -1.0, 1e300)
DTYPES = ((np.int32, np.float64), (np.int64, np.float32), (np.int64, np.float64), (np.int32, np.float32))


def widen(loc, val, n, K, rng, N=None):
    """A problem of n rows with k stored entries in every row (sparse_problem / sparse_problem_distinct) as (N, K) cols /
    vals: row i's entries keep their order and land in k of the K slots drawn at random, the other slots are holes --
    in front, between (tied) entries and behind -- and the rows n .. N - 1 are holes throughout."""
    k = loc.shape[0] // n
    assert loc.shape[0] == n * k and k <= K and np.array_equal(loc[:, 0], np.repeat(np.arange(n), k))
    N = n if N is None else N
    cols = rng.choice(np.array(HOLE_COLS), (N, K)).astype(np.int64)
    vals = rng.choice(np.array(HOLE_VALS), (N, K))
    for i in range(n):
        at = np.sort(rng.choice(K, k, replace=False))
        cols[i, at] = loc[i * k:(i + 1) * k, 1]
        vals[i, at] = val[i * k:(i + 1) * k]
    return cols, vals


def stack(probs, N, K, fill_col=-1, fill_val=np.nan):
    """[(cols_b (n_b, K), vals_b)] -> cols (B, N, K) int64, vals (B, N, K) float64, rows (B,) int32; the rows beyond n_b
    hold fill_col / fill_val."""
    B = len(probs)
    cols = np.full((B, N, K), fill_col, dtype=np.int64)
    vals = np.full((B, N, K), fill_val, dtype=np.float64)
    rows = np.empty(B, dtype=np.int32)
    for b, (c, v) in enumerate(probs):
        cols[b, :c.shape[0]] = c
        vals[b, :c.shape[0]] = v
        rows[b] = c.shape[0]
    return cols, vals, rows


def packed_by_loops(cols, vals, rows=None):
    """The definition, as a plain double loop: the entries of rows 0 .. rows[b] - 1 in row order, within a row in slot
    order, holes (negative columns) dropped; loc int32, val float64."""
    out = []
    for b in range(cols.shape[0]):
        loc, val = [], []
        for i in range(cols.shape[1] if rows is None else int(rows[b])):
            for k in range(cols.shape[2]):
                if cols[b, i, k] >= 0:
                    loc.append((i, int(cols[b, i, k])))
                    val.append(float(vals[b, i, k]))
        out.append((np.array(loc, dtype=np.int32).reshape(-1, 2), np.array(val, dtype=np.float64)))
    return out


def max_matching(adj, m):
    """Cardinality of a maximum matching of rows (adj[i]: the columns of row i) into m columns: augmenting paths."""
    owner = [-1] * m

    def augment(i, seen):
        for j in adj[i]:
            if j not in seen:
                seen.add(j)
                if owner[j] == -1 or augment(owner[j], seen):
                    owner[j] = i
                    return True
        return False
    return sum(augment(i, set()) for i in range(len(adj)))


def expected_status(cols, vals, rows, n_cols, prices=None, cardinality_check=True):
    """(status, matching_size, counts (B, 3) = n_rows, n_cols, nnz of the meta record) of every problem, from the
    definition: the first check that fails in the order of include/misslap.h."""
    B, N, K = cols.shape
    status, size, counts = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32), np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        n = N if rows is None else int(rows[b])
        if n < 1 or n > N:
            status[b] = BAD_SHAPE
            continue
        c, v = cols[b, :n], vals[b, :n]
        valid = c >= 0
        m = int(c[valid].max()) + 1 if valid.any() else 0
        counts[b] = (n, min(m, INT_MAX), int(valid.sum()))
        empty = not valid.any(axis=1).all()
        clean = not empty and m <= n_cols
        if cardinality_check and clean:
            size[b] = max_matching([list(dict.fromkeys(int(j) for j in c[i][valid[i]])) for i in range(n)], m)
        if empty:
            status[b] = EMPTY_ROW
        elif not np.isfinite(v[valid].astype(np.float64)).all():
            status[b] = INFINITE_VALUE
        elif m > n_cols:
            status[b] = TOO_LARGE
        elif prices is not None and prices.shape[1] < m:
            status[b] = PRICES_TOO_NARROW
        elif cardinality_check and size[b] < n:
            status[b] = INFEASIBLE
        elif prices is not None and not np.isfinite(prices[b, :m]).all():
            status[b] = PRICE_NOT_FINITE
        elif prices is not None and np.signbit(prices[b, :m]).any():
            status[b] = PRICE_NEGATIVE
    return status, size, counts


# ---- the mixed batch: a healthy problem at every even index, a condemned one at every odd index
MIXED_N, MIXED_K, MIXED_COLS, MIXED_P = 24, 9, 40, 36


@functools.lru_cache(maxsize=1)
def mixed_batch():
    """dict(cols int64 (B, N, K), vals, rows, prices (B, P), kinds (B,)): kinds[b] is the status planted in problem b, the
    FIRST check it fails; several carry a second defect that a later check would report.  Problems are healthy draws
    with a planted perfect matching; every column is below MIXED_P except where a defect says otherwise."""
    rng = np.random.default_rng([9, 1])
    N, K, P = MIXED_N, MIXED_K, MIXED_P
    probs, rows, kinds = [], [], []

    def healthy(n=None, m=30, k=5, kind="uniform"):
        n = int(rng.integers(3, N + 1)) if n is None else n
        loc, val = sparse_problem(rng, n, max(m, n), k, kind)
        return widen(loc, val, n, K, rng)

    def entries(c, i):
        return np.flatnonzero(c[i] >= 0)

    def add(cv, kind, n=None):
        probs.append(cv)
        rows.append(cv[0].shape[0] if n is None else n)
        kinds.append(kind)

    def bad_shape(r):
        c, v = healthy()
        add((c, v), BAD_SHAPE, r)

    def empty_row(also_nan=False):
        c, v = healthy(n=10)
        c[4] = rng.choice(np.array(HOLE_COLS), K)
        if also_nan:
            v[2, entries(c, 2)[0]] = np.nan
        add((c, v), EMPTY_ROW)

    def infinite(bad, also_large=False):
        c, v = healthy(n=12)
        v[7, entries(c, 7)[-1]] = bad
        if also_large:
            c[0, entries(c, 0)[0]] = MIXED_COLS + 3
        add((c, v), INFINITE_VALUE)

    def too_large(col, also_infeasible=False):
        c, v = healthy(n=9)
        c[5, entries(c, 5)[1]] = col
        if also_infeasible:
            c[1], c[2] = -1, -1
            c[1, 3], c[2, 0] = 7, 7
            v[1, 3], v[2, 0] = 1.0, 2.0
        add((c, v), TOO_LARGE)

    def too_narrow(also_bad_price=False):
        c, v = healthy(n=8)
        c[3, entries(c, 3)[0]] = P + 1  # (below MIXED_COLS, beyond the prices)
        add((c, v), PRICES_TOO_NARROW)
        return also_bad_price

    def infeasible(also_bad_price=False):
        c, v = healthy(n=11)
        c[2], c[9] = -1, -3  # two rows whose only entry is the same column
        c[2, K - 1], c[9, 0] = 6, 6
        v[2, K - 1], v[9, 0] = 1.5, 2.5
        add((c, v), INFEASIBLE)
        return also_bad_price

    def bad_price(kind):
        add(healthy(n=7), kind)

    plans = [lambda: bad_shape(0), lambda: bad_shape(N + 1), lambda: bad_shape(-5), lambda: empty_row(),
             lambda: empty_row(also_nan=True), lambda: infinite(np.nan), lambda: infinite(np.inf, also_large=True),
             lambda: infinite(-np.inf), lambda: too_large(MIXED_COLS), lambda: too_large(MIXED_COLS + 4),
             lambda: too_large(2**31 + 5),
             lambda: too_large(CAP + 7, also_infeasible=True), lambda: too_narrow(), lambda: too_narrow(True),
             lambda: infeasible(), lambda: infeasible(True), lambda: bad_price(PRICE_NOT_FINITE),
             lambda: bad_price(PRICE_NOT_FINITE), lambda: bad_price(PRICE_NEGATIVE), lambda: bad_price(PRICE_NEGATIVE)]
    spoil = []  # problems whose starting prices get a second defect
    for plan in plans:
        add(healthy(kind="ints" if len(probs) % 4 == 0 else "uniform"), OK)
        if plan():
            spoil.append(len(probs) - 1)
    add(healthy(n=N), OK)
    # a healthy problem with a NaN and a column beyond every bound in its holes' VALUES only, and rows beyond n_b that
    # hold what would condemn it if they were read
    cols, vals, _ = stack(probs, N, K, fill_col=INT_MAX, fill_val=np.inf)
    rows = np.array(rows, dtype=np.int32)
    kinds = np.array(kinds, dtype=np.int32)
    B = len(probs)
    prices = rng.uniform(0, 5, (B, P))
    prices[::4] = 0.0
    seen = {PRICE_NOT_FINITE: 0, PRICE_NEGATIVE: 0}
    for b in np.flatnonzero(np.isin(kinds, (PRICE_NOT_FINITE, PRICE_NEGATIVE))):
        c = cols[b, :rows[b]]
        used = np.unique(c[c >= 0])
        bad = {PRICE_NOT_FINITE: (np.nan, np.inf), PRICE_NEGATIVE: (-0.0, -3.0)}[int(kinds[b])][seen[int(kinds[b])] % 2]
        prices[b, used[-1]] = bad
        if kinds[b] == PRICE_NOT_FINITE and seen[PRICE_NOT_FINITE]:
            prices[b, used[0]] = -1.0  # (a later check too)
        seen[int(kinds[b])] += 1
    for b in spoil:
        prices[b, 0] = np.nan
    for b in np.flatnonzero(kinds == OK):  # what lies beyond a problem's columns is not its price
        c = cols[b, :rows[b]]
        prices[b, int(c.max()) + 1:] = np.nan if b % 8 == 0 else -1.0
    for a in (cols, vals, rows, prices, kinds):
        a.setflags(write=False)
    return dict(cols=cols, vals=vals, rows=rows, prices=prices, kinds=kinds)
