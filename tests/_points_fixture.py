"""Shared by test_points_batch.py (GPU) and test_points_batch_nogpu.py: the draws of point sets, the definition's chain
as a plain loop, the fused chain it must not be, and the CPU side of the verdict table of auction_solve_points_batch.

expected_status derives the code of every problem from points_to_dense and numpy alone, in the call's order; it never
runs the code under test.
"""
from fractions import Fraction

import numpy as np

from sslap_amd import points_to_dense

OK, INFINITE_VALUE, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE, BAD_OUTSIDE = 0, 3, 4, 5, 6, 7, 15
DTYPES = ("float64", "float32")
KINDS = ("uniform", "grid", "repeated")


def draw(kind, shape, dtype, rng):
    """Coordinates of `shape` = (..., D): uniform with full mantissas, an integer grid 0..15 (many exact ties), or
    repeated points (zero costs, identical rows)."""
    if kind == "uniform":
        return rng.uniform(-1, 1, shape).astype(dtype)
    if kind == "grid":
        return rng.integers(0, 16, shape).astype(dtype)
    if kind == "repeated":
        base = rng.uniform(-1, 1, shape[:-2] + (max(shape[-2] // 3, 1), shape[-1]))
        idx = rng.integers(0, base.shape[-2], shape[-2])
        return np.ascontiguousarray(base[..., idx, :]).astype(dtype)
    raise AssertionError(kind)


def dense_by_loops(x, y, shapes=None):
    """points_to_dense as a plain Python loop of float64 operations in the stated order (Python's float is an IEEE
    double and every operator rounds once)."""
    B, N, D = x.shape
    M = y.shape[1]
    out = np.full((B, N, M), np.inf)
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        for i in range(n):
            for j in range(m):
                d = float(x[b, i, 0]) - float(y[b, j, 0])
                s = d * d
                for k in range(1, D):
                    d = float(x[b, i, k]) - float(y[b, j, k])
                    q = d * d
                    s = s + q
                out[b, i, j] = s
    return out


def _fma(a, b, c):
    """fma(a, b, c) of three finite doubles: the exact a * b + c, rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds to nearest even)


def fused_by_loops(x, y):
    """The chain a contracting compiler would make: s_0 = d_0 * d_0, s_k = fma(d_k, d_k, s_(k-1)).  Finite inputs."""
    B, N, D = x.shape
    M = y.shape[1]
    out = np.empty((B, N, M))
    for b in range(B):
        for i in range(N):
            for j in range(M):
                d = float(x[b, i, 0]) - float(y[b, j, 0])
                s = d * d
                for k in range(1, D):
                    d = float(x[b, i, k]) - float(y[b, j, k])
                    s = _fma(d, d, s)
                out[b, i, j] = s
    return out


def outside_rows(outside, B, N):
    """outside in any of its three forms as a (B, N) float64 array."""
    o = np.asarray(outside, dtype=np.float64)
    return np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, N))


def expected_status(x, y, shapes=None, prices=None, outside=None):
    """(status, matching_size) of every problem: the first check that fails in the order shape, (outside value no entry,)
    a cost or outside value that is not finite, (n_b > m_b,) price not finite, price sign.  The brackets: with / without
    outside only.  matching_size is min(n_b, m_b) for a good shape without outside, else -1."""
    cost = points_to_dense(x, y)
    B, N, M = cost.shape
    status = np.zeros(B, dtype=np.int32)
    size = np.full(B, -1, dtype=np.int32)
    o = None if outside is None else outside_rows(outside, B, N)
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        if n < 1 or n > N or m < 1 or m > M:
            status[b] = BAD_SHAPE
            continue
        a = cost[b, :n, :m]
        p = None if prices is None else prices[b, :m]
        if o is None:
            size[b] = min(n, m)
        with np.errstate(invalid="ignore"):
            if o is not None and (~(o[b, :n] >= 0)).any():
                status[b] = BAD_OUTSIDE
            elif not np.isfinite(a).all() or (o is not None and np.isinf(o[b, :n]).any()):
                status[b] = INFINITE_VALUE
            elif o is None and n > m:
                status[b] = INFEASIBLE
            elif p is not None and not np.isfinite(p).all():
                status[b] = PRICE_NOT_FINITE
            elif p is not None and np.signbit(p).any():
                status[b] = PRICE_NEGATIVE
    return status, size


def verdict_batch(dtype="float64", N=9, M=11, D=3, seed=3):
    """dict(x, y, shapes, prices, outside, kinds): a mixed batch for the verdict table.  Healthy problems on the even
    indices; on the odd ones the defects in turn.  Coordinates beyond a shape are NaN / inf / 1e200 in places, which a
    kernel that read them would report.  outside: a (B, N) array, negative in one problem (used with outside only)."""
    rng = np.random.default_rng(seed)
    kinds = ["ok", "nan_coord", "ok", "inf_coord", "ok", "overflow", "ok", "n_gt_m", "ok", "shape_0_5", "ok", "shape_N1_1",
             "ok", "price_nan", "ok", "price_neg", "ok", "bad_outside", "ok", "nan_and_n_gt_m", "ok", "inf_outside"]
    B = len(kinds)
    x = rng.uniform(-1, 1, (B, N, D)).astype(dtype)
    y = rng.uniform(-1, 1, (B, M, D)).astype(dtype)
    shapes = np.empty((B, 2), dtype=np.int32)
    prices = np.zeros((B, M))
    outside = rng.uniform(0.5, 3.0, (B, N))
    for b, kind in enumerate(kinds):
        n = int(rng.integers(2, N))
        m = int(rng.integers(n, M))
        shapes[b] = (n, m)
        # bad coordinates BEYOND the shape: no effect
        x[b, n:] = [np.nan, np.inf, -np.inf][b % 3]
        y[b, m:] = [np.inf, np.nan, 1e30][b % 3]
        outside[b, n:] = [np.nan, -1.0, np.inf][b % 3]
        if b % 4 == 2:
            prices[b, :m] = rng.uniform(0, 1, m)
        if kind == "nan_coord":
            x[b, n - 1, D - 1] = np.nan
        elif kind == "inf_coord":
            y[b, 0, 0] = -np.inf
        elif kind == "overflow":
            if dtype == "float64":  # (2e200)^2 overflows to +inf
                x[b, 0, 1], y[b, m - 1, 1] = 1e200, -1e200
            else:  # (the square of a widened float32 difference cannot overflow a float64)
                x[b, 0, 1] = np.inf
        elif kind == "n_gt_m":
            m2 = min(m, N - 1)
            shapes[b] = (m2 + 1, m2)
            x[b, :m2 + 1] = rng.uniform(-1, 1, (m2 + 1, D))
            y[b, :m2] = rng.uniform(-1, 1, (m2, D))
            outside[b, :m2 + 1] = rng.uniform(0.5, 3.0, m2 + 1)
        elif kind == "shape_0_5":
            shapes[b] = (0, 5)
        elif kind == "shape_N1_1":
            shapes[b] = (N + 1, 1)
        elif kind == "price_nan":
            prices[b, m - 1] = np.nan
            prices[b, 0] = -1.0  # (a later check would fail as well)
        elif kind == "price_neg":
            prices[b, 0] = -0.0
        elif kind == "bad_outside":
            outside[b, n - 1] = -0.5
            x[b, 0, 0] = np.nan  # (a later check would fail as well)
        elif kind == "nan_and_n_gt_m":
            shapes[b] = (3, 2)
            x[b, :3] = rng.uniform(-1, 1, (3, D))
            y[b, :2] = rng.uniform(-1, 1, (2, D))
            y[b, 1, 0] = np.nan
            outside[b, :3] = rng.uniform(0.5, 3.0, 3)
        elif kind == "inf_outside":
            outside[b, 0] = np.inf
    for a in (x, y, shapes, prices, outside):
        a.setflags(write=False)
    return dict(x=x, y=y, shapes=shapes, prices=prices, outside=outside, kinds=kinds)
