"""Shared by test_points_whiten.py (GPU) and test_points_whiten_nogpu.py: draws of whitening matrices, the whitened
definition as a plain loop, the fused chain it must not be, the edge cases of the chain and the CPU side of the
verdict table of auction_solve_points_batch(whiten=).

Nothing here runs the code under test: expected_status derives every code from points_to_dense(whiten=) and numpy.
"""
from fractions import Fraction

import numpy as np

from sslap_amd import points_to_dense
from tests._points_fixture import BAD_OUTSIDE, BAD_SHAPE, INFEASIBLE, INFINITE_VALUE, outside_rows

WHITEN_DIMS = (1, 2, 3, 4)


def draw_whiten(kind, shape, dtype, rng):
    """Lower-triangular matrices of `shape` = (..., D, D) with NaN above the diagonal: uniform entries with full
    mantissas (a positive diagonal away from zero), or an integer grid -2 .. 2 with a diagonal 1 .. 3 (exact ties; every
    cost of integer coordinates is an integer)."""
    D = shape[-1]
    if kind == "uniform":
        w = rng.uniform(-1, 1, shape)
        w[..., np.arange(D), np.arange(D)] = rng.uniform(0.5, 2.0, shape[:-1])
    elif kind == "grid":
        w = rng.integers(-2, 3, shape).astype(np.float64)
        w[..., np.arange(D), np.arange(D)] = rng.integers(1, 4, shape[:-1])
    else:
        raise AssertionError(kind)
    w[..., ~np.tril(np.ones((D, D), dtype=bool))] = np.nan
    return w.astype(dtype)


def identity_whiten(B, N, D, dtype):
    """The identity for every row, NaN above the diagonal."""
    w = np.full((B, N, D, D), np.nan, dtype=dtype)
    w[..., np.tril(np.ones((D, D), dtype=bool))] = 0.0
    w[..., np.arange(D), np.arange(D)] = 1.0
    return w


def whitened_by_loops(x, y, w, shapes=None):
    """points_to_dense(x, y, shapes, whiten=w) as a plain Python loop of float64 operations in the stated order
    (Python's float is an IEEE double and every operator rounds once).  Reads W[b, i, k, l] for l <= k, i < n_b only."""
    B, N, D = x.shape
    M = y.shape[1]
    out = np.full((B, N, M), np.inf)
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        for i in range(n):
            for j in range(m):
                d = [float(x[b, i, l]) - float(y[b, j, l]) for l in range(D)]
                s = 0.0
                for k in range(D):
                    z = float(w[b, i, k, 0]) * d[0]
                    for l in range(1, k + 1):
                        z = z + float(w[b, i, k, l]) * d[l]
                    q = z * z
                    s = q if k == 0 else s + q
                out[b, i, j] = s
    return out


def _fma(a, b, c):
    """fma(a, b, c) of three finite doubles: the exact a * b + c, rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def whitened_fused_by_loops(x, y, w):
    """The chain a contracting compiler would make: z_k = fma(W[k][l], d_l, z_k), s_k = fma(z_k, z_k, s_(k-1)).
    Finite inputs."""
    B, N, D = x.shape
    M = y.shape[1]
    out = np.empty((B, N, M))
    for b in range(B):
        for i in range(N):
            for j in range(M):
                d = [float(x[b, i, l]) - float(y[b, j, l]) for l in range(D)]
                s = 0.0
                for k in range(D):
                    z = float(w[b, i, k, 0]) * d[0]
                    for l in range(1, k + 1):
                        z = _fma(float(w[b, i, k, l]), d[l], z)
                    s = z * z if k == 0 else _fma(z, z, s)
                out[b, i, j] = s
    return out


def inf_minus_inf_case():
    """(x, y, w) of one 1 x 1 float64 problem with D = 2 and finite inputs whose cost is a NaN: row 1 of W times
    d = (1e200, -1e200) is 1e400 - 1e400 = inf - inf."""
    x = np.array([[[1e200, -1e200]]])
    y = np.zeros((1, 1, 2))
    w = np.array([[[[1.0, np.nan], [1e200, 1e200]]]])
    return x, y, w


def expected_status(x, y, w, shapes=None, prices=None, outside=None):
    """(status, matching_size) of every problem of a whitened call, as tests._points_fixture.expected_status derives
    them, on points_to_dense(x, y, shapes, whiten=w)."""
    cost = points_to_dense(x, y, shapes, whiten=w)
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
                status[b] = 5
            elif p is not None and np.signbit(p).any():
                status[b] = 6
    return status, size


def verdict_batch(dtype="float64", N=9, M=11, D=3, seed=4):
    """dict(x, y, w, shapes, outside, kinds): a mixed whitened batch for the verdict table.  Healthy problems on the
    even indices (NaN above every diagonal and in the rows beyond every shape); on the odd ones the defects in turn."""
    rng = np.random.default_rng(seed)
    kinds = ["ok", "nan_triangle", "ok", "inf_w000", "ok", "nan_upper_only", "ok", "nan_rows_beyond", "ok", "overflow",
             "ok", "inf_minus_inf", "ok", "shape_0_5", "ok", "bad_outside", "ok", "nan_coord"]
    B = len(kinds)
    x = rng.uniform(-1, 1, (B, N, D)).astype(dtype)
    y = rng.uniform(-1, 1, (B, M, D)).astype(dtype)
    w = draw_whiten("uniform", (B, N, D, D), dtype, rng)
    shapes = np.empty((B, 2), dtype=np.int32)
    outside = rng.uniform(0.5, 3.0, (B, N))
    for b, kind in enumerate(kinds):
        n = int(rng.integers(2, N))
        m = int(rng.integers(n, M))
        shapes[b] = (n, m)
        w[b, n:] = [np.nan, np.inf, -np.inf][b % 3]  # beyond the shape: never read
        x[b, n:] = np.nan
        outside[b, n:] = np.nan
        if kind == "nan_triangle":
            w[b, n - 1, D - 1, 0] = np.nan
        elif kind == "inf_w000":
            w[b, 0, 0, 0] = np.inf
        elif kind == "overflow":
            if dtype == "float64":  # z_0 = 1e100 * 2e100 is finite, its square overflows to +inf
                w[b, 0, 0, 0], x[b, 0, 0], y[b, :m, 0] = 1e100, 1e100, -1e100
            else:  # (float32 inputs cannot overflow the float64 chain)
                w[b, 0, 0, 0] = np.inf
        elif kind == "inf_minus_inf":
            if dtype == "float64":  # finite inputs, a NaN cost: 1e400 - 1e400 in row 1 of the matrix
                w[b, 1, 0, 0], w[b, 1, 1, 0], w[b, 1, 1, 1] = 0.0, 1e200, 1e200
                x[b, 1, 0], x[b, 1, 1] = 1e200, -1e200
                y[b, 0, 0], y[b, 0, 1] = 0.0, 0.0
            else:
                w[b, 1, 1, 0] = np.nan
        elif kind == "shape_0_5":
            shapes[b] = (0, 5)
            w[b, 0, 0, 0] = np.nan  # (nothing of the problem is read)
        elif kind == "bad_outside":
            outside[b, n - 1] = -0.5
            w[b, 0, 0, 0] = np.nan  # (a later check would fail as well)
        elif kind == "nan_coord":
            y[b, m - 1, 0] = np.nan
    for a in (x, y, w, shapes, outside):
        a.setflags(write=False)
    return dict(x=x, y=y, w=w, shapes=shapes, outside=outside, kinds=kinds)
