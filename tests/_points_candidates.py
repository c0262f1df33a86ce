"""What tests/test_points_candidates_nogpu.py and tests/test_points_candidates.py share: the brute-force restatement of
sslap_amd.points_to_ell, the four forms of a limit, and small constructed batches whose rows have 0, k and k + 1
candidates, ties that straddle the k-th key, and costs that are not finite."""
import math

import numpy as np

from sslap_amd import points_to_dense

DTYPES = ("float64", "float32")
FORMS = ("none", "scalar", "per_problem", "per_row")
KEYS = ("cols", "vals", "counts", "rows")


def ell_by_loops(x, y, k, shapes=None, limit=None):
    """points_to_ell as a per-row Python loop over points_to_dense: candidates by Python's own float comparison, the k
    smallest by the tuple (finite?, cost, column), then in column order."""
    c = points_to_dense(x, y)
    B, N, M = c.shape
    lim = None
    if limit is not None:
        lim = np.asarray(limit, dtype=np.float64)
        lim = np.broadcast_to(lim if lim.ndim != 1 else lim[:, None], (B, N))
    cols = np.full((B, N, k), -1, dtype=np.int32)
    vals = np.zeros((B, N, k), dtype=np.float64)
    counts = np.zeros((B, N), dtype=np.int32)
    rows = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(v) for v in np.asarray(shapes)[b])
        if not (1 <= n <= N and 1 <= m <= M):
            continue
        rows[b] = n
        for i in range(n):
            cand = []
            for j in range(m):
                v = float(c[b, i, j])
                if not math.isfinite(v):
                    cand.append((0, 0.0, j))
                elif lim is None or v <= float(lim[b, i]):
                    cand.append((1, v, j))
            counts[b, i] = len(cand)
            kept = sorted(sorted(cand)[:k], key=lambda t: t[2])
            for s, (finite, v, j) in enumerate(kept):
                cols[b, i, s] = j
                vals[b, i, s] = v if finite else math.inf
    return dict(cols=cols, vals=vals, counts=counts, rows=rows)


def same_bytes(got, want):
    """Whether two results agree byte for byte in all four arrays (dtype and shape included)."""
    for key in KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


def grid(shape, dtype, rng, hi=4):
    """Integer-grid coordinates 0 .. hi - 1: equal costs are common."""
    return rng.integers(0, hi, shape).astype(dtype)


def limit_of(form, x, y, rng):
    """A limit in one of the four forms.  The per-row form holds, in turn, a value exactly equal to a cost of the row, a
    value between two costs, a small cost, -0.0, -1.0, a NaN, +inf and a negative NaN; the others a value equal to some cost."""
    if form == "none":
        return None
    c = points_to_dense(x, y)
    B, N, M = c.shape
    finite = np.where(np.isfinite(c), c, 0.0)
    if form == "scalar":
        return float(np.median(finite))
    if form == "per_problem":
        return np.ascontiguousarray(np.median(finite.reshape(B, -1), axis=1))
    lim = np.empty((B, N))
    special = (-0.0, -1.0, np.nan, np.inf, -np.nan)
    for b in range(B):
        for i in range(N):
            kind = (b * N + i) % (len(special) + 3)
            row = np.sort(finite[b, i])
            at = int(rng.integers(0, M))
            if kind == 0:
                lim[b, i] = row[at]  # equal to a cost
            elif kind == 1:
                lim[b, i] = row[at] + 0.25  # between two costs of an integer grid
            elif kind == 2:
                lim[b, i] = row[min(at, 2)]  # a small one: few candidates
            else:
                lim[b, i] = special[kind - 3]
    return lim


def counted_rows(dtype, k, M):
    """x, y (1, 4, 1) / (1, M, 1) and a per-row limit: y_j = j and every x_i = 0, so the costs of a row are j * j and
    the rows have 0, exactly k, k + 1 and M candidates (M >= k + 1)."""
    x = np.zeros((1, 4, 1), dtype=dtype)
    y = np.arange(M, dtype=dtype).reshape(1, M, 1)
    lim = np.array([[-1.0, float((k - 1) ** 2), float(k * k), np.inf]])
    return x, y, lim, np.array([0, k, k + 1, M])


def tied_rows(dtype, M):
    """x, y (1, 2, 2) / (1, M, 2): every y but the last lies at distance 1 from x_0 = (0, 0) (four directions in turn),
    the last ON x_0, so under truncation the last column comes first and the ties go by column; x_1 = (5, 5) sees
    ties of two values."""
    ring = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=dtype)
    y = np.concatenate([ring[np.arange(M - 1) % 4], np.zeros((1, 2), dtype=dtype)])[None]
    x = np.array([[[0, 0], [5, 5]]], dtype=dtype)
    return x, y


def non_finite_batch(dtype):
    """x (4, 3, 2), y (4, 5, 2): problem 0 has a NaN coordinate in row 1, problem 1 an infinite one in column 2,
    problem 2 (float64) coordinates whose squared distance overflows for row 0 and column 4, problem 3 is healthy."""
    rng = np.random.default_rng(5)
    x, y = grid((4, 3, 2), dtype, rng), grid((4, 5, 2), dtype, rng)
    x[0, 1, 1] = np.nan
    y[1, 2, 0] = np.inf
    if dtype == "float64":
        x[2, 0, 0] = 1e200
        y[2, 4, 0] = -1e200
    return x, y
