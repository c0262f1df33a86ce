"""Shared by test_dense_signed.py (GPU) and test_dense_signed_nogpu.py: the oracle's result on one packed problem of
dense_to_packed, the verdicts of a finite-mode batch derived from numpy and the host matcher alone, and the draws.

Under entries="finite" an element is an entry iff it is not a NaN.  Problem b of a batch is then the reference's sparse
solver on dense_to_packed(mats, shapes, "finite")[b]: auction_solve(loc=loc_b, val=val_b, cardinality_check=False), given
size=(., n_b) so that `fast` means eps = 1 / n_b as in every dense call (from_sparse without a size takes the largest row
index for N, auction_.pyx:594).
"""
import numpy as np

from tests._batch_shapes import sparse_expect

OK, TOO_FEW_VALUES, EMPTY_ROW, INFINITE_VALUE, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE = range(8)
BAD_OUTSIDE = 15


def packed_expect(loc, val, problem, n, p0=None, **kw):
    """What the oracle gives for one packed problem of n rows (plain values, as sparse_expect returns them)."""
    return sparse_expect(loc, val, problem, size=(int(loc[:, 1].max()) + 1, n), p0=p0, cardinality_check=False, **kw)


def expected_status(packed, shapes, stack, prices=None, cardinality_check=True):
    """(status, matching_size) of a finite-mode batch from its packed problems: the first check that fails in the order
    shape, entry count, empty row, infinity, matching guard, price not finite, price sign.  packed: dense_to_packed's
    list; shapes: (B, 2); stack: (N, M)."""
    from sslap_amd.check_feasible import cardinality
    N, M = stack
    B = len(packed)
    status, size = np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    for b, (loc, val) in enumerate(packed):
        n, m = int(shapes[b][0]), int(shapes[b][1])
        if n < 1 or n > N or m < 1 or m > M:
            status[b] = BAD_SHAPE
            continue
        card = -1
        if cardinality_check:
            card = cardinality(loc, n, m) if len(loc) else 0
        size[b] = card
        p = None if prices is None else prices[b, :m]
        if len(loc) < n:
            status[b] = TOO_FEW_VALUES
        elif len(np.unique(loc[:, 0])) < n:
            status[b] = EMPTY_ROW
        elif np.isinf(val).any():
            status[b] = INFINITE_VALUE
        elif cardinality_check and card < n:
            status[b] = INFEASIBLE
        elif p is not None and not np.isfinite(p).all():
            status[b] = PRICE_NOT_FINITE
        elif p is not None and np.signbit(p).any():
            status[b] = PRICE_NEGATIVE
    return status, size


def signed_ints(rng, n, m, lo=-20, hi=21, hole_share=0.3):
    """An n x m (n <= m) matrix of integer values in [lo, hi) with NaN holes; a random injection of the rows into the
    columns keeps its entries, so the problem stays feasible."""
    v = rng.integers(lo, hi, (n, m)).astype(np.float64)
    planted = rng.permutation(m)[:n]
    holes = rng.random((n, m)) < hole_share
    holes[np.arange(n), planted] = False
    v[holes] = np.nan
    return v


def signed_uniform(rng, n, m, hole_share=0.2):
    """Uniform doubles in [-50, 50) with NaN holes that keep a planted injection."""
    v = rng.uniform(-50, 50, (n, m))
    planted = rng.permutation(m)[:n]
    holes = rng.random((n, m)) < hole_share
    holes[np.arange(n), planted] = False
    v[holes] = np.nan
    return v
