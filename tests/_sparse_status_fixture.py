"""The mixed batch of the sparse status-mode tests (tests/test_sparse_batch_status.py on the GPU; pinned on the CPU by
tests/test_sparse_batch_status_nogpu.py): healthy problems on the even indices, and on the odd ones a problem of every
status code auction_solve_sparse_batch(errors="status") can give, in turn, every second round broken in a second way that
a LATER check would report, so that the order of the checks shows.

expected_status derives the code of every problem from numpy and the host matcher (misslap_hopcroft_karp) alone, in the
order include/misslap.h gives for misslap_solve_sparse_batch_status: it never runs the code under test.
"""
import numpy as np

CAP = 2048  # MISSLAP_SPARSE_BATCH_MAX_DIM
INT_MAX = 2**31 - 1
(OK, TOO_FEW_VALUES, _, INFINITE_VALUE, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE, _, NO_ENTRIES, DIVISION_BY_ZERO,
 NEGATIVE_INDEX, ROWS_UNSORTED, ROW_GAP, TOO_LARGE, PRICES_TOO_NARROW) = range(15)
# the codes a sparse problem can get, in the order of the verdict
ORDER = (NO_ENTRIES, DIVISION_BY_ZERO, TOO_FEW_VALUES, INFEASIBLE, NEGATIVE_INDEX, ROWS_UNSORTED, ROW_GAP, INFINITE_VALUE,
         TOO_LARGE, PRICES_TOO_NARROW, PRICE_NOT_FINITE, PRICE_NEGATIVE)
DIMS = (14, 16)  # the caller's bound of the runs with dims: ordinary problems have n <= 12 and m <= 14
P = 14           # columns of the starting prices


def healthy(rng, n, m, per_row=4):
    """n x m (n <= m), per_row stored entries in every row in shuffled column order (duplicates possible), rows
    ascending, a perfect matching of the rows planted."""
    k = min(per_row, m)
    assert 2 <= k and n <= m
    cols = rng.integers(0, m, (n, k)).astype(np.int32)
    cols[:, 0] = rng.permutation(m)[:n]
    cols[0, 1] = m - 1  # the problem has exactly m columns
    cols = rng.permuted(cols, axis=1)
    loc = np.ascontiguousarray(np.stack([np.repeat(np.arange(n, dtype=np.int32), k), cols.ravel()], axis=1))
    return loc, rng.uniform(0, 100, n * k)


def _narrow(loc):
    """rows 0..2 only reach column 0: at most n - 2 rows can be matched"""
    loc = loc.copy()
    loc[loc[:, 0] < 3, 1] = 0
    return loc


def mixed_batch(B=144, seed=0):
    """dict(probs: list of (loc int32 (z, 2), val float64 (z,)), sizes int64 (B, 2), prices float64 (B, P), kinds int (B,)).
    kinds[b] is the defect planted in problem b as a status code with fast=True and dims=DIMS (0: none)."""
    rng = np.random.default_rng(seed)
    probs, sizes = [], np.empty((B, 2), dtype=np.int64)
    prices = np.zeros((B, P))
    kinds = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = int(rng.integers(4, 13))
        m = int(rng.integers(n, 15))
        loc, val = healthy(rng, n, m)
        size = (m, n)  # from_sparse reads size as (M, N)
        if b % 8 == 2:
            prices[b, :m] = rng.uniform(0, 20, m)
        if b % 2 == 1:
            k = b // 2
            kind = ORDER[k % len(ORDER)]
            rnd = k // len(ORDER)
            twice = rnd % 2 == 1  # every second round: a later check would fail as well
            kinds[b] = kind
            if kind == NO_ENTRIES:  # (and a NaN price)
                loc, val = np.zeros((0, 2), dtype=np.int32), np.zeros(0)
                if twice:
                    prices[b, 0] = np.nan
            elif kind == DIVISION_BY_ZERO:  # from_sparse's N is 0 (and a negative column)
                size = (m, 0)
                if twice:
                    loc[3, 1] = -2
            elif kind == TOO_FEW_VALUES:  # fewer entries than N (and an infeasible graph)
                size = (m, loc.shape[0] + 1 + rnd)
                if twice:
                    loc = _narrow(loc)
            elif kind == INFEASIBLE:  # (and an infinity in val)
                loc = _narrow(loc)
                if twice:
                    val[-1] = np.inf
            elif kind == NEGATIVE_INDEX:  # a negative column, or the last entry's row (and rows out of order)
                if rnd % 4 < 2:
                    loc[5, 1] = -1 - rnd
                else:
                    loc[-1, 0] = -3
                if twice:
                    loc[[0, 9]] = loc[[9, 0]]
            elif kind == ROWS_UNSORTED:  # (and a NaN in val)
                loc[[1, 10]] = loc[[10, 1]]
                if twice:
                    val[2] = np.nan
            elif kind == ROW_GAP:  # row 2 has no entry (and a negative price)
                keep = loc[:, 0] != 2
                loc, val = np.ascontiguousarray(loc[keep]), np.ascontiguousarray(val[keep])
                if twice:
                    prices[b, 1] = -1.0
            elif kind == INFINITE_VALUE:  # (and a column beyond the cap)
                val[4] = (np.nan, np.inf, -np.inf)[rnd % 3]
                if twice:
                    loc[0, 1] = CAP
            elif kind == TOO_LARGE:  # beyond dims, beyond the cap, a column whose + 1 does not fit (and a bad price)
                how = rnd % 3
                if how == 0:  # within the cap, column indices >= DIMS[1]: only too wide for P without dims
                    n, m = (16, 20) if twice else (10, 19)
                    loc, val = healthy(rng, n, m)
                    size = (m, n)
                else:
                    loc[0, 1] = CAP if how == 1 else INT_MAX - (rnd % 2)
                if twice:
                    prices[b, 0] = -1.0
            elif kind == PRICES_TOO_NARROW:  # more columns than the prices (and a NaN price)
                n, m = 8, P + 1 + rnd % 2
                loc, val = healthy(rng, n, m)
                size = (m, n)
                if twice:
                    prices[b, 3] = np.nan
            elif kind == PRICE_NOT_FINITE:  # (and a negative price before it)
                prices[b, m - 1] = np.inf if twice else np.nan
                if twice:
                    prices[b, 0] = -2.0
            else:  # PRICE_NEGATIVE: the sign bit
                prices[b, 1] = -0.0 if twice else -3.5
        probs.append((np.ascontiguousarray(loc, dtype=np.int32), np.ascontiguousarray(val)))
        sizes[b] = size
    return dict(probs=probs, sizes=sizes, prices=prices, kinds=kinds)


def pack(probs, pad=0):
    """(loc, val, offsets) of the problems back to back; with pad, `pad` entries before and behind them that no kernel may
    read: +inf values at column indices far beyond every carve.  The packed arrays are then [pad:-pad] of the result."""
    locs = [p[0] for p in probs]
    vals = [p[1] for p in probs]
    if pad:
        guard = np.full((pad, 2), INT_MAX, dtype=np.int32)
        locs = [guard] + locs + [guard]
        vals = [np.full(pad, np.inf)] + vals + [np.full(pad, np.inf)]
    loc = np.ascontiguousarray(np.concatenate(locs), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate(vals))
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in probs])]).astype(np.int64)
    return loc, val, offsets


def graph_is_clean(loc):
    """rows ascending from 0 without a gap and no negative index: what the device guard matches (within the cap)"""
    if loc.shape[0] == 0 or (loc < 0).any():
        return False
    d = np.diff(np.concatenate([[-1], loc[:, 0].astype(np.int64)]))
    return bool(((d == 0) | (d == 1)).all())


def expected_status(probs, sizes=None, prices=None, fast=False, cardinality_check=True, dims=None):
    """(status, matching_size) of every problem, from numpy and the host Hopcroft-Karp: the first check that fails in the
    order of ORDER.  matching_size is -1 where the device guard does not run: no guard in the call, no entries, a graph
    that is not clean, or one beyond the cap."""
    from sslap_amd.check_feasible import cardinality
    Nlim, Mlim = (CAP, CAP) if dims is None else dims
    B = len(probs)
    status = np.zeros(B, dtype=np.int32)
    size = np.full(B, -1, dtype=np.int32)
    for b, (loc, val) in enumerate(probs):
        z = loc.shape[0]
        if z == 0:
            status[b] = NO_ENTRIES
            continue
        rows, cols = loc[:, 0].astype(np.int64), loc[:, 1].astype(np.int64)
        n, m = int(rows.max()) + 1, int(cols.max()) + 1
        N = int(sizes[b][1]) if sizes is not None else n - 1  # (sic: the reference's N without size is the max row)
        clean = graph_is_clean(loc)
        if cardinality_check and clean and n <= CAP and m <= CAP:
            size[b] = cardinality(loc, n, m)
        ok = (rows >= 0) & (cols >= 0)
        prev = np.concatenate([[-1], rows[:-1]])
        p = None if prices is None else prices[b, :min(m, prices.shape[1])]
        if fast and N == 0:
            status[b] = DIVISION_BY_ZERO
        elif z < N:
            status[b] = TOO_FEW_VALUES
        elif size[b] >= 0 and size[b] < n:
            status[b] = INFEASIBLE
        elif not ok.all():
            status[b] = NEGATIVE_INDEX
        elif (rows < prev).any():
            status[b] = ROWS_UNSORTED
        elif (rows > prev + 1).any():
            status[b] = ROW_GAP
        elif not np.isfinite(val).all():
            status[b] = INFINITE_VALUE
        elif n > Nlim or m > Mlim:
            status[b] = TOO_LARGE
        elif prices is not None and m > prices.shape[1]:
            status[b] = PRICES_TOO_NARROW
        elif p is not None and not np.isfinite(p).all():
            status[b] = PRICE_NOT_FINITE
        elif p is not None and np.signbit(p).any():
            status[b] = PRICE_NEGATIVE
    return status, size
