"""Shared by test_sparse_outside.py (GPU) and test_sparse_outside_nogpu.py: ragged packed problems with rows without
entries, the same problems as an ELL stack padded with holes, the verdict of auction_solve_sparse_batch(outside=) restated
on the CPU, and the mixed batch of healthy and defective problems."""
import functools

import numpy as np

from tests._batch_shapes import dense_values

INT_MAX = 2**31 - 1
CAP = 2048
(OK, INFINITE_VALUE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE, NO_ENTRIES, NEGATIVE_INDEX, ROWS_UNSORTED, TOO_LARGE,
 PRICES_TOO_NARROW) = 0, 3, 5, 6, 7, 8, 10, 11, 13, 14


def ragged(rng, lens, m, kind="ints"):
    """One packed problem: row i holds lens[i] entries (0: a row without any) at distinct columns below m, in a random
    stored order; rows ascending.  Returns (loc int32 (nnz, 2), val float64 (nnz,))."""
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.concatenate([rng.choice(m, k, replace=False) for k in lens] + [np.zeros(0, dtype=np.int64)])
    loc = np.ascontiguousarray(np.stack([rows, cols], axis=1), dtype=np.int32).reshape(-1, 2)
    return loc, dense_values(kind, (loc.shape[0],), rng)


def pack(probs):
    loc = np.ascontiguousarray(np.concatenate([p[0].reshape(-1, 2) for p in probs]), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate([p[1] for p in probs]), dtype=np.float64)
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in probs])]).astype(np.int64)
    return loc, val, offsets


def rows_of(probs, sizes=None):
    """n_b of every problem: sizes[b, 1], else the last stored row + 1."""
    if sizes is not None:
        return [int(s[1]) for s in sizes]
    return [int(lo[-1, 0]) + 1 if len(lo) else 0 for lo, _ in probs]


def to_ell(probs, ns, N):
    """The same problems as an ELL stack (B, N, K): row i's entries in stored order in slots 0 .. len - 1, the rest holes
    (column -1, value NaN); K = the longest row (at least 1).  Returns (cols int64, vals, rows int32)."""
    K = max([1] + [int(np.bincount(lo[:, 0]).max()) for lo, _ in probs if len(lo)])
    cols, vals = np.full((len(probs), N, K), -1, dtype=np.int64), np.full((len(probs), N, K), np.nan)
    for b, (lo, va) in enumerate(probs):
        slot = np.zeros(N, dtype=np.int64)
        for (i, j), v in zip(lo, va):
            cols[b, i, slot[i]], vals[b, i, slot[i]] = j, v
            slot[i] += 1
    return cols, vals, np.array(ns, dtype=np.int32)


def expected_status(loc, val, offsets, sizes, outside, dims, prices):
    """(status (B,), counts (B, 3) = the record's n_rows, n_cols, nnz) of the outside mode, from its definition: the
    first check that fails, in the order NO_ENTRIES, NEGATIVE_INDEX, ROWS_UNSORTED, BAD_SHAPE, INFINITE_VALUE, TOO_LARGE,
    PRICES_TOO_NARROW, PRICE_NOT_FINITE, PRICE_NEGATIVE.  outside: a float, (B,) or (B, P)."""
    B = len(offsets) - 1
    Nmax, Mmax = dims
    status, counts = np.zeros(B, dtype=np.int32), np.zeros((B, 3), dtype=np.int64)
    o = np.asarray(outside, dtype=np.float64)
    for b in range(B):
        lo, va = loc[offsets[b]:offsets[b + 1]].astype(np.int64), val[offsets[b]:offsets[b + 1]]
        nnz = len(lo)
        if nnz == 0 and sizes is None:
            status[b] = NO_ENTRIES
            continue
        if (lo < 0).any():
            status[b] = NEGATIVE_INDEX
            continue
        if (np.diff(lo[:, 0]) < 0).any():
            status[b] = ROWS_UNSORTED
            continue
        last = int(lo[-1, 0]) if nnz else -1
        n = int(sizes[b][1]) if sizes is not None else last + 1
        if sizes is not None and n < max(1, last + 1):
            status[b] = BAD_SHAPE
            continue
        m = int(lo[:, 1].max()) + 1 if nnz else 0
        counts[b] = (min(n, INT_MAX), min(m + n, INT_MAX), nnz + n)
        read = min(n, Nmax)  # the rows whose outside value is read
        ob = np.broadcast_to(o if o.ndim == 0 else o[b] if o.ndim == 1 else o[b, :read], (read,))
        if not (np.isfinite(va).all() and np.isfinite(ob).all()):
            status[b] = INFINITE_VALUE
        elif n > Nmax or m > Mmax:
            status[b] = TOO_LARGE
        elif prices is not None and prices.shape[1] < m:
            status[b] = PRICES_TOO_NARROW
        elif prices is not None and not np.isfinite(prices[b, :m]).all():
            status[b] = PRICE_NOT_FINITE
        elif prices is not None and np.signbit(prices[b, :m]).any():
            status[b] = PRICE_NEGATIVE
    return status, counts


V_DIMS, V_P = (16, 30), 26


@functools.lru_cache(maxsize=None)
def mixed(with_sizes):
    """A healthy problem (some with rows without entries) at every even index, at every odd index one with a defect
    (kinds[b]: the first check it fails).  with_sizes: BAD_SHAPE can occur and NO_ENTRIES cannot; without: the reverse."""
    rng = np.random.default_rng([61, int(with_sizes)])
    Nmax, Mmax = V_DIMS
    probs, ns, kinds, outs, bad_price = [], [], [], [], []

    def healthy(n=None, gaps=True):
        n = int(rng.integers(3, Nmax - 2)) if n is None else n
        lens = rng.integers(1, 6, n)
        if gaps:
            lens[rng.random(n) < 0.3] = 0
        lens[-1] = max(lens[-1], 1)  # (the last row is stored: n_b is the same with and without sizes)
        return ragged(rng, lens, 22, "uniform")

    def add(p, kind, n=None, price=None):
        lo = p[0]
        n_true = int(lo[-1, 0]) + 1 if len(lo) and lo[-1, 0] >= 0 else 0
        probs.append(p)
        ns.append(n_true + int(rng.integers(0, 3)) if n is None else n)  # (trailing rows without entries, named by sizes)
        kinds.append(kind)
        row = np.full(Nmax + 3, np.nan)  # (beyond n_b: never read)
        read = min(max(ns[-1] if with_sizes else n_true, 0), Nmax)
        row[:read] = rng.uniform(10, 60, read)
        outs.append(row)
        bad_price.append(price)

    def edit(fn, kind, n=9, price=None, gaps=True):
        """A healthy problem of 9 rows (the last one stored) with a defect; n: what sizes says of its rows."""
        lo, va = healthy(n=9, gaps=gaps)
        fn(lo, va)
        add((lo, va), kind, n=n, price=price)

    def none(lo, va):
        pass

    def set_(what, k, v):
        def fn(lo, va):
            if what == "val":
                va[k] = v
            else:
                lo[k, 0 if what == "row" else 1] = v
        return fn

    def unsorted(lo, va):
        lo[[0, -1]] = lo[[-1, 0]]

    def bad_outside(value):
        edit(none, INFINITE_VALUE)
        outs[-1][int(rng.integers(0, 9))] = value

    plans = [lambda: edit(set_("col", 2, -1), NEGATIVE_INDEX), lambda: edit(set_("row", 0, -3), NEGATIVE_INDEX),
             lambda: edit(unsorted, ROWS_UNSORTED),
             lambda: edit(set_("val", 3, np.nan), INFINITE_VALUE), lambda: edit(set_("val", 0, -np.inf), INFINITE_VALUE),
             lambda: bad_outside(np.nan), lambda: bad_outside(np.inf),
             lambda: edit(set_("col", 1, Mmax), TOO_LARGE), lambda: edit(set_("col", 4, INT_MAX), TOO_LARGE),
             lambda: edit(set_("col", 1, V_P + 1), PRICES_TOO_NARROW),
             lambda: edit(none, PRICE_NOT_FINITE, price=np.nan),
             lambda: edit(none, PRICE_NOT_FINITE, price=np.inf),
             lambda: edit(none, PRICE_NEGATIVE, price=-0.0),
             lambda: edit(none, PRICE_NEGATIVE, price=-3.0)]
    if with_sizes:
        plans += [lambda: edit(none, BAD_SHAPE, n=5), lambda: edit(none, BAD_SHAPE, n=-4),
                  lambda: add((np.zeros((0, 2), dtype=np.int32), np.zeros(0)), BAD_SHAPE, n=0),
                  lambda: add((np.zeros((0, 2), dtype=np.int32), np.zeros(0)), OK, n=4),  # no entries, rows named: solved
                  lambda: edit(none, TOO_LARGE, n=Nmax + 1)]
    else:
        plans += [lambda: add((np.zeros((0, 2), dtype=np.int32), np.zeros(0)), NO_ENTRIES),
                  lambda: edit(set_("row", -1, Nmax), TOO_LARGE)]
    for plan in plans:
        add(healthy(), OK)
        plan()
    B = len(probs)
    loc, val, offsets = pack(probs)
    sizes = np.stack([np.full(B, 99), np.array(ns)], axis=1).astype(np.int64) if with_sizes else None  # (sizes[:, 0]: not read)
    prices = rng.uniform(0, 5, (B, V_P))
    prices[::4] = 0.0
    for b, (lo, _) in enumerate(probs):
        cols = lo[:, 1][(lo[:, 1] >= 0) & (lo[:, 1] < V_P)]
        top = int(cols.max()) + 1 if len(cols) else 0
        if bad_price[b] is not None:
            prices[b, top - 1] = bad_price[b]
        if kinds[b] == OK:  # what lies beyond a problem's real columns is not its price
            prices[b, top:] = np.nan if b % 8 == 0 else -1.0
    for a in (loc, val, offsets, prices):
        a.setflags(write=False)
    return dict(probs=probs, loc=loc, val=val, offsets=offsets, sizes=sizes, outside=np.stack(outs), prices=prices,
                kinds=np.array(kinds, dtype=np.int32))
