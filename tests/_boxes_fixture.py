"""Shared by test_boxes_batch.py (GPU) and test_boxes_batch_nogpu.py: draws of box sets, the pairs that exercise every
select of the chain, the definition of boxes_to_dense as a plain loop, the fused chain it must not be, the sort-based
restatement of boxes_to_ell and the CPU side of the verdict table of auction_solve_boxes_batch.

Nothing here runs the code under test: the loops use Python floats (IEEE doubles, one rounding per operator) and
expected_status derives every code from them.
"""
import math
from fractions import Fraction

import numpy as np

OK, INFINITE_VALUE, INFEASIBLE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE, BAD_OUTSIDE, BAD_BOX = 0, 3, 4, 5, 6, 7, 15, 16
DTYPES = ("float64", "float32")
METRICS = ("iou", "giou")
KINDS = ("uniform", "grid")


def draw_boxes(kind, shape, dtype, rng, span=3):
    """Boxes of `shape` = (..., 4), (x1, y1, x2, y2) with x2 >= x1 and y2 >= y1, drawn so that a box overlaps several
    others: centres on a coarse span x span grid of spacing 1 (uniform: jittered, full mantissas; grid: on it) with
    sizes of the order of the spacing (uniform: 0.5 .. 2.5; grid: 1, 2 or 3, one in ten 0, so zero-area boxes, identical
    boxes and exact ties are common)."""
    if kind == "uniform":
        c = rng.integers(0, span, shape[:-1] + (2,)) + rng.uniform(-0.3, 0.3, shape[:-1] + (2,))
        s = rng.uniform(0.5, 2.5, shape[:-1] + (2,))
    elif kind == "grid":
        c = rng.integers(0, span, shape[:-1] + (2,)).astype(np.float64)
        s = rng.integers(1, 4, shape[:-1] + (2,)) * (rng.random(shape[:-1] + (2,)) >= 0.1)
    else:
        raise AssertionError(kind)
    lo, hi = (c - s / 2).astype(dtype), (c + s / 2).astype(dtype)
    return np.concatenate([lo, np.maximum(hi, lo)], axis=-1)


# two pairs (a, b), b nested in a and sharing its upper right corner, for which hull - u comes out negative by rounding:
# the first is exact in float32 (and so serves both types), the second is float64 only
HULL_NEGATIVE = tuple(tuple([float.fromhex(v) for v in box] for box in pair) for pair in (
    (["-0x1.de8176p-5", "-0x1.db61fp-4", "0x1.5d4860p+0", "0x1.28da96p+0"],
     ["0x1.33883ap+0", "-0x1.ce76c8p-4", "0x1.5d4860p+0", "0x1.28da96p+0"]),
    (["0x1.3f3f669406987p+1", "0x1.bb920ca219c08p+2", "0x1.066ec9dc1328cp+2", "0x1.1acf225414d6cp+3"],
     ["0x1.580d8a46c2e68p+1", "0x1.e7d981329da83p+2", "0x1.066ec9dc1328cp+2", "0x1.1acf225414d6cp+3"]),
))

# rows and columns whose pairs take both branches of every select: (row, column) -> what it is
SPECIAL_A = [[1.0, 1.0, 3.0, 2.0],    # 0
             [0.0, 0.0, 4.0, 4.0],    # 1: holds column 2
             [2.0, 2.0, 2.0, 2.0],    # 2: zero area, a point
             [5.0, 1.0, 5.0, 3.0],    # 3: zero area, a segment
             [-0.0, -0.0, 0.0, 0.0]]  # 4: a point at the origin, signed zeros
SPECIAL_B = [[1.0, 1.0, 3.0, 2.0],    # 0: identical to row 0 (cost +0.0)
             [3.0, 1.0, 4.0, 2.0],    # 1: touches row 0 along x = 3 (iw = 0)
             [1.0, 1.0, 2.0, 2.0],    # 2: nested in row 1, and in row 0
             [2.0, 2.0, 2.0, 2.0],    # 3: the point of row 2 (u = 0: the iou = 0 branch; hull = 0: the r = 0 branch)
             [9.0, 9.0, 10.0, 11.0],  # 4: disjoint from every row
             [5.0, 0.0, 5.0, 4.0],    # 5: a segment that holds row 3 (both of zero area)
             [0.0, 0.0, -0.0, -0.0]]  # 6: the origin again, the other signs (min and max of +0.0 and -0.0)


def special_boxes(dtype):
    """(a (1, 7, 4), b (1, 9, 4)): SPECIAL_A and SPECIAL_B, and behind them the HULL_NEGATIVE pairs that dtype holds
    exactly."""
    pairs = HULL_NEGATIVE if dtype == "float64" else HULL_NEGATIVE[:1]
    a = np.array(SPECIAL_A + [p[0] for p in pairs] + [SPECIAL_A[0]] * (2 - len(pairs)), dtype=dtype)[None]
    b = np.array(SPECIAL_B + [p[1] for p in pairs] + [SPECIAL_B[4]] * (2 - len(pairs)), dtype=dtype)[None]
    return a, b


def pair_chain(p, q, giou, fused=False):
    """The chain of boxes_to_dense for row box p and column box q (sequences of 4 numbers) in Python floats, operator by
    operator.  Returns dict(c, flagged, inverted, e_raw): the cost as the chain leaves it, whether a coordinate is not
    finite or an intermediate is infinite, whether either box has x2 < x1 or y2 < y1, and (giou) hull - u before its
    clamp.  fused: the chain a contracting compiler would make of it, finite inputs only -- every a * b +- c in one
    rounding: s = fma(wa, ha, area_b), u = fma(-iw, ih, s), e = fma(cw, ch, -u)."""
    ax1, ay1, ax2, ay2 = (float(v) for v in p)
    bx1, by1, bx2, by2 = (float(v) for v in q)
    inf = math.inf
    flagged = not all(math.isfinite(v) for v in (ax1, ay1, ax2, ay2, bx1, by1, bx2, by2))
    inverted = ax2 < ax1 or ay2 < ay1 or bx2 < bx1 or by2 < by1
    if flagged:  # (nothing below is defined on a NaN)
        return dict(c=math.nan, flagged=True, inverted=inverted, e_raw=math.nan)

    def fma(x, y, z):
        return float(Fraction(x) * Fraction(y) + Fraction(z))

    wa, ha = ax2 - ax1, ay2 - ay1
    wb, hb = bx2 - bx1, by2 - by1
    area_a, area_b = wa * ha, wb * hb
    iw = (ax2 if ax2 < bx2 else bx2) - (ax1 if ax1 > bx1 else bx1)
    ih = (ay2 if ay2 < by2 else by2) - (ay1 if ay1 > by1 else by1)
    seen = [wa, ha, wb, hb, area_a, area_b, iw, ih]
    iw = iw if iw > 0 else 0.0
    ih = ih if ih > 0 else 0.0
    inter = iw * ih
    s = fma(wa, ha, area_b) if fused else area_a + area_b
    seen += [inter, s]
    if any(abs(v) == inf for v in seen):
        return dict(c=math.nan, flagged=True, inverted=inverted, e_raw=math.nan)
    u = fma(-iw, ih, s) if fused else s - inter
    iou = inter / u if u > 0 else 0.0
    if not giou:
        return dict(c=1.0 - iou, flagged=False, inverted=inverted, e_raw=math.nan)
    cw = (ax2 if ax2 > bx2 else bx2) - (ax1 if ax1 < bx1 else bx1)
    ch = (ay2 if ay2 > by2 else by2) - (ay1 if ay1 < by1 else by1)
    hull = cw * ch
    if any(abs(v) == inf for v in (cw, ch, hull)):
        return dict(c=math.nan, flagged=True, inverted=inverted, e_raw=math.nan)
    e_raw = fma(cw, ch, -u) if fused else hull - u
    e = e_raw if e_raw > 0 else 0.0
    r = e / hull if hull > 0 else 0.0
    return dict(c=1.0 - (iou - r), flagged=False, inverted=inverted, e_raw=e_raw)


def dense_by_loops(a, b, shapes=None, metric="iou", fused=False):
    """boxes_to_dense as a plain Python loop: the chain's cost, +inf for a pair that is flagged or holds a bad box and
    beyond the shapes."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    out = np.full((B, N, M), np.inf)
    for p in range(B):
        n, m = (N, M) if shapes is None else (max(int(shapes[p][0]), 0), max(int(shapes[p][1]), 0))
        for i in range(min(n, N)):
            for j in range(min(m, M)):
                r = pair_chain(a[p, i], b[p, j], metric == "giou", fused)
                if not r["flagged"] and not r["inverted"]:
                    out[p, i, j] = r["c"]
    return out


def ell_by_sorting(cost, k, shapes=None, limit=None):
    """boxes_to_ell restated on a cost stack: per row the candidates (not finite, or <= the limit by Python's own float
    comparison), the k smallest by the tuple (finite?, cost, column), then in column order."""
    B, N, M = cost.shape
    lim = None
    if limit is not None:
        lim = np.asarray(limit, dtype=np.float64)
        lim = np.broadcast_to(lim if lim.ndim != 1 else lim[:, None], (B, N))
    cols = np.full((B, N, k), -1, dtype=np.int32)
    vals = np.zeros((B, N, k), dtype=np.float64)
    counts = np.zeros((B, N), dtype=np.int32)
    rows = np.zeros(B, dtype=np.int32)
    for p in range(B):
        n, m = (N, M) if shapes is None else (int(v) for v in np.asarray(shapes)[p])
        if not (1 <= n <= N and 1 <= m <= M):
            continue
        rows[p] = n
        for i in range(n):
            cand = []
            for j in range(m):
                v = float(cost[p, i, j])
                if not math.isfinite(v):
                    cand.append((0, 0.0, j))
                elif lim is None or v <= float(lim[p, i]):
                    cand.append((1, v, j))
            counts[p, i] = len(cand)
            for s, (finite, v, j) in enumerate(sorted(sorted(cand)[:k], key=lambda t: t[2])):
                cols[p, i, s] = j
                vals[p, i, s] = v if finite else math.inf
    return dict(cols=cols, vals=vals, counts=counts, rows=rows)


def outside_rows(outside, B, N):
    """outside in any of its three forms as a (B, N) float64 array."""
    o = np.asarray(outside, dtype=np.float64)
    return np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, N))


def expected_status(a, b, shapes=None, prices=None, outside=None, metric="iou"):
    """(status, matching_size) of every problem: the first check that fails in the order shape, (outside value no entry,)
    a pair that is flagged or an outside value of +inf, a bad box, (n_b > m_b,) price not finite, price sign.  The
    brackets: with / without outside only.  matching_size is min(n_b, m_b) for a good shape without outside, else -1."""
    B, N, M = a.shape[0], a.shape[1], b.shape[1]
    status = np.zeros(B, dtype=np.int32)
    size = np.full(B, -1, dtype=np.int32)
    o = None if outside is None else outside_rows(outside, B, N)
    for p in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[p][0]), int(shapes[p][1]))
        if n < 1 or n > N or m < 1 or m > M:
            status[p] = BAD_SHAPE
            continue
        pairs = [pair_chain(a[p, i], b[p, j], metric == "giou") for i in range(n) for j in range(m)]
        q = None if prices is None else prices[p, :m]
        if o is None:
            size[p] = min(n, m)
        with np.errstate(invalid="ignore"):
            if o is not None and (~(o[p, :n] >= 0)).any():
                status[p] = BAD_OUTSIDE
            elif any(r["flagged"] for r in pairs) or (o is not None and np.isinf(o[p, :n]).any()):
                status[p] = INFINITE_VALUE
            elif any(r["inverted"] for r in pairs):
                status[p] = BAD_BOX
            elif o is None and n > m:
                status[p] = INFEASIBLE
            elif q is not None and not np.isfinite(q).all():
                status[p] = PRICE_NOT_FINITE
            elif q is not None and np.signbit(q).any():
                status[p] = PRICE_NEGATIVE
    return status, size


def verdict_batch(dtype="float64", N=9, M=11, seed=5):
    """dict(a, b, shapes, prices, outside, kinds): a mixed batch for the verdict table.  Healthy problems on the even
    indices; on the odd ones the defects in turn.  Beyond a shape the boxes are NaN, infinite or inverted in places,
    which a kernel that read them would report.  The overflow kinds are float64's (a float32 box cannot overflow the
    float64 chain: there they are an infinite coordinate); overflow_hull overflows under "giou" only."""
    rng = np.random.default_rng(seed)
    kinds = ["ok", "nan_coord", "ok", "inf_coord", "ok", "overflow_width", "ok", "overflow_area", "ok", "overflow_hull",
             "ok", "bad_box_row", "ok", "bad_box_col", "ok", "n_gt_m", "ok", "shape_0_5", "ok", "shape_N1_1", "ok",
             "price_nan", "ok", "price_neg", "ok", "bad_outside", "ok", "nan_and_bad_box", "ok", "inf_outside", "ok",
             "bad_box_and_n_gt_m", "ok", "zero_size"]
    B = len(kinds)
    a, b = draw_boxes("uniform", (B, N, 4), dtype, rng), draw_boxes("uniform", (B, M, 4), dtype, rng)
    shapes = np.empty((B, 2), dtype=np.int32)
    prices = np.zeros((B, M))
    outside = rng.uniform(0.3, 1.2, (B, N))
    f64 = dtype == "float64"
    for p, kind in enumerate(kinds):
        n = int(rng.integers(2, N))
        m = int(rng.integers(n, M))
        shapes[p] = (n, m)
        a[p, n:] = [np.nan, np.inf, -np.inf][p % 3]
        b[p, m:] = [[3.0, 3.0, 1.0, 1.0], [np.nan] * 4, [0.0, np.inf, 1.0, 1.0]][p % 3]  # (the first: a bad box)
        outside[p, n:] = [np.nan, -1.0, np.inf][p % 3]
        if p % 4 == 2:
            prices[p, :m] = rng.uniform(0, 1, m)
        if kind == "nan_coord":
            a[p, n - 1, 3] = np.nan
        elif kind == "inf_coord":
            b[p, 0, 2] = np.inf
        elif kind == "overflow_width":  # x2 - x1 = 2e308 = +inf
            b[p, m - 1] = [-1e308, 0.0, 1e308, 1.0] if f64 else [-np.inf, 0.0, 1.0, 1.0]
        elif kind == "overflow_area":  # 1e200 * 1e200
            a[p, 0] = [0.0, 0.0, 1e200, 1e200] if f64 else [0.0, 0.0, np.inf, 1.0]
        elif kind == "overflow_hull":  # widths, areas and their sum are finite; with giou cw * ch = 1e200 * 1e200
            if f64:
                a[p, 0], b[p, 0] = [0.0, 0.0, 1e200, 1.0], [0.0, 0.0, 1.0, 1e200]
            else:
                b[p, 0, 1] = -np.inf
        elif kind == "bad_box_row":
            a[p, 1] = [2.0, 1.0, 1.5, 3.0]  # x2 < x1
        elif kind == "bad_box_col":
            b[p, m - 1] = [1.0, 3.0, 2.0, 2.5]  # y2 < y1
        elif kind in ("n_gt_m", "bad_box_and_n_gt_m"):
            m2 = min(m, N - 1)
            shapes[p] = (m2 + 1, m2)
            a[p, :m2 + 1] = draw_boxes("uniform", (m2 + 1, 4), dtype, rng)
            b[p, :m2] = draw_boxes("uniform", (m2, 4), dtype, rng)
            outside[p, :m2 + 1] = rng.uniform(0.3, 1.2, m2 + 1)
            if kind == "bad_box_and_n_gt_m":  # BAD_BOX ranks ahead of INFEASIBLE
                a[p, m2] = [1.0, 1.0, 0.0, 2.0]
        elif kind == "shape_0_5":
            shapes[p] = (0, 5)
        elif kind == "shape_N1_1":
            shapes[p] = (N + 1, 1)
        elif kind == "price_nan":
            prices[p, m - 1] = np.nan
            prices[p, 0] = -1.0  # (a later check would fail as well)
        elif kind == "price_neg":
            prices[p, 0] = -0.0
        elif kind == "bad_outside":
            outside[p, n - 1] = -0.5
            a[p, 0, 0] = np.nan  # (a later check would fail as well)
        elif kind == "nan_and_bad_box":  # INFINITE_VALUE ranks ahead of BAD_BOX
            a[p, 0] = [2.0, 1.0, 1.0, 3.0]
            b[p, 1, 0] = np.nan
        elif kind == "inf_outside":
            outside[p, 0] = np.inf
        elif kind == "zero_size":  # zero width and zero height are legal
            a[p, 0], b[p, 0] = [1.0, 1.0, 1.0, 2.0], [1.0, 1.0, 1.0, 1.0]
    for t in (a, b, shapes, prices, outside):
        t.setflags(write=False)
    return dict(a=a, b=b, shapes=shapes, prices=prices, outside=outside, kinds=kinds)


# the status every kind has, by metric and outside mode (the kinds whose code depends on them are spelt out)
def verdict_table(kind, metric, with_outside, f64=True):
    table = dict(ok=OK, zero_size=OK, nan_coord=INFINITE_VALUE, inf_coord=INFINITE_VALUE, overflow_width=INFINITE_VALUE,
                 overflow_area=INFINITE_VALUE, bad_box_row=BAD_BOX, bad_box_col=BAD_BOX, shape_0_5=BAD_SHAPE,
                 shape_N1_1=BAD_SHAPE, price_nan=PRICE_NOT_FINITE, price_neg=PRICE_NEGATIVE, nan_and_bad_box=INFINITE_VALUE,
                 bad_box_and_n_gt_m=BAD_BOX)
    if kind in table:
        return table[kind]
    if kind == "overflow_hull":
        return INFINITE_VALUE if metric == "giou" or not f64 else OK
    if kind == "n_gt_m":
        return OK if with_outside else INFEASIBLE
    if kind == "bad_outside":
        return BAD_OUTSIDE if with_outside else INFINITE_VALUE
    if kind == "inf_outside":
        return INFINITE_VALUE if with_outside else OK
    raise AssertionError(kind)
