"""Shared by test_builder_edges.py (GPU) and test_builder_edges_nogpu.py: the cases that put the three candidate builders
(k_points_candidates, k_points_whiten_candidates, k_boxes_batch_candidates) where no other test puts them -- the ends
of the key range and neighbouring keys in the bisection of the truncated path, and batches larger than the grid's y
extent, where a workgroup takes a second problem.

Nothing here runs the code under test and nothing here is the expected result: that is always points_to_ell /
boxes_to_ell.  bisect_model restates the kernel's loop on a row's integer keys so that every case can be held to the
situation it claims (which key T the loop ends on, by which exit, after how many steps).  numpy only.
"""
import functools
import math

import numpy as np

from sslap_amd import boxes_to_dense, boxes_to_ell, points_to_dense, points_to_ell

KEYS = ("cols", "vals", "counts", "rows")
KEY_INF = 0x7ff0000000000000  # the bits of +inf: the limit key without a limit, and the largest key (that of DBL_MAX)
FAMILIES = ("points", "whitened", "boxes")
# (family, coordinate type, metric): the eight instances the bisection cases run on
INSTANCES = (("points", "float64", None), ("points", "float32", None), ("whitened", "float64", None),
             ("whitened", "float32", None), ("boxes", "float64", "iou"), ("boxes", "float64", "giou"),
             ("boxes", "float32", "iou"), ("boxes", "float32", "giou"))
ROWS = 4  # rows per problem of a stacked batch: one workgroup, the case at wavefronts 0 and 3, fillers at 1 and 2
STACK_M = 24  # the common column count every case is padded to by `shapes`
ADJACENT_M = 12
SEARCH_SEED, SEARCH_TRIALS = 20, 16384


# ---- the kernel's keys and its loop, restated

def cost_keys(costs):
    """The keys of points_candidate_key for a row of float64 costs, as Python integers: 0 for a cost that is not
    finite, bits(cost) + 1 else (a finite cost is >= +0.0, so its bits order as it does)."""
    c = np.ascontiguousarray(costs, dtype=np.float64)
    assert not np.signbit(c[np.isfinite(c)]).any()
    return [int(u) + 1 if math.isfinite(v) else 0 for u, v in zip(c.view(np.uint64).tolist(), c.tolist())]


def limit_key(limit):
    """The key of points_limit_key: the largest key a candidate may have.  None and +inf admit every finite cost, -0.0
    admits +0.0 (key 1), a negative value and every NaN admit key 0 only."""
    if limit is None:
        return KEY_INF
    u = int(np.array([limit], dtype=np.float64).view(np.uint64)[0])
    if u > KEY_INF:
        return 1 if u == 0x8000000000000000 else 0
    return KEY_INF if u == KEY_INF else u + 1


def bisect_model(keys, K, lim):
    """The loop of points_candidates_truncate (and of its two copies) on a row's keys, in Python integers:

        lo = 0, hi = lim
        while lo < hi:   mid = lo + ((hi - lo) >> 1);  le = #{key <= mid}
                         le == K: lo = mid, ties = K, stop      ("early")
                         le >  K: hi = mid
                         le <  K: lo = mid + 1, under = le
        ties = K - under unless the early exit set it

    Returns (T, under, ties, steps, exit): T the final lo, the key whose candidates are kept in column order up to
    `ties` of them behind all `under` below it; exit is "early", "converged" (the loop ran and ended with lo == hi) or
    "none" (the row has at most K candidates and the kernel never enters this path: T is None; or lo == hi on entry,
    which is lim == 0: T = 0).  It is not the expected result; the cases use it to prove what they claim to be."""
    count = sum(1 for k in keys if k <= lim)
    if count <= K:
        return None, count, 0, 0, "none"
    lo, hi, under, ties, steps, how = 0, lim, 0, 0, 0, "none"
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        steps += 1
        le = sum(1 for k in keys if k <= mid)
        if le == K:
            lo, ties, how = mid, K, "early"
            break
        if le > K:
            hi = mid
        else:
            lo, under = mid + 1, le
        how = "converged"
    if not ties:
        ties = K - under
    return lo, under, ties, steps, how


def cap(N):
    """The largest gridDim.y of a builder launch for stacks of N rows.  Restated from points_candidates_grid
    (csrc/abi_points_candidates.hpp): min(65535, 2^22 / gridDim.x) with gridDim.x = ceil(N / 4), at least 1."""
    return max(1, min(65535, 2 ** 22 // -(-N // 4)))


# ---- one row against M columns: the cases

def _case(name, family, dtype, x, y, K, limit, metric=None, w=None, **claim):
    """A case: row `x` (D,) against columns `y` (M, D) (boxes: D = 4) with K and the row's limit (None: no limit);
    claim: what test_builder_edges_nogpu.py proves of it with bisect_model."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    assert x.ndim == 1 and y.ndim == 2 and y.shape[1] == x.shape[0] and y.shape[0] <= STACK_M
    return dict(name=name, family=family, dtype=dtype, metric=metric, x=x, y=y, w=w, K=K, limit=limit, claim=claim)


def _whiten_2i(D, dtype):
    """W = 2 I, NaN above the diagonal (never read)."""
    w = np.full((D, D), np.nan, dtype=dtype)
    w[np.tril_indices(D)] = 0.0
    w[np.arange(D), np.arange(D)] = 2.0
    return w


def case_costs(case):
    """The float64 (M,) costs of the case's row by the family's definition (points_to_dense / boxes_to_dense)."""
    x, y = case["x"][None, None, :], case["y"][None]
    if case["family"] == "boxes":
        return boxes_to_dense(x, y, metric=case["metric"])[0, 0]
    w = None if case["w"] is None else case["w"][None, None]
    return points_to_dense(x, y, whiten=w)[0, 0]


def case_model(case):
    """bisect_model on the case's own keys, K and limit."""
    return bisect_model(cost_keys(case_costs(case)), case["K"], limit_key(case["limit"]))


LADDER = {
    # one row at x = 0 against these columns: the costs are their squares.  float64: +0.0, 2^-1074 = 5e-324 (the
    # smallest subnormal: key 2), 2^-1000, 1e-200, 1e-20, 1, 1e20, 1e200, 1.69e308, an overflow and a NaN (both key 0)
    "float64": [0.0, 2.0 ** -537, 2.0 ** -500, 1e-100, 1e-10, 1.0, 1e10, 1e100, 1.3e154, 1.4e154, np.nan],
    # float32 coordinates cannot reach the ends of the float64 range: the smallest subnormal and the largest finite
    # float32 (costs 2^-298 and 1.2e77), and an infinite and a NaN coordinate for key 0
    "float32": [0.0, 2.0 ** -149, 2.0 ** -100, 1e-30, 1e-10, 1.0, 1e10, 1e30, 3.4028234663852886e38, np.inf, np.nan],
}


def ladder_columns(family, dtype):
    """The (M, 1) columns of the key-range ladder.  Whitened (W = 2 I): the columns halved, so that (2 d)^2 is the very
    cost of the plain ladder -- halving is exact for all but the float32 subnormal, which stays (its cost is 2^-296)."""
    y = np.array(LADDER[dtype], dtype=dtype)
    if family == "whitened":
        half = y / np.asarray(2, dtype=dtype)
        if dtype == "float32":
            half[1] = y[1]
        y = half
    return y[:, None]


def ladder_cases(family, dtype, K):
    """The ladder at K (1 .. 21).
    K <= 10, the 11 columns: without a limit, with every finite cost of the row as the limit (hi starts on every key)
    and with +inf.  The finite keys of this row are all different, so the loop ends by the early exit on some midpoint
    between the K-th key and the next (bisect_model's T is that midpoint, not a key).
    Every K, every column stored twice (22 columns): for odd K the K-th and (K+1)-th keys are one key and the loop can
    only converge onto it -- T = key 0 (K = 1, 3), key 1 (the cost +0.0; K = 5), key 2 (float64: the smallest subnormal;
    K = 7), ... and the largest key of the row (K = 21) in turn --, without a limit and with the K-th cost itself as
    the limit, where T = lim (-1.0 where that cost is not finite: lim = 0 and the loop does not run)."""
    y = ladder_columns(family, dtype)
    w = _whiten_2i(1, dtype) if family == "whitened" else None
    out = []
    if K < len(y):
        base = _case("ladder", family, dtype, [0.0], y, K, None, w=w)
        costs = case_costs(base)
        finite = np.sort(costs[np.isfinite(costs)])
        out.append(dict(base, name=f"ladder K={K} no limit", claim=dict(truncated=True)))
        for v in finite.tolist() + [math.inf]:
            out.append(dict(base, name=f"ladder K={K} limit={v!r}", limit=v, claim=dict()))
    twice = _case("ladder twice", family, dtype, [0.0], np.repeat(y, 2, axis=0), K, None, w=w)
    kth = float(np.sort(np.where(np.isfinite(case_costs(twice)), case_costs(twice), -1.0))[K - 1])
    out.append(dict(twice, name=f"ladder twice K={K} no limit", claim=dict(truncated=True, twice=True)))
    out.append(dict(twice, name=f"ladder twice K={K} limit=K-th", limit=kth, claim=dict(twice=True, t_is_lim=True)))
    return out


def adjacent_columns(family, dtype, metric=None):
    """(x, y) whose M = 12 sorted keys differ by exactly 1 each (float32 boxes: see searched_boxes).
    points / whitened, D = 2: x = (0, 0), y_j = (1, sqrt(j) 2^-26): the costs are 1 + j 2^-52 (whitened: 4 + j 2^-50),
    consecutive doubles.  boxes, float64: a = (0, 0, 1, 1), b_j = (1 - j 2^-52, 0, 2 - j 2^-52, 1): an overlap of width
    j 2^-52 in a union of 2 - j 2^-52, the costs 1 - j 2^-53, consecutive doubles below 1 (no hull excess: both
    metrics)."""
    j = np.arange(ADJACENT_M, dtype=np.float64)
    if family != "boxes":
        return np.zeros(2), np.stack([np.ones(ADJACENT_M), np.sqrt(j) * 2.0 ** -26], axis=1)
    if dtype == "float32":
        return searched_boxes(metric)[:2]
    e = j * 2.0 ** -52
    return np.array([0.0, 0.0, 1.0, 1.0]), np.stack([1.0 - e, np.zeros(ADJACENT_M), 2.0 - e, np.ones(ADJACENT_M)], axis=1)


@functools.lru_cache(maxsize=None)
def searched_boxes(metric):
    """float32 boxes whose costs come as close as a seeded search finds: (a (4,), b (12, 4), position, gap).  The
    float64 recipe of adjacent_columns has no float32 form (2 - j 2^-52 is no float32, and with float32 steps the
    smallest gap between two keys of a row is about 2^28), so the search draws SEARCH_TRIALS rows of 12 boxes
    b = (1 - p 2^-24, r 2^-24, 2 - q 2^-23, 1 - s 2^-24) with p in 1 .. 63 and q, r, s in 0 .. 63 against
    a = (0, 0, 1, 1) from default_rng(SEARCH_SEED) and keeps the row with the smallest positive difference between two
    keys that are neighbours in the sorted row.  Found: a gap of 8 under "iou" and of 16 under "giou" (asserted in
    test_builder_edges_nogpu.py).  position: the 0-based rank of the lower of the two keys in the sorted row, so K =
    position + 1 puts the K-th and (K+1)-th keys there.  The claim is only that: distinct, and neighbours in the row."""
    rng = np.random.default_rng(SEARCH_SEED)
    shape = (SEARCH_TRIALS, ADJACENT_M)
    p, q, r, s = rng.integers(1, 64, shape), rng.integers(0, 64, shape), rng.integers(0, 64, shape), rng.integers(0, 64, shape)
    b = np.stack([1.0 - p * 2.0 ** -24, r * 2.0 ** -24, 2.0 - q * 2.0 ** -23, 1.0 - s * 2.0 ** -24], axis=2).astype(np.float32)
    a = np.tile(np.array([0.0, 0.0, 1.0, 1.0], dtype=np.float32), (SEARCH_TRIALS, 1, 1))
    cost = boxes_to_dense(a, b, metric=metric)[:, 0, :]
    assert np.isfinite(cost).all()
    keys = np.sort(cost.view(np.uint64).astype(np.int64), axis=1)
    gaps = np.diff(keys, axis=1)
    gaps = np.where(gaps > 0, gaps, np.iinfo(np.int64).max)
    t, at = np.unravel_index(np.argmin(gaps), gaps.shape)
    return a[t, 0], b[t], int(at), int(gaps[t, at])


def adjacent_cases(family, dtype, K, metric=None):
    """The adjacent keys at K (1 .. 11), three cases: without a limit, where the loop walks the whole key range down to
    two neighbours; with the (K+1)-th cost as the limit, where hi starts one above T; and, without a limit, with the
    column of the K-th cost stored once more as column 0, so that K - 1 keys lie below T, two ON it and the next one
    above it -- and the first of the two at T comes ahead of every column below T: a compaction that kept one too many
    at T would push the last of those out of the K slots.
    Where the K-th and (K+1)-th keys differ, some midpoint holds exactly K (every one from the K-th key up to the next
    key), and hi can only come down to T through a midpoint ON T, which is such a one: the first two cases can only end
    by the early exit, late (the first, after >= 50 steps, with lo == mid == T where hi - lo == 1).  The third has no
    such midpoint and ends by convergence onto T, between two keys at T - 1 and T + 1."""
    x, y = adjacent_columns(family, dtype, metric)
    w = _whiten_2i(2, dtype) if family == "whitened" else None
    base = _case("adjacent", family, dtype, x, y, K, None, metric=metric, w=w)
    order = np.argsort(case_costs(base), kind="stable")
    nxt = float(case_costs(base)[order[K]])
    tied = _case("adjacent", family, dtype, x, np.concatenate([y[order[K - 1]][None], y]), K, None, metric=metric, w=w)
    searched = family == "boxes" and dtype == "float32"
    claim = dict(neighbours=True) if searched else dict(adjacent=True)
    return [dict(base, name=f"adjacent K={K} no limit", claim=dict(claim, truncated=True)),
            dict(base, name=f"adjacent K={K} limit=(K+1)-th", limit=nxt, claim=dict(claim, truncated=True)),
            dict(tied, name=f"adjacent K={K} K-th twice", claim=dict(claim, truncated=True, exit="converged"))]


def _far_boxes(count):
    """`count` healthy boxes that overlap (0, 0, 1, 1) in part, all different"""
    t = 0.25 + np.arange(count) / 16.0
    return np.stack([t, np.zeros(count), t + 1.0, np.ones(count)], axis=1)


def early_case(family, dtype, K, metric=None):
    """A row whose first midpoint has exactly K keys at or below it, with more than K candidates: the early exit at
    step 1.  points / whitened (no limit: the first midpoint is the key of a cost just under 1.5): K columns ON the
    row's point and three at distance 2 (cost 4; whitened 16).  boxes (costs never reach 1.5: limit = 1.0, whose first
    midpoint lies at 2^-512): K columns identical to the row's box (cost +0.0) and three that overlap it in part."""
    if family == "boxes":
        a = np.array([0.0, 0.0, 1.0, 1.0])
        y = np.concatenate([_far_boxes(2), np.tile(a, (K, 1)), _far_boxes(3)[2:]])
        return _case(f"early K={K}", family, dtype, a, y, K, 1.0, metric=metric, exit="early", steps=1, truncated=True)
    y = np.concatenate([[[2.0, 0.0], [0.0, 2.0]], np.zeros((K, 2)), [[-2.0, 0.0]]])
    w = _whiten_2i(2, dtype) if family == "whitened" else None
    return _case(f"early K={K}", family, dtype, [0.0, 0.0], y, K, None, w=w, exit="early", steps=1, truncated=True)


def many_non_finite_cases(family, dtype, K, metric=None):
    """A row with K + 2 costs that are not finite among three finite ones: limit = -1.0 (lim = 0: the loop does not run,
    T = 0) and no limit (T = 0 by bisection).  points / whitened: NaN and infinite coordinates in turn (float64: an
    overflowing one as well); boxes: inverted boxes and NaN coordinates in turn."""
    if family == "boxes":
        x = np.array([0.0, 0.0, 1.0, 1.0])
        bad = [[1.0, 0.0, 0.5, 1.0], [np.nan, 0.0, 1.0, 1.0], [0.0, 1.0, 1.0, 0.25], [0.0, 0.0, 1.0, np.nan]]
        good = _far_boxes(3)
    else:
        x = np.zeros(2)
        bad = [[np.nan, 0.0], [1.0, np.inf], [-np.inf, 2.0]] + ([[1.0, 1.4e154]] if dtype == "float64" else [])
        good = np.array([[1.0, 0.0], [0.0, 0.0], [1.0, 1.0]])
    y = np.concatenate([good[:1], [bad[c % len(bad)] for c in range(K + 2)], good[1:]])
    w = _whiten_2i(2, dtype) if family == "whitened" else None
    base = _case("non-finite", family, dtype, x, y, K, None, metric=metric, w=w)
    return [dict(base, name=f"non-finite K={K} limit=-1", limit=-1.0, claim=dict(T=0, exit="none", truncated=True)),
            dict(base, name=f"non-finite K={K} no limit", claim=dict(T=0, truncated=True, bisected=True))]


def stack_ks(group):
    return range(1, 2 * len(LADDER["float64"])) if group == "ladder" else range(1, ADJACENT_M)


def stack_groups(family):
    """The stacks of a family: cases of one D go into one call."""
    return ("adjacent",) if family == "boxes" else ("ladder", "adjacent")


def stack_cases(family, dtype, metric, group, K):
    """The cases of one stacked batch: "ladder" (D = 1) or "adjacent" (D = 2 / boxes: the adjacent keys, the early exit
    and the many non-finite costs)."""
    if group == "ladder":
        return ladder_cases(family, dtype, K)
    return adjacent_cases(family, dtype, K, metric) + [early_case(family, dtype, K, metric)] + \
        many_non_finite_cases(family, dtype, K, metric)


def stack(cases, no_limit_only=False):
    """The cases of one family, type, D and K as one batch: dict(x (B, 4, D), y (B, 16, D), w or None, shapes (B, 2),
    limit (B, 4) or None, K, cases).  Problem b is case b: its row at rows 0 and 3 of the problem (wavefronts 0 and 3
    of the one workgroup) under its own limit -- no limit is +inf here, the same key -- and twice more at rows 1 and 2
    under the limits -1.0 and NaN, which admit the non-finite costs only; the columns beyond the case's own M are NaN
    and cut off by shapes.  no_limit_only: the cases without a limit alone, with limit None."""
    if no_limit_only:
        cases = [c for c in cases if c["limit"] is None]
    first = cases[0]
    B, D, dtype = len(cases), first["x"].shape[0], first["dtype"]
    assert all(c["K"] == first["K"] and c["family"] == first["family"] and c["dtype"] == dtype and
               c["metric"] == first["metric"] for c in cases)
    x = np.empty((B, ROWS, D), dtype=dtype)
    y = np.full((B, STACK_M, D), np.nan, dtype=dtype)
    shapes = np.empty((B, 2), dtype=np.int32)
    limit = np.empty((B, ROWS))
    for b, c in enumerate(cases):
        x[b] = c["x"]
        y[b, :len(c["y"])] = c["y"]
        shapes[b] = (ROWS, len(c["y"]))
        own = math.inf if c["limit"] is None else c["limit"]
        limit[b] = (own, -1.0, np.nan, own)
    w = None
    if first["w"] is not None:
        w = np.ascontiguousarray(np.broadcast_to(first["w"], (B, ROWS, D, D)))
    return dict(family=first["family"], metric=first["metric"], x=x, y=y, w=w, shapes=shapes,
                limit=None if no_limit_only else limit, K=first["K"], cases=cases)


def to_ell(family, x, y, K, shapes=None, limit=None, w=None, metric=None):
    """The definition of the family on a batch: points_to_ell / boxes_to_ell."""
    if family == "boxes":
        return boxes_to_ell(x, y, K, shapes, limit, metric)
    return points_to_ell(x, y, K, shapes, limit, whiten=w)


def stack_to_ell(s):
    return to_ell(s["family"], s["x"], s["y"], s["K"], s["shapes"], s["limit"], s["w"], s["metric"])


# ---- batches past the grid's y extent

LAP_P = 7  # distinct problems of a lap batch: coprime to both caps (65535 = 3 5 17 257 and powers of two)


def _draw(family, shape, dtype, rng):
    """Integer-grid coordinates (ties are common); boxes: x2 >= x1 and y2 >= y1 on that grid."""
    if family != "boxes":
        return rng.integers(0, 4, shape).astype(dtype)
    lo = rng.integers(0, 4, shape[:-1] + (2,))
    return np.concatenate([lo, lo + rng.integers(0, 3, shape[:-1] + (2,))], axis=-1).astype(dtype)


def lap_batch(family, dtype, B, N, M, K, metric=None, D=2, seed=9):
    """B problems for a launch whose grid is shorter than B: LAP_P = 7 distinct small problems, repeated in turn
    (problem b is distinct problem b % 7), so that a workgroup's second problem differs from its first whatever the
    cap.  The shapes are (N, M), (1, 1), (N, M - 1), (N, M), the bad shape (N + 1, M) -- which only a device array can
    carry --, (N - 1 or 1, M) and (N, 1); the per-row limits hold, in turn, a cost of the row, a value between two
    costs, -0.0, -1.0, a NaN, +inf and a negative NaN.
    Returns dict(x, y, w, shapes, limit (the B problems), K, metric, family, base (the same of the 7), want):
    want = np.tile of points_to_ell / boxes_to_ell on the 7."""
    rng = np.random.default_rng([seed, N, M, K])
    P = LAP_P
    Dc = 4 if family == "boxes" else D
    x, y = _draw(family, (P, N, Dc), dtype, rng), _draw(family, (P, M, Dc), dtype, rng)
    w = None
    if family == "whitened":
        w = np.full((P, N, Dc, Dc), np.nan, dtype=dtype)
        w[..., np.tril(np.ones((Dc, Dc), dtype=bool))] = rng.integers(1, 3, (P, N, Dc * (Dc + 1) // 2)).astype(dtype)
    shapes = np.array([[N, M], [1, 1], [N, max(M - 1, 1)], [N, M], [N + 1, M], [max(N - 1, 1), M], [N, 1]], dtype=np.int32)
    if family == "boxes":
        cost = boxes_to_dense(x, y, metric=metric)
    else:
        cost = points_to_dense(x, y, whiten=w)
    special = (-0.0, -1.0, np.nan, np.inf, -np.nan)
    limit = np.empty((P, N))
    for b in range(P):
        for i in range(N):
            kind = (b * N + i) % (len(special) + 2)
            row = np.sort(cost[b, i])
            at = int(rng.integers(0, M))
            limit[b, i] = row[at] if kind == 0 else row[at] + 2.0 ** -10 if kind == 1 else special[kind - 2]
    base = dict(x=x, y=y, w=w, shapes=shapes, limit=limit)
    want7 = to_ell(family, x, y, K, shapes, limit, w, metric)
    reps = -(-B // P)

    def tile(a):
        return None if a is None else np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B])

    out = {key: tile(v) for key, v in base.items()}
    out.update(K=K, metric=metric, family=family, base=base, want={key: tile(want7[key]) for key in KEYS})
    return out


FIRST_CAP = dict(B=65535 + 9, N=3, M=5, K=2)  # gridDim = (1, 65535): three active wavefronts and one idle
SECOND_CAP = dict(B=8192 + 3, N=2048, M=2, K=1)  # gridDim = (512, 8192): B N >= 2^24 rows, whatever N


def second_cap_problem():
    """The second cap's input, a few KB: one problem x (1, 2048, 1), y (1, 2, 1) of float32 (the caller expands both to
    B problems with stride 0) and six (shape, limit) combinations, problem b taking combination b % 6 -- the workgroup
    that took problem b takes b + 8192 next, another combination.  Returns dict(x, y, shapes6 (6, 2), limit6 (6,),
    combo (B,), want6): want6 = points_to_ell of the six single problems, (6, 2048, 1) / (6, 2048) / (6,)."""
    rng = np.random.default_rng(17)
    N, M, B = SECOND_CAP["N"], SECOND_CAP["M"], SECOND_CAP["B"]
    x = rng.integers(0, 6, (1, N, 1)).astype(np.float32)
    y = np.array([[[1.0], [4.0]]], dtype=np.float32)
    shapes6 = np.array([[N, M], [N - 1, 1], [1, M], [N + 1, M], [N, M], [5, M]], dtype=np.int32)
    limit6 = np.array([np.inf, 4.0, -0.0, 1.0, 1.0, np.nan])
    want = points_to_ell(np.repeat(x, 6, axis=0), np.repeat(y, 6, axis=0), SECOND_CAP["K"], shapes6, limit6)
    return dict(x=x, y=y, shapes6=shapes6, limit6=limit6, combo=np.arange(B) % 6, want6=want)
