"""Shared by test_batch_launch_shapes.py (GPU) and test_batch_launch_shapes_nogpu.py: the inputs that take the
one-workgroup-per-problem solves (auction_solve_batch, auction_solve_sparse_batch) through every workgroup size and lane
edge of their shared round loop, and the oracle's result for each of them.

The loop (batch_solve, csrc/kernels_batch_solve.hpp) is launched with 256, 512 or 1024 threads, by the largest row count
of the call (batch_solve_threads, csrc/abi_batch_common.hpp; `threads_for` below).  The dense bid stages a row in up to
16 slots of 64 columns, the sparse bid strides a row's stored entries by 64, the unassigned list is compacted in
64-wide chunks.  The cases here sit on both sides of each of those steps.

Also here, and imported from here by the older batch test modules: the value kinds, the sparse problem draw and the
comparison with the oracle, split into `*_expect` (what the oracle gives, as plain values) and `*_compare` (every field
of a result against it, `==` on every bit), so that an expectation is computed once and shared.
"""
import functools

import numpy as np

from oracle import oracle as orc

META_KEYS = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "start_eps", "final_eps")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def threads_for(rows):
    """The workgroup size of a call whose largest row count (dense: the stack's N; sparse status mode: dims[0]) is rows."""
    return 256 if rows <= 256 else 512 if rows <= 512 else 1024


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ---- what the oracle gives, and the comparison of a result with it ----------------------------------------------------
def _solved(o, p0):
    if p0 is not None:  # the reference's solve() with self.p starting at p0 instead of zeros (auction_.pyx:220)
        np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))[:] = p0[:o.M]
    sol = o.solve()
    return dict(sol=sol.copy(), meta=dict(o.meta), extra=dict(o.extra), N=o.N, M=o.M, p=o.state()["p"].copy())


def dense_expect(mat, problem, p0=None, **kw):
    """What the reference gives for one float64 slice (_from_matrix(mat).solve()), as plain values."""
    return _solved(orc.from_matrix(np.ascontiguousarray(mat), problem=problem, **kw), p0)


def sparse_expect(loc, val, problem, size=None, p0=None, **kw):
    """What the reference gives for one loc / val (_from_sparse(loc, val, size=size).solve()), as plain values."""
    return dict(_solved(orc.from_sparse(loc, val.copy(), problem=problem, size=size, **kw), p0), nnz=loc.shape[0])


def _compare_common(res, b, want, n):
    meta = res["meta"]
    sol = host(res["sol"])[b]
    assert np.array_equal(sol[:n], want["sol"]), b
    assert (sol[n:] == -1).all(), b
    for k in META_KEYS:
        assert meta[k][b] == want["meta"][k], (b, k, meta[k][b], want["meta"][k])
    assert meta["obj_f64"][b] == want["extra"]["obj_f64"], b
    for k in ("start_eps_f32", "final_eps_f32"):
        assert np.float32(meta[k][b]).view(np.uint32) == np.float32(want["extra"][k]).view(np.uint32), (b, k)


def dense_compare(res, b, want, n, m, p0=None):
    """Problem b (n x m) of a dense batch result against dense_expect's values."""
    _compare_common(res, b, want, n)
    assert res["meta"]["n_cols"][b] == want["M"] and res["meta"]["n_rows"][b] == n, b
    p = host(res["prices"])[b]
    assert p.dtype == np.float64
    assert np.array_equal(bits(p[:want["M"]]), bits(want["p"])), b
    rest = np.zeros(m - want["M"]) if p0 is None else p0[want["M"]:m]  # columns without a valid entry are never bid for
    assert np.array_equal(bits(p[want["M"]:m]), bits(rest)), b
    assert (p[m:] == 0).all(), b


def sparse_compare(res, b, want):
    """Problem b of a sparse batch result against sparse_expect's values."""
    _compare_common(res, b, want, want["N"])
    meta = res["meta"]
    assert meta["n_cols"][b] == want["M"] and meta["n_rows"][b] == want["N"] and meta["nnz"][b] == want["nnz"], b
    p = host(res["prices"])[b]
    assert p.dtype == np.float64
    assert np.array_equal(bits(p[:want["M"]]), bits(want["p"])), b
    assert (p[want["M"]:] == 0).all(), b


# ---- draws ------------------------------------------------------------------------------------------------------------
def dense_values(kind, shape, rng):
    if kind == "uniform":  # benchmarking.py's recipe: doubles that are not fp32-exact
        return rng.uniform(0, 100, shape)
    if kind == "ints":  # many ties
        return rng.integers(0, 5, shape).astype(np.float64)
    if kind == "fp32":
        return rng.uniform(0, 100, shape).astype(np.float32).astype(np.float64)
    if kind == "holes":  # 30 % invalid, as -1 and NaN; the diagonal stays
        v = rng.uniform(0, 100, shape)
        h = rng.random(shape) < 0.3
        v[h] = np.where(rng.random(shape) < 0.5, -1.0, np.nan)[h]
        v[..., np.arange(shape[-2]), np.arange(shape[-2]) % shape[-1]] = rng.uniform(0, 100, shape[:-2] + (shape[-2],))
        return v
    raise AssertionError(kind)


def sparse_problem(rng, n, m, per_row, kind="uniform", shuffle=True):
    """n x m (n <= m) with per_row stored entries in every row, rows ascending; column perm[i] planted in row i (a perfect
    matching of the rows exists).  Random columns may repeat: duplicate (i, j) entries are part of the input class."""
    k = min(per_row, m) if per_row > 0 else m
    cols = rng.integers(0, m, (n, k)).astype(np.int32)
    cols[:, 0] = rng.permutation(m)[:n]
    if shuffle:
        cols = rng.permuted(cols, axis=1)
    else:
        cols.sort(axis=1)
    loc = np.ascontiguousarray(np.stack([np.repeat(np.arange(n, dtype=np.int32), k), cols.ravel()], axis=1))
    return loc, dense_values(kind, (n * k,), rng)


def sparse_problem_distinct(rng, n, m, k, kind="uniform", shuffle=True):
    """As sparse_problem, but the k columns of a row are distinct: no (i, j) entry is stored twice."""
    planted = rng.permutation(m)[:n]
    cols = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        c = rng.choice(m, k, replace=False)
        if planted[i] not in c:
            c[0] = planted[i]
        cols[i] = rng.permutation(c) if shuffle else np.sort(c)
    loc = np.ascontiguousarray(np.stack([np.repeat(np.arange(n, dtype=np.int32), k), cols.ravel()], axis=1))
    return loc, dense_values(kind, (n * k,), rng)


def sparse_pack(probs):
    loc = np.ascontiguousarray(np.concatenate([p[0] for p in probs]), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate([p[1] for p in probs]))
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in probs])]).astype(np.int64)
    return loc, val, offsets


def has_repeated_entry(loc):
    return np.unique(loc, axis=0).shape[0] < loc.shape[0]


def row_lengths(loc):
    return np.bincount(loc[:, 0])


def tied_extreme(mat, problem):
    """Whether some row of an all-valid matrix holds its best value (the maximum for 'max', the minimum for 'min': the
    bid's first-round maximum of a_ij - p_j) in two different lanes of the dense bid, and -- where the row is wider than
    one slot -- in two slots of one lane (columns c and c + 64) as well."""
    best = mat.max(axis=1, keepdims=True) if problem == "max" else mat.min(axis=1, keepdims=True)
    hit = mat == best
    M = mat.shape[1]
    lanes = np.zeros((mat.shape[0], 64), dtype=bool)
    for q in range(0, M, 64):
        w = min(64, M - q)
        lanes[:, :w] |= hit[:, q:q + w]
    two_lanes = lanes.sum(axis=1) >= 2
    if M <= 64:
        return bool(two_lanes.any())
    two_slots = (hit[:, :M - 64] & hit[:, 64:]).any(axis=1)
    return bool((two_lanes & two_slots).any())


# ---- 1. the dense ladder: a stack of three problems of one shape, one per value kind ---------------------------------------
PROBLEMS = ("min", "max")
LADDER_KINDS = ("uniform", "ints", "holes")
# the workgroup-size steps, square; then the staging-slot edges with N on each side of a step
LADDER_SHAPES = [(64, 64), (65, 65), (256, 256), (257, 257), (512, 512), (513, 513),
                 (65, 128), (65, 129), (129, 192), (129, 193), (257, 960), (257, 961), (513, 1023), (1023, 1024)]


def shape_id(shape):
    return "x".join(str(int(d)) for d in shape)


@functools.lru_cache(maxsize=2)
def ladder_stack(shape):
    N, M = shape
    return _frozen(np.stack([dense_values(kind, (N, M), np.random.default_rng([1, N, M, k]))
                             for k, kind in enumerate(LADDER_KINDS)]))


@functools.lru_cache(maxsize=None)
def ladder_expect(shape, problem):
    return [dense_expect(mat, problem) for mat in ladder_stack(shape)]


# ---- 2. the same launches through the status kernel and the typed kernels --------------------------------------------------
STATUS_SHAPES = [(257, 257), (512, 512), (513, 1023)]
STATUS_KINDS = ("uniform", "ints", "condemned", "holes")  # the condemned problem sits between live ones
CONDEMNED = STATUS_KINDS.index("condemned")
EMPTY_ROW_STATUS = 2  # MISSLAP_BATCH_STATUS_EMPTY_ROW


@functools.lru_cache(maxsize=2)
def status_stack(shape):
    """(mats, prices): four problems of one shape -- problems 0 and 2 with starting prices, problem 2 with an empty row."""
    N, M = shape
    mats = np.stack([dense_values("uniform" if kind == "condemned" else kind, (N, M), np.random.default_rng([2, N, M, k]))
                     for k, kind in enumerate(STATUS_KINDS)])
    mats[CONDEMNED, N // 2, :] = np.where(np.arange(M) % 2 == 0, -1.0, np.nan)
    prices = np.zeros((len(STATUS_KINDS), M))
    prices[0] = np.random.default_rng([2, N, M, 99]).uniform(0, 20, M)
    prices[CONDEMNED] = np.random.default_rng([2, N, M, 98]).uniform(1, 20, M)  # (its price row must come back as zeros)
    return _frozen(mats, prices)


@functools.lru_cache(maxsize=None)
def status_expect(shape, problem):
    mats, prices = status_stack(shape)
    return [None if b == CONDEMNED else dense_expect(mats[b], problem, p0=prices[b]) for b in range(len(mats))]


TYPED_DTYPES = ("float16", "bfloat16")
TYPED_SHAPES = [(257, 961), (513, 513)]  # the 2-byte staging slots 3 .. 15 at odd M
TYPED_KINDS = ("uniform", "ints")


def round_to(draw, dtype):
    """A float64 draw rounded to dtype and widened again (numpy has no bfloat16: that one goes through torch)."""
    if dtype == "bfloat16":
        import torch
        return torch.from_numpy(np.array(draw, dtype=np.float64)).to(torch.bfloat16).double().numpy()
    return draw.astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=2)
def typed_stack(shape, dtype):
    """The widened float64 stack: `uniform` rounded to the type (dense ties) and `ints` (exact in every type)."""
    N, M = shape
    return _frozen(np.stack([round_to(dense_values(kind, (N, M), np.random.default_rng([3, N, M, k])), dtype)
                             for k, kind in enumerate(TYPED_KINDS)]))


@functools.lru_cache(maxsize=None)
def typed_expect(shape, dtype, problem):
    return [dense_expect(mat, problem) for mat in typed_stack(shape, dtype)]


# ---- 3. a 1024-thread launch around small problems ------------------------------------------------------------------------
SMALL_STACK = (10, 600, 640)
SMALL_SHAPES = np.array([[1, 40], [2, 64], [63, 63], [64, 65], [65, 129], [256, 300], [257, 257], [512, 640], [513, 577],
                         [600, 601]])
# (values 0 .. 4 start at eps = 2 and fall under 1 / n after two reductions where n < 23: the tiny problems are `uniform`)
SMALL_KINDS = ("uniform", "uniform", "holes", "ints", "uniform", "holes", "ints", "uniform", "holes", "ints")


@functools.lru_cache(maxsize=1)
def small_stack():
    mats = np.full(SMALL_STACK, np.inf)  # +inf would be rejected (default mode) or reported (status mode) if it were read
    for b, ((n, m), kind) in enumerate(zip(SMALL_SHAPES, SMALL_KINDS)):
        mats[b, :n, :m] = dense_values(kind, (int(n), int(m)), np.random.default_rng([4, b]))
    return _frozen(mats)


@functools.lru_cache(maxsize=None)
def small_expect(problem):
    mats = small_stack()
    return [dense_expect(mats[b, :n, :m], problem) for b, (n, m) in enumerate(SMALL_SHAPES)]


# ---- 4. the sparse ladder ------------------------------------------------------------------------------------------------
SPARSE_ROWS = [256, 257, 512, 513]
SPARSE_KINDS = ("uniform_distinct_k63", "ints_distinct_shuffled_k65", "uniform_repeated_k128_129", "rectangular_k8")
SPARSE_DISTINCT = (0, 1)  # the problems without a repeated (i, j) entry: the oracle ends with soln_found == 1
SPARSE_K = {256: (63, 65, 128, 8), 257: (63, 65, 129, 8), 512: (63, 65, 129, 8), 513: (63, 65, 128, 8)}


@functools.lru_cache(maxsize=None)
def sparse_batch(n):
    k = SPARSE_K[n]
    rng = [np.random.default_rng([5, n, i]) for i in range(4)]
    probs = [sparse_problem_distinct(rng[0], n, n, k[0], "uniform", shuffle=False),
             sparse_problem_distinct(rng[1], n, n, k[1], "ints", shuffle=True),
             sparse_problem(rng[2], n, n, k[2], "uniform"),
             sparse_problem(rng[3], n, n + 43, k[3], "uniform")]
    for loc, val in probs:
        _frozen(loc, val)
    return probs


@functools.lru_cache(maxsize=None)
def sparse_expect_batch(n, problem):
    return [sparse_expect(loc, val, problem) for loc, val in sparse_batch(n)]


SPARSE_BIG_DIMS = [(512, 600), (1024, 1100)]  # status mode: the carve, and with it the workgroup size, comes from dims


@functools.lru_cache(maxsize=None)
def sparse_small_batch():
    """Problems of 5 .. 40 rows, for the carves of SPARSE_BIG_DIMS."""
    rng = np.random.default_rng([6])
    rows = [5, 40] + [int(x) for x in rng.integers(6, 40, 6)]
    # (one `ints` problem, at 40 rows: below 23 rows values 0 .. 4 end after two eps reductions)
    probs = [sparse_problem(rng, n, 45, 6, "ints" if n == 40 else "uniform") for n in rows]
    for loc, val in probs:
        _frozen(loc, val)
    return probs


@functools.lru_cache(maxsize=None)
def sparse_small_expect(problem):
    return [sparse_expect(loc, val, problem) for loc, val in sparse_small_batch()]


# ---- 5. stopped solves at each workgroup size -------------------------------------------------------------------------------
STOP_DENSE = [(256, 256), (512, 512), (513, 513)]
STOP_SPARSE = [256, 512, 513]  # rows; k = 65 distinct columns
STOP_NAMES = ("0", "1", "2", "3", "10", "half", "last")


def stops(its):
    """The seven values of max_iter for a solve of `its` rounds."""
    return [0, 1, 2, 3, 10, its // 2, its - 1]


@functools.lru_cache(maxsize=None)
def stop_dense_input(shape):
    N, M = shape
    return _frozen(dense_values("uniform", (N, M), np.random.default_rng([7, N, M])))


@functools.lru_cache(maxsize=None)
def stop_sparse_input(n):
    return _frozen(*sparse_problem_distinct(np.random.default_rng([8, n]), n, n, 65, "uniform"))


@functools.lru_cache(maxsize=None)
def stop_dense_expect(shape, problem):
    """(the full solve, [(max_iter, the solve stopped there)] for the seven stops)."""
    mat = stop_dense_input(shape)
    full = dense_expect(mat, problem)
    return full, [(r, dense_expect(mat, problem, max_iter=r)) for r in stops(full["meta"]["its"])]


@functools.lru_cache(maxsize=None)
def stop_sparse_expect(n, problem):
    loc, val = stop_sparse_input(n)
    full = sparse_expect(loc, val, problem)
    return full, [(r, sparse_expect(loc, val, problem, max_iter=r)) for r in stops(full["meta"]["its"])]
