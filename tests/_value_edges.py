"""Shared by test_batch_value_edges.py (GPU) and test_batch_value_edges_nogpu.py: the values that take the round loop of
the batch solves (batch_solve, csrc/kernels_batch_solve.hpp) and the check pass in front of it to the edges of the value
range -- negative entries, a C = max |v| that overflows, underflows or rounds as a float32, magnitudes at which eps
falls below one ulp of the prices, and an eps_start at the float32 limits -- with the oracle's result for each.

One graph carries every sparse case (70 x 70, 9 distinct entries per row; a second one of 257 rows for the two cases
that also run in a 512-thread launch), one 40 x 56 matrix with holes every dense case: only the values change.  A case
is (name, rows, values, opts, stop): opts the call's eps_start, stop the max_iter given to BOTH sides -- None only where
the oracle ends on its own in fewer than 1000 rounds (test_batch_value_edges_nogpu.py holds every case to that, so that
no workgroup is ever sent into a solve that only the default max_iter of 1 000 000 would end).
"""
import collections
import functools

import numpy as np

from tests._batch_shapes import dense_expect, dense_values, sparse_expect, sparse_problem_distinct

FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = float(np.finfo(np.float64).max)
ROWS, BIG_ROWS, PER_ROW = 70, 257, 9
DENSE_SHAPE = (40, 56)
PROBLEMS = ("min", "max")

Case = collections.namedtuple("Case", "name rows val opts stop")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def graph(rows):
    """(loc, u, ints): the graph of `rows` rows, its uniform [0, 100) values and integers 0 .. 4 on the same entries."""
    loc, u = sparse_problem_distinct(np.random.default_rng([91, rows]), rows, rows, PER_ROW, "uniform")
    ints = np.random.default_rng([92, rows]).integers(0, 5, len(u)).astype(np.float64)
    return _frozen(loc, u, ints)


def _odd_offset(u):
    """16777217 or 16777218, whichever makes the largest floor(u) + offset odd: between 2^24 and 2^25 a float32 holds the
    even integers only, so C is then a tie between two of them and rounds to the even mantissa."""
    return 16777217.0 if np.floor(u).max() % 2 == 0 else 16777218.0


def _flt_max_exact(u):
    w = u / u.max() * FLT_MAX
    w[np.argmax(u)] = FLT_MAX
    return np.minimum(w, FLT_MAX)


# 25601.25 * 2^-149: as a float32 C is 25601 * 2^-149, and C / 2 = 12800.5 * 2^-149 is a tie that goes to the even 12800;
# halved BEFORE it is narrowed, 12800.625 * 2^-149 would go to 12801.  (Not in the issue's list: the one magnitude at
# which the order of the two steps of eps = (float)((double)(float)C / 2.0) shows.)
_TIE = 25601.25 * 2.0 ** -149

# the magnitudes of C, as functions of non-negative values u of any shape: (name, f, stop)
MAGNITUDES = (
    ("above_flt_max", lambda u: u * 1e37, 60),                       # C = +inf as a float32
    ("dbl_max", lambda u: u / 100 * DBL_MAX, 60),
    ("flt_max_exact", _flt_max_exact, 300),                          # C narrows exactly, eps = FLT_MAX / 2
    ("c_is_zero", lambda u: u * 2.0 ** -160, 200),                   # every value below 2^-150: C == 0 and eps == 0
    ("zeros", lambda u: u * 0.0, 200),
    ("c_subnormal_f32", lambda u: u * 2.0 ** -140, None),            # C is a float32 subnormal (the oracle ends)
    ("c_subnormal_tie", lambda u: u * (_TIE / u.max()), None),        # ... and C / 2 is a tie as a float32
    ("round_to_f32", lambda u: np.floor(u) + _odd_offset(u), 4000),  # C is not float32-exact
    ("ulp_2_53", lambda u: np.floor(u * 2.0 ** 47), 300),            # eps falls below one ulp of the prices
    ("ties_2_52", None, 300),                                        # integers 0 .. 4 times 2^52 (from `ints`)
)
# eps_start on plain u: (name, eps_start, stop)
EPS_STARTS = (
    ("eps_1e-46", 1e-46, None),  # narrows to 0: the default C / 2 holds
    ("eps_1e-45", 1e-45, 2000),  # a float32 subnormal: it holds, and the solve is one phase
    ("eps_3e38", 3e38, 300),
    ("eps_1e39", 1e39, 60),      # +inf
)
BIG = ("neg_mixed", "round_to_f32")  # the cases on the graph of 257 rows
SIGN_NAMES = ("neg_mixed", "all_neg", "neg_ints", "c_from_negative", "neg_zero")
STOPPED = {name: stop for name, _, stop in MAGNITUDES + EPS_STARTS if stop is not None}
# What a stop is for.  NEVER_ENDS: C or eps is +inf or every value is 0 -- no variant of the case ends, each is cut at
# its stop.  ENDS_LATE: the oracle ends on its own (eCE == 1) in every variant, but in more than 1000 rounds: the stop is
# a bound above that, never reached.  The other stopped cases are cut in most variants and end on their own, below the
# stop, in a few (with eps == 0 a solve of distinct values can end; so can one at 2^53 after float32 rounding).
NEVER_ENDS = ("above_flt_max", "dbl_max", "zeros", "eps_1e39")
ENDS_LATE = ("round_to_f32", "eps_1e-45")


def _neg_ints(ints):
    return ints - 2.0


def _neg_zero(ints):
    v = _neg_ints(ints)
    v[v == 0.0] = -0.0
    return v


def _c_from_negative(u):
    v = u.copy()
    v[len(v) // 2] = -1000.0
    return v


@functools.lru_cache(maxsize=None)
def sparse_cases():
    """{name: Case}: the sign cases, the magnitudes of C and the eps_start cases on the sparse graphs."""
    out = []

    def add(name, f, stop, opts=(), use_ints=False):
        rows = BIG_ROWS if name in BIG else ROWS
        _, u, ints = graph(rows)
        with np.errstate(over="raise"):
            val = np.ascontiguousarray(f(ints.copy() if use_ints else u.copy()), dtype=np.float64)
        assert np.isfinite(val).all()
        out.append(Case(name, rows, _frozen(val), tuple(sorted(dict(opts).items())), stop))

    add("neg_mixed", lambda u: u - 50.0, None)
    add("all_neg", lambda u: -u - 1.0, None)
    add("neg_ints", _neg_ints, None, use_ints=True)
    add("c_from_negative", _c_from_negative, None)
    add("neg_zero", _neg_zero, None, use_ints=True)
    for name, f, stop in MAGNITUDES:
        if name == "ties_2_52":
            add(name, lambda ints: ints * 2.0 ** 52, stop, use_ints=True)
        else:
            add(name, f, stop)
    for name, eps, stop in EPS_STARTS:
        add(name, lambda u: u, stop, opts=dict(eps_start=eps))
    return {c.name: c for c in out}


def rounded_f32(val):
    """val rounded to float32 and widened again; None where a finite value has no finite float32."""
    with np.errstate(over="ignore"):
        w = val.astype(np.float32)
    finite = np.isfinite(val)
    if not np.isfinite(w[finite]).all():
        return None
    return w.astype(np.float64)


def sparse_problem_of(case, f32=False):
    """(loc, val) of a case; f32: the values rounded to float32 (the oracle of a float32 call is the oracle of these)."""
    loc = graph(case.rows)[0]
    return loc, (rounded_f32(case.val) if f32 else case.val)


def has_f32(case):
    return rounded_f32(case.val) is not None


def oracle_opts(case):
    o = dict(case.opts, cardinality_check=False)
    if case.stop is not None:
        o["max_iter"] = case.stop
    return o


@functools.lru_cache(maxsize=None)
def sparse_want(name, problem, f32=False):
    case = sparse_cases()[name]
    loc, val = sparse_problem_of(case, f32)
    with np.errstate(over="ignore"):  # (eps_start = 1e39 narrows to +inf)
        return sparse_expect(loc, val, problem, size=(case.rows, case.rows), **oracle_opts(case))


def groups(cases):
    """Options are per call: [(rows, opts, stop, [cases])], the cases of one (rows, eps_start, stop) in one batch."""
    out = {}
    for c in cases:
        out.setdefault((c.rows, c.opts, c.stop), []).append(c)
    return [(rows, dict(opts), stop, cs) for (rows, opts, stop), cs in out.items()]


def call_opts(opts, stop):
    """The keywords of a library call for a group."""
    kw = dict(opts, cardinality_check=False)
    if stop is not None:
        kw["max_iter"] = stop
    return kw


# ---- `fast`: eps = (float)(1.0 / n) per problem, at row counts whose reciprocal is inexact
FAST_ROWS = (1, 2, 3, 7, 70)


@functools.lru_cache(maxsize=None)
def fast_mix():
    """[(loc, val)] of 1, 2, 3, 7 and 70 rows (9 distinct entries per row), and their sizes (m_b, n_b)."""
    probs = [_frozen(*sparse_problem_distinct(np.random.default_rng([93, n]), n, max(n, PER_ROW), PER_ROW, "uniform"))
             for n in FAST_ROWS]
    sizes = np.array([[int(loc[:, 1].max()) + 1, n] for (loc, _), n in zip(probs, FAST_ROWS)], dtype=np.int64)
    return probs, _frozen(sizes)


@functools.lru_cache(maxsize=None)
def fast_want(problem):
    probs, sizes = fast_mix()
    return [sparse_expect(loc, val, problem, size=(int(m), int(n)), fast=True, cardinality_check=False)
            for (loc, val), (m, n) in zip(probs, sizes)]


# ---- the dense cases: the magnitudes and the eps_start cases on one 40 x 56 matrix with holes
@functools.lru_cache(maxsize=None)
def dense_base():
    """(u, valid, ints): uniform [0, 100) with 30 % holes (-1 and NaN), the mask of its valid entries, integers 0 .. 4."""
    rng = np.random.default_rng([94])
    u = dense_values("holes", DENSE_SHAPE, rng)
    with np.errstate(invalid="ignore"):
        valid = u >= 0
    ints = rng.integers(0, 5, DENSE_SHAPE).astype(np.float64)
    return _frozen(u, valid, ints)


@functools.lru_cache(maxsize=None)
def dense_cases():
    """{name: Case}: val is the (40, 56) matrix, its holes kept."""
    u, valid, ints = dense_base()
    out = []

    def add(name, vals, stop, opts=()):
        mat = u.copy()
        mat[valid] = vals
        assert np.isfinite(mat[valid]).all() and not np.signbit(mat[valid]).any()
        out.append(Case(name, DENSE_SHAPE[0], _frozen(mat), tuple(sorted(dict(opts).items())), stop))

    for name, f, stop in MAGNITUDES:
        add(name, ints[valid] * 2.0 ** 52 if name == "ties_2_52" else f(u[valid].copy()), stop)
    for name, eps, stop in EPS_STARTS:
        add(name, u[valid], stop, opts=dict(eps_start=eps))
    return {c.name: c for c in out}


def dense_rounded_f32(mat):
    """The matrix as float32 (holes kept), or None where a valid value has no finite float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        w = mat.astype(np.float32)
        bad = np.isinf(w) & np.isfinite(mat)
    return None if bad.any() else w


@functools.lru_cache(maxsize=None)
def dense_want(name, problem, f32=False):
    case = dense_cases()[name]
    mat = dense_rounded_f32(case.val).astype(np.float64) if f32 else case.val
    with np.errstate(over="ignore"):
        return dense_expect(mat, problem, **oracle_opts(case))


# ---- the outside modes: (case, outside value, dense too)
OUTSIDE = (
    ("neg_mixed", -75.0, False),      # below every entry of (-50, 50): C is the outside value's alone
    ("all_neg", -150.0, False),       # below every entry of (-101, -1]
    ("ulp_2_53", 2.0 ** 52, True),
    ("c_is_zero", 0.0, True),         # (dense: -0.0, a valid entry there)
    ("above_flt_max", 3.0, True),
)
OUTSIDE_STOP = 300  # for the cases that have no stop of their own: the eps-scaled solve of a rectangular problem
OUTSIDE_OPTS = dict(fast=False)  # eps-scaling from C / 2: with `fast` eps is 1 / n and C is never used


def outside_stop(name):
    return STOPPED.get(name, OUTSIDE_STOP)


def outside_dense_value(name, value):
    return -0.0 if name == "c_is_zero" else value


@functools.lru_cache(maxsize=None)
def outside_sparse_want(name, problem, f32=False):
    """(want, m, n): the oracle on sparse_to_augmented's problem (test_batch_value_edges_nogpu.py: ell_to_packed(outside=)
    gives the same one, so this serves the ELL call too)."""
    from sslap_amd import sparse_to_augmented
    value = dict((k, v) for k, v, _ in OUTSIDE)[name]
    loc, val = sparse_problem_of(sparse_cases()[name], f32)
    (lo, va, m, n), = sparse_to_augmented(loc, val, np.array([0, len(val)]), None, value)
    return sparse_expect(lo, va, problem, size=(m + n, n), max_iter=outside_stop(name), **OUTSIDE_OPTS), m, n


@functools.lru_cache(maxsize=None)
def outside_dense_want(name, problem, f32=False):
    from sslap_amd import dense_to_augmented
    value = outside_dense_value(name, dict((k, v) for k, v, _ in OUTSIDE)[name])
    mat = dense_cases()[name].val
    mat = dense_rounded_f32(mat).astype(np.float64) if f32 else mat
    aug, = dense_to_augmented(mat[None], None, outside=value)
    want = dense_expect(aug, problem, cardinality_check=False, max_iter=outside_stop(name), **OUTSIDE_OPTS)
    with np.errstate(invalid="ignore"):
        want["nnz"] = int((aug >= 0).sum())
    return want, mat.shape[1], mat.shape[0]
