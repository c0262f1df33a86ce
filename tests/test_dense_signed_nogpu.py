"""Signed dense stacks (entries="finite") without a GPU: the option word MISSLAP_DENSE_ENTRIES_FINITE | mat_dtype is
validated before any device is touched, the front ends check `entries` and `outside`, dense_to_packed is the definition
it is documented to be, and that definition is sound: the CPU oracle on the packed problem reaches scipy's optimum on
the same entries.
"""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from oracle import oracle as orc
from sslap_amd import _batch, _lib, auction_solve_batch, dense_to_packed, hopcroft_solve_batch
from tests._dense_signed import packed_expect, signed_ints
from tests.test_dense_strided_nogpu import _FakeDeviceTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE = 0x100
SIX = ("misslap_solve_dense_batch_status", "misslap_solve_dense_batch_outside", "misslap_solve_dense_batch_status_strided",
       "misslap_solve_dense_batch_outside_strided", "misslap_matching_dense_batch", "misslap_matching_dense_batch_strided")


# ---- the option word -------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(built_lib):
    """name -> f(mat_dtype): the entry point on a 2 x 3 x 4 stack with that option word, every other argument valid.  The
    stack is large enough for any element type; no call here may get as far as reading it."""
    mat = np.ones((2, 3, 4))
    sol, status = np.empty((2, 3), dtype=np.int32), np.empty(2, dtype=np.int32)
    outside = np.ones(2)
    size, rows, cols = (np.empty(2, dtype=np.int32) for _ in range(3))
    metas = (_lib.DenseBatchMeta * 2)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def options(mat_dtype, on_device):
        o = _lib.Options()
        o.struct_size = C.sizeof(_lib.Options)
        o.max_iter = 10
        o.input_on_device = on_device
        o.mat_dtype = mat_dtype
        return o

    def status_call(dt, strides=()):
        f = built_lib.misslap_solve_dense_batch_status_strided if strides else built_lib.misslap_solve_dense_batch_status
        return f(2, 3, 4, *strides, mat.ctypes.data, None, 0, None, 1, C.byref(options(dt, 1 if strides else 0)), None,
                 None, 0, sol.ctypes.data, None, 0, status.ctypes.data, None, C.cast(metas, C.c_void_p), None)

    def outside_call(dt, strides=()):
        f = built_lib.misslap_solve_dense_batch_outside_strided if strides else built_lib.misslap_solve_dense_batch_outside
        return f(2, 3, 4, *strides, mat.ctypes.data, None, 1, None, C.byref(options(dt, 1 if strides else 0)), None, None,
                 0, outside.ctypes.data, 0, sol.ctypes.data, None, None, 0, status.ctypes.data, None,
                 C.cast(metas, C.c_void_p), None)

    def matching_call(dt, strides=()):
        f = built_lib.misslap_matching_dense_batch_strided if strides else built_lib.misslap_matching_dense_batch
        return f(2, 3, 4, *strides, mat.ctypes.data, None, C.byref(options(dt, 1 if strides else 0)), size.ctypes.data,
                 rows.ctypes.data, cols.ctypes.data, None, 0, None, 0, 0, None)

    def default_call(dt):
        return built_lib.misslap_solve_dense_batch(2, 3, 4, mat.ctypes.data, None, None, None, 1, C.byref(options(dt, 0)),
                                                   sol.ctypes.data, None, 0, metas, None)

    transposed = (12, 1, 3)
    return {
        SIX[0]: status_call, SIX[1]: outside_call, SIX[2]: lambda dt: status_call(dt, transposed),
        SIX[3]: lambda dt: outside_call(dt, transposed), SIX[4]: matching_call,
        SIX[5]: lambda dt: matching_call(dt, transposed), "misslap_solve_dense_batch": default_call,
    }


@pytest.mark.parametrize("name", SIX)
def test_the_flag_rides_on_every_element_type(calls, built_lib, name):
    """0x100 .. 0x103 pass every check made before a device is touched: the call ends looking for one."""
    err = built_lib.misslap_last_error
    for dt in range(4):
        assert calls[name](dt) == _lib.ERR_NO_DEVICE, (dt, err())
        assert calls[name](FINITE | dt) == _lib.ERR_NO_DEVICE, (dt, err())
    for bad in (0x104, 0x200, FINITE | 0x80, 4, -1, FINITE | 4, -FINITE):
        assert calls[name](bad) == _lib.ERR_INVALID, bad
        assert b"mat_dtype" in err(), err()


def test_the_default_mode_call_names_the_status_call(calls, built_lib):
    err = built_lib.misslap_last_error
    call = calls["misslap_solve_dense_batch"]
    assert call(0) == _lib.ERR_NO_DEVICE
    for dt in range(4):
        assert call(FINITE | dt) == _lib.ERR_INVALID
        assert b"MISSLAP_DENSE_ENTRIES_FINITE" in err() and b"misslap_solve_dense_batch_status" in err(), err()


def test_other_entry_points_do_not_take_the_flag(built_lib):
    """The float64-only entry points and the ELL / sparse batches read mat_dtype as an element type they do not have."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.mat_dtype = FINITE
    handle = C.c_void_p()
    loc, val = np.zeros((1, 2), dtype=np.int32), np.ones(1)
    assert built_lib.misslap_create(C.byref(handle), 1, loc.ctypes.data, val.ctypes.data, C.byref(o)) == _lib.ERR_INVALID
    assert b"mat_dtype" in built_lib.misslap_last_error()


def test_the_flag_is_the_headers_and_the_workspace_does_not_depend_on_it(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    assert "#define MISSLAP_DENSE_ENTRIES_FINITE 0x100" in header and _lib.DENSE_ENTRIES_FINITE == FINITE
    assert "#define MISSLAP_ABI_VERSION 2" in header
    # neither sizing function takes the options: the bytes of a call are those of the same call without the flag
    for name, args in (("misslap_dense_batch_workspace_bytes", (7, 65, 130, 1, 1)),
                       ("misslap_dense_batch_outside_workspace_bytes", (7, 65, 130, 1))):
        assert len(_lib.SYMBOLS[name][1]) == len(args) and all(t is not C.c_void_p for t in _lib.SYMBOLS[name][1])
        assert getattr(built_lib, name)(*args) > 0
    carve = lambda B, guard: sum(-(-x // 256) * 256 for x in (32 * B, 8 * B, 4 * B if guard else 0))  # noqa: E731
    assert built_lib.misslap_dense_batch_workspace_bytes(7, 65, 130, 1, 1) == carve(7, True)


# ---- the front ends ---------------------------------------------------------------------------------------------------
def test_entries_keyword_is_checked_first():
    mats = np.ones((2, 3, 4))
    for bad in ("signed", "Finite", None, 1, b"finite"):
        with pytest.raises(ValueError, match="entries must be 'nonneg' or 'finite'"):
            auction_solve_batch(mats, entries=bad)
        with pytest.raises(ValueError, match="entries must be 'nonneg' or 'finite'"):
            hopcroft_solve_batch(mats=mats, entries=bad)
        with pytest.raises(ValueError, match="entries must be 'nonneg' or 'finite'"):
            dense_to_packed(mats, entries=bad)
    with pytest.raises(TypeError, match="entries goes with mats"):
        hopcroft_solve_batch(loc=np.zeros((1, 2), dtype=np.int32), offsets=[0, 1], entries="finite")
    assert _batch._entries_flag("nonneg") == 0 and _batch._entries_flag("finite") == FINITE


def test_outside_checks_in_either_mode():
    mats = np.ones((2, 3, 4))
    for entries in ("nonneg", "finite"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="outside must be finite"):
                auction_solve_batch(mats, outside=bad, entries=entries)
    with pytest.raises(ValueError, match="outside must be >= 0"):
        auction_solve_batch(mats, outside=-1.5)
    # a negative scalar passes Python's checks in finite mode only: the call goes on to the library, which has no device
    with pytest.raises(RuntimeError, match="no HIP device"):
        auction_solve_batch(mats, outside=-1.5, entries="finite")
    # arrays are the library's to judge (status 15 for a NaN, as today): they pass, whatever they hold
    with pytest.raises(RuntimeError, match="no HIP device"):
        auction_solve_batch(mats, outside=np.array([np.nan, -2.0]), entries="finite")
    with pytest.raises(RuntimeError, match="no HIP device"):
        auction_solve_batch(mats, outside=np.array([np.nan, -2.0]))


def test_finite_mode_takes_the_status_call_with_the_flag_in_the_option_word(monkeypatch):
    """errors="raise" on a host stack and on a contiguous device tensor: misslap_solve_dense_batch_status with
    mat_dtype | 0x100, never the default mode's own call; "nonneg" goes where it always went."""
    seen = []

    class Lib:
        def __getattr__(self, name):
            def f(*args):
                opts = [a for a in args if hasattr(a, "_obj") and isinstance(a._obj, _lib.Options)]
                seen.append((name, opts[0]._obj.mat_dtype if opts else None))
                raise RuntimeError("stop")
            return f

    monkeypatch.setattr(_lib, "load", lambda: Lib())
    mats = np.ones((2, 3, 4), dtype=np.float32)
    for kw, want in ((dict(entries="finite"), ("misslap_solve_dense_batch_status", FINITE | 1)),
                     (dict(entries="finite", errors="status"), ("misslap_solve_dense_batch_status", FINITE | 1)),
                     (dict(entries="finite", outside=-2.0), ("misslap_solve_dense_batch_outside", FINITE | 1)),
                     (dict(), ("misslap_solve_dense_batch", 1)),
                     (dict(errors="status"), ("misslap_solve_dense_batch_status", 1)),
                     (dict(outside=2.0), ("misslap_solve_dense_batch_outside", 1))):
        del seen[:]
        with pytest.raises(RuntimeError, match="stop"):
            auction_solve_batch(mats, mat_dtype="float32", **kw)
        assert seen == [want], (kw, seen)
    del seen[:]
    with pytest.raises(RuntimeError, match="stop"):
        hopcroft_solve_batch(mats=mats, mat_dtype="float32", entries="finite")
    assert seen == [("misslap_matching_dense_batch", FINITE | 1)]
    t = _FakeDeviceTensor(np.zeros((2, 3, 4)), "float64")
    assert _batch._stack_strides(t, True) is None  # contiguous: the non-strided entry point gets the flag


# ---- dense_to_packed ----------------------------------------------------------------------------------------------------
def test_dense_to_packed_by_hand():
    nan = np.nan
    mats = np.array([[[1.0, nan, -0.0, -2.5],
                      [nan, nan, nan, nan],
                      [0.0, 5e-324, -np.inf, 7.0]],
                     [[-1.0, 2.0, nan, 9.0],
                      [nan, -3.0, 4.0, 9.0],
                      [9.0, 9.0, 9.0, 9.0]]])
    shapes = np.array([[3, 4], [2, 3]])
    (l0, v0), (l1, v1) = dense_to_packed(mats, shapes, entries="finite")
    assert l0.dtype == np.int32 and v0.dtype == np.float64 and l0.shape == (7, 2)
    assert l0.tolist() == [[0, 0], [0, 2], [0, 3], [2, 0], [2, 1], [2, 2], [2, 3]]
    assert v0.view(np.uint64).tolist() == np.array([1.0, -0.0, -2.5, 0.0, 5e-324, -np.inf, 7.0]).view(np.uint64).tolist()
    assert l1.tolist() == [[0, 0], [0, 1], [1, 1], [1, 2]] and v1.tolist() == [-1.0, 2.0, -3.0, 4.0]
    # "nonneg": what from_matrix keeps (v >= 0: -0.0 is kept, negatives and NaN are not)
    (l0, v0), (l1, v1) = dense_to_packed(mats, shapes)
    assert l0.tolist() == [[0, 0], [0, 2], [2, 0], [2, 1], [2, 3]]
    assert v0.view(np.uint64).tolist() == np.array([1.0, -0.0, 0.0, 5e-324, 7.0]).view(np.uint64).tolist()
    assert l1.tolist() == [[0, 1], [1, 2]] and v1.tolist() == [2.0, 4.0]
    for b, (n, m) in enumerate(shapes):  # ... literally: the oracle's own dense scan
        a = np.ascontiguousarray(mats[b, :n, :m])
        loc, val = np.empty((n * m, 2), dtype=np.int32), np.empty(n * m)
        k = orc.lib().oracle_dense_to_coo(a.ctypes.data, n, m, loc.ctypes.data, val.ctypes.data)
        got = dense_to_packed(mats, shapes, "nonneg")[b]
        assert np.array_equal(got[0], loc[:k]) and np.array_equal(got[1].view(np.uint64), val[:k].view(np.uint64))
    # without shapes: the whole slice; a float32 stack is widened exactly
    whole = dense_to_packed(mats.astype(np.float32), entries="finite")
    assert whole[1][0].shape == (10, 2) and whole[1][1].dtype == np.float64 and whole[0][1][4] == 0.0  # (5e-324 -> 0 in fp32)
    with pytest.raises(ValueError, match="3 dimensions"):
        dense_to_packed(mats[0])


# ---- the definition is sound -----------------------------------------------------------------------------------------------
DRAWS = 200


def _draw(k):
    rng = np.random.default_rng([41, k])
    n = int(rng.integers(1, 40))
    m = n if k % 2 == 0 else int(rng.integers(n, 40))
    return signed_ints(rng, n, m)


def _optimum(v, problem):
    """linear_sum_assignment on the same entries: a hole costs more than any assignment of entries can differ by."""
    big = np.nansum(np.abs(v)) + 1.0
    cost = np.where(np.isnan(v), big if problem == "min" else -big, v)
    r, c = linear_sum_assignment(cost, maximize=problem == "max")
    assert not np.isnan(v[r, c]).any()  # (the planted injection: an assignment without a hole exists)
    return float(v[r, c].sum())


def _oracle_total(v, problem, **kw):
    n, m = v.shape
    (loc, val), = dense_to_packed(v[None], entries="finite")
    want = packed_expect(loc, val, problem, n, **kw)
    sol = want["sol"]
    assert want["meta"]["soln_found"] == 1 and want["N"] == n
    assert len(set(sol.tolist())) == n and sol.min() >= 0 and sol.max() < m and not np.isnan(v[np.arange(n), sol]).any()
    return float(v[np.arange(n), sol].sum())


@pytest.mark.parametrize("problem", ["min", "max"])
def test_the_oracle_on_the_packed_problem_is_optimal(problem):
    """200 signed integer-valued problems with n <= m < 40 and NaN holes: with `fast` (one phase at eps = 1 / n from zero
    prices: within n * eps = 1 of the optimum, and totals are integers) the oracle reaches scipy's optimum, and on the
    square ones so does the default eps-scaling."""
    squares = 0
    for k in range(DRAWS):
        v = _draw(k)
        best = _optimum(v, problem)
        assert _oracle_total(v, problem, fast=True) == best, k
        if v.shape[0] == v.shape[1]:
            squares += 1
            assert _oracle_total(v, problem) == best, k
    assert squares >= DRAWS // 2
