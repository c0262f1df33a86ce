"""Candidate lists from two point sets (points_to_ell, points_candidates, auction_solve_points_batch(candidates=K);
misslap_points_batch_candidates) without a GPU: the definition against a brute-force restatement, at the edges of the
limit and of the non-finite costs; the theorem behind the route -- with an outside value per row and nothing truncated,
the optimum of the lists is the optimum of the full problem -- on the CPU oracle, every draw counting, and one truncated
example where it is not; the front end's checks before the library is reached; the declarations.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sslap_amd
from oracle import oracle as orc
from sslap_amd import (_lib, auction_solve_points_batch, dense_to_augmented, ell_to_packed, points_candidates,
                       points_to_dense, points_to_ell)
from tests._points_candidates import (DTYPES, FORMS, counted_rows, ell_by_loops, grid, limit_of, non_finite_batch,
                                      same_bytes, tied_rows)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "misslap_points_batch_candidates"


def test_entry_point_is_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    assert NAME in declared and NAME in _lib.SYMBOLS and getattr(built_lib, NAME) is not None
    assert NAME in header.split("Additions since")[1].split("*/")[0]
    assert len(_lib.SYMBOLS[NAME][1]) == 22
    assert "#define MISSLAP_ABI_VERSION 2\n" in header and built_lib.misslap_abi_version() == 2
    assert "#define MISSLAP_POINTS_CANDIDATES_MAX_K 64\n" in header and _lib.POINTS_CANDIDATES_MAX_K == 64
    for name in ("points_to_ell", "points_candidates", "auction_solve_points_batch"):
        assert name in sslap_amd.__all__ and callable(getattr(sslap_amd, name)), name
    from sslap_amd import build
    unit = open(os.path.join(build.CSRC, "misslap.hip")).read()
    order = re.findall(r'#include "([a-z_0-9]+\.hpp)"', unit)
    mine = ["kernels_points_candidates.hpp", "abi_points_candidates.hpp"]
    assert order[order.index(mine[0]):][:2] == mine and order.index(mine[0]) > order.index("abi_points_finish.hpp")
    assert all(name in build.SOURCES for name in mine)


# ---- points_to_ell is the definition: against the per-row loop

SHAPES = np.array([[7, 11], [3, 11], [7, 4], [0, 5], [8, 11], [1, 1], [7, 12], [5, 9]])  # cropped, bad (3, 4, 6), 1 x 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_points_to_ell_is_the_brute_force_loop(dtype, D):
    rng = np.random.default_rng([3, D])
    B, N, M = len(SHAPES), 7, 11
    x, y = grid((B, N, D), dtype, rng), grid((B, M, D), dtype, rng)
    seen = dict(truncated=0, full=0, empty=0)
    for form in FORMS:
        limit = limit_of(form, x, y, rng)
        for shapes in (None, SHAPES):
            for k in (1, 3, 11, 64):
                got, want = points_to_ell(x, y, k, shapes, limit), ell_by_loops(x, y, k, shapes, limit)
                assert same_bytes(got, want), (form, k, shapes is None)
                assert got["cols"].dtype == np.int32 and got["vals"].dtype == np.float64
                assert got["counts"].dtype == np.int32 and got["rows"].dtype == np.int32
                seen["truncated"] += int((got["counts"] > k).sum())
                seen["full"] += int((got["counts"] == k).sum())
                seen["empty"] += int((got["counts"] == 0).sum())
                if shapes is not None:
                    assert got["rows"].tolist() == [7, 3, 7, 0, 0, 1, 0, 5]
                    for b in (3, 4, 6):
                        assert (got["cols"][b] == -1).all() and not got["vals"][b].any() and not got["counts"][b].any()
                    assert not got["counts"][1, 3:].any() and (got["cols"][2] < 4).all()
    assert min(seen.values()) > 0, seen
    import torch
    t = points_to_ell(torch.from_numpy(x), torch.from_numpy(y), 3, torch.from_numpy(SHAPES), 2.0)
    assert same_bytes(t, ell_by_loops(x, y, 3, SHAPES, 2.0))


def test_an_untruncated_row_is_the_gate_in_column_order():
    rng = np.random.default_rng(2)
    x, y = grid((2, 6, 2), "float32", rng, 6), grid((2, 9, 2), "float32", rng, 6)
    c = points_to_dense(x, y)
    got = points_to_ell(x, y, 9, limit=8.0)
    for b in range(2):
        for i in range(6):
            (want,) = np.nonzero(c[b, i] <= 8.0)
            assert got["counts"][b, i] == want.size
            assert got["cols"][b, i, :want.size].tolist() == want.tolist() and (got["cols"][b, i, want.size:] == -1).all()
            assert np.array_equal(got["vals"][b, i, :want.size], c[b, i, want])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2, 5, 63, 64])
def test_rows_with_zero_k_and_k_plus_one_candidates(dtype, k):
    x, y, lim, counts = counted_rows(dtype, k, k + 3)
    got = points_to_ell(x, y, k, limit=lim)
    assert same_bytes(got, ell_by_loops(x, y, k, limit=lim))
    assert got["counts"][0].tolist() == counts.tolist()
    assert (got["cols"][0, 0] == -1).all()
    for i in (1, 2, 3):  # exactly k, and the k nearest of k + 1 and of all: columns 0 .. k - 1
        assert got["cols"][0, i].tolist() == list(range(k)), i
        assert got["vals"][0, i].tolist() == [float(j * j) for j in range(k)], i


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_limit_is_an_ieee_comparison(dtype):
    x = np.zeros((1, 6, 2), dtype=dtype)
    y = np.array([[[0, 0], [1, 0], [0, 0], [1, 1]]], dtype=dtype)  # costs 0, 1, 0, 2 for every row
    lim = np.array([[-0.0, 1.0, np.nan, np.inf, -1e-300, np.nextafter(1.0, 0.0)]])
    got = points_to_ell(x, y, 4, limit=lim)
    assert same_bytes(got, ell_by_loops(x, y, 4, limit=lim))
    assert got["counts"][0].tolist() == [2, 3, 0, 4, 0, 2]  # -0.0 admits +0.0; equal admits; a NaN none; +inf all
    assert got["cols"][0, 0].tolist() == [0, 2, -1, -1] and got["cols"][0, 1].tolist() == [0, 1, 2, -1]
    assert not np.signbit(got["vals"][0, 0]).any()
    assert same_bytes(points_to_ell(x, y, 4), points_to_ell(x, y, 4, limit=np.inf))
    for form in (np.nan, np.array([np.nan]), -0.0):
        assert same_bytes(points_to_ell(x, y, 2, limit=form), ell_by_loops(x, y, 2, limit=form))


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_that_straddle_the_kth_key_go_by_column(dtype):
    x, y = tied_rows(dtype, 11)
    for k in (1, 2, 3, 6, 10, 11):
        got = points_to_ell(x, y, k)
        assert same_bytes(got, ell_by_loops(x, y, k))
        assert got["counts"][0].tolist() == [11, 11]
        want = sorted([10] + list(range(k - 1))) if k < 11 else list(range(11))
        assert got["cols"][0, 0].tolist() == want, k


@pytest.mark.parametrize("dtype", DTYPES)
def test_costs_that_are_not_finite_are_candidates_first_and_stored_as_inf(dtype):
    x, y = non_finite_batch(dtype)
    for limit in (None, -1.0, 2.0, np.nan):
        for k in (1, 2, 5):
            got = points_to_ell(x, y, k, limit=limit)
            assert same_bytes(got, ell_by_loops(x, y, k, limit=limit)), (limit, k)
            assert not np.isnan(got["vals"]).any()
            # the NaN row: every column, so the first k in column order, all +inf
            assert got["counts"][0, 1] == 5 and got["cols"][0, 1].tolist() == list(range(min(k, 5)))
            assert np.isposinf(got["vals"][0, 1]).all()
            # the infinite column: a candidate of every row under any limit, and first under truncation
            for i in range(3):
                at = got["cols"][1, i].tolist()
                assert 2 in at and np.isposinf(got["vals"][1, i, at.index(2)]), (limit, k, i)
            if dtype == "float64":  # the overflow: row 0 against every column, every row against column 4
                assert np.isposinf(got["vals"][2, 0, :min(k, 5)]).all() and got["counts"][2, 0] == 5
                assert all(4 in got["cols"][2, i].tolist() for i in (1, 2))
            if limit == -1.0:  # nothing finite is admitted: only the non-finite costs are candidates
                assert got["counts"][3].tolist() == [0, 0, 0] and got["counts"][1].tolist() == [1, 1, 1]


# ---- the theorem: with an outside value per row and nothing truncated, the lists keep the optimum

def _lists_optimum(x, y, outside, k):
    """The oracle's single phase on the lists of one problem: (objective, truncated rows)."""
    ell = points_to_ell(x[None], y[None], k, limit=outside[None])
    (loc, val), = ell_to_packed(ell["cols"], ell["vals"], ell["rows"], outside=outside[None])
    n = x.shape[0]
    mb = int(ell["cols"].max()) + 1 if (ell["cols"] >= 0).any() else 0
    res = orc.auction_solve(loc=loc, val=val.copy(), size=(mb + n, n), problem="min", fast=True)
    assert res["meta"]["eCE"] == 1
    sol = np.asarray(res["sol"])
    assert (sol >= 0).all() and len(set(sol.tolist())) == n
    chosen = {(int(i), int(j)): float(v) for (i, j), v in zip(loc, val)}
    return sum(chosen[i, int(sol[i])] for i in range(n)), int((ell["counts"] > k).sum())


def _full_optimum(x, y, outside):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    (aug,) = dense_to_augmented(points_to_dense(x[None], y[None]), outside=outside[None])
    full = np.where(aug >= 0, aug, 1e9)
    r, c = lsa(full)
    return float(full[r, c].sum())


def test_untruncated_lists_keep_the_optimum_of_the_full_problem():
    """400 draws on integer coordinates 0 .. 7 with an integer outside value per row and k >= m: the oracle's single
    phase (fast=True) on the lists reaches scipy's optimum of the FULL augmented dense problem, exactly (integers, and
    n * eps < 1), on every draw: a pair dearer than its row's outside value is never in an optimal assignment."""
    rng = np.random.default_rng(29)
    pruned = unmatched = 0
    for t in range(400):
        D, n, m = int(rng.integers(1, 4)), int(rng.integers(1, 45)), int(rng.integers(1, 45))
        x = rng.integers(0, 8, (n, D)).astype(np.float64)
        y = rng.integers(0, 8, (m, D)).astype(np.float64)
        outside = rng.integers(0, 1 + int(rng.integers(1, 40)), n).astype(np.float64)
        k = int(rng.integers(m, 65))
        got, truncated = _lists_optimum(x, y, outside, k)
        assert truncated == 0
        want = _full_optimum(x, y, outside)
        assert got == want, (t, D, n, m, got, want)
        pruned += int((points_to_dense(x[None], y[None])[0] > outside[:, None]).sum())
        unmatched += got > 0
    assert pruned > 10000 and unmatched > 100  # the gate removed pairs, and the optimum was not trivially 0


def test_a_truncated_list_can_lose_the_optimum_and_says_so():
    """Two rows that both see columns 0 and 1 nearest, k = 1: each keeps column 0 only, one of them must take its
    outside value, and `counts > k` reports both rows."""
    x = np.array([[0.0], [0.0]])
    y = np.array([[1.0], [2.0]])
    outside = np.array([10.0, 10.0])
    full = _full_optimum(x, y, outside)
    assert full == 1.0 + 4.0
    got, truncated = _lists_optimum(x, y, outside, 1)
    assert truncated == 2 and got == 1.0 + 10.0 and got > full
    got, truncated = _lists_optimum(x, y, outside, 2)
    assert truncated == 0 and got == full


# ---- the front end without a GPU

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)
    import torch
    monkeypatch.setattr(torch, "from_numpy", lambda a: (_ for _ in ()).throw(_NoFFI()))  # (no upload either)


X = np.arange(24, dtype=np.float64).reshape(2, 4, 3)
Y = np.arange(30, dtype=np.float64).reshape(2, 5, 3) / 7


def test_argument_errors_raise_before_the_library_is_reached(no_ffi):
    for f in (lambda k, **kw: points_candidates(X, Y, k, **kw),
              lambda k, **kw: auction_solve_points_batch(X, Y, candidates=k, **kw),
              lambda k, **kw: points_to_ell(X, Y, k)):
        for bad in (0, 65, -1):
            with pytest.raises(ValueError, match="1 .. 64"):
                f(bad)
        for bad in (2.0, "3", True):
            with pytest.raises(TypeError, match="must be an integer"):
                f(bad)
    with pytest.raises(ValueError, match="problem='min'"):
        auction_solve_points_batch(X, Y, candidates=4, problem="max")
    with pytest.raises(ValueError, match="limit must have shape"):
        points_candidates(X, Y, 4, limit=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="limit must be float64"):
        points_candidates(X, Y, 4, limit=np.zeros(2, dtype=np.float32))
    with pytest.raises(TypeError, match="limit must be a float"):
        points_candidates(X, Y, 4, limit="1.0")
    with pytest.raises(ValueError, match="limit must be a float or have shape"):
        points_to_ell(X, Y, 4, limit=np.zeros(3))
    with pytest.raises(ValueError, match="outside must have shape"):
        auction_solve_points_batch(X, Y, candidates=4, outside=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="outside must be finite"):
        auction_solve_points_batch(X, Y, candidates=4, outside=float("inf"))
    with pytest.raises(ValueError, match="outside 1 .. 4 x 1 .. 5"):
        points_candidates(X, Y, 4, shapes=np.array([[4, 5], [5, 5]]))
    with pytest.raises(ValueError, match="one dtype"):
        points_candidates(X, Y.astype(np.float32), 4)
    with pytest.raises(ValueError, match="at most 2048 x 2048"):
        auction_solve_points_batch(np.zeros((1, 2049, 1)), np.zeros((1, 2, 1)), candidates=4)
    with pytest.raises(ValueError, match="eps_start is NaN"):
        auction_solve_points_batch(X, Y, candidates=4, eps_start=float("nan"))
    with pytest.raises(ValueError, match="finish must be left out or 'reverse'"):
        auction_solve_points_batch(X, Y, candidates=4, finish="forward")
    with pytest.raises(TypeError, match="finish=None"):
        auction_solve_points_batch(X, Y, candidates=4, finish=None)
    with pytest.raises(ValueError, match="errors must be"):
        auction_solve_points_batch(X, Y, candidates=4, errors="ignore")
    # what is the kernel's business reaches the upload: any float as a limit, any value in an array
    for ok in (dict(limit=-1.0), dict(limit=float("nan")), dict(limit=float("inf")), dict(limit=np.array([np.nan, -1.0])),
               dict(limit=np.full((2, 4), np.inf)), dict()):
        with pytest.raises(_NoFFI):
            points_candidates(X, Y, 4, **ok)
    for ok in (dict(), dict(outside=1.0), dict(outside=np.array([1.0, np.nan])), dict(finish="reverse")):
        with pytest.raises(_NoFFI):
            auction_solve_points_batch(X, Y, candidates=4, **ok)


def test_without_candidates_the_call_rejects_what_it_rejected(no_ffi):
    for unknown in ("cardinality_check", "mat_dtype", "entries", "limit", "k"):
        with pytest.raises(TypeError, match=unknown):
            auction_solve_points_batch(X, Y, **{unknown: None})
    with pytest.raises(TypeError, match="finish=None"):
        auction_solve_points_batch(X, Y, finish=None)
    with pytest.raises(ValueError, match="outside must be >= 0"):
        auction_solve_points_batch(X, Y, outside=-1.0)
    with pytest.raises(ValueError, match="prices must have shape"):
        auction_solve_points_batch(X, Y, prices=np.zeros((2, 4)))
    with pytest.raises(_NoFFI):  # candidates=None is the call without the keyword: problem="max" is taken
        auction_solve_points_batch(X, Y, candidates=None, problem="max")


def test_c_entry_point_validates_before_a_device_is_touched(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.input_on_device = 1
    buf = np.zeros(64)
    p = buf.ctypes.data

    def call(B=1, N=2, M=2, D=3, xp=p, xs=(6, 3, 1), yp=p, ys=(6, 3, 1), K=4, lim=None, ld=0, opts=o, cols=p, rows=p):
        return built_lib.misslap_points_batch_candidates(B, N, M, D, xp, *xs, yp, *ys, K, None, lim, ld, C.byref(opts), None,
                                                         cols, p, p, rows)

    err = built_lib.misslap_last_error
    for K in (0, 65, -3):
        assert call(K=K) == _lib.ERR_INVALID and b"MISSLAP_POINTS_CANDIDATES_MAX_K" in err(), K
    assert call(N=2049) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_DIM" in err()
    assert call(M=0) == _lib.ERR_INVALID and call(B=0) == _lib.ERR_INVALID
    for D in (0, 9):
        assert call(D=D) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_COORDS" in err()
    assert call(xp=None) == _lib.ERR_INVALID and b"null x" in err()
    assert call(cols=None) == _lib.ERR_INVALID and call(rows=None) == _lib.ERR_INVALID
    assert call(lim=p, ld=1) == _lib.ERR_INVALID and b"limit_ld" in err()
    assert call(xs=(6, -3, 1)) == _lib.ERR_INVALID and b"a stride must be >= 0" in err()
    assert call(ys=(6, 2**62, 1)) == _lib.ERR_INVALID and b"62 bits" in err()
    host = _lib.Options()
    host.struct_size = C.sizeof(_lib.Options)
    assert call(opts=host) == _lib.ERR_INVALID and b"input_on_device" in err()
    half = _lib.Options()
    half.struct_size = C.sizeof(_lib.Options)
    half.input_on_device = 1
    half.mat_dtype = _lib.DTYPE_F16
    assert call(opts=half) == _lib.ERR_INVALID and b"mat_dtype" in err()
