"""The whitening matrix per row of the points batch (whiten=, misslap_solve_points_batch_whitened,
misslap_points_batch_candidates_whitened) without a GPU: the symbols, the definition points_to_dense(whiten=) against a
plain loop and against the fused chain it must not be, what is read and what is not, the edge values of the chain, the
front end's whole-call errors, the C entry points' argument errors, the gate (the optimum over the in-gate pairs is the
optimum of the full problem with outside) and points_to_ell(whiten=) against a brute-force restatement.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, auction_solve_points_batch, points_candidates, points_to_dense, points_to_ell
from tests._batch_shapes import bits
from tests._points_fixture import DTYPES, dense_by_loops, draw
from tests._points_whiten import (WHITEN_DIMS, draw_whiten, expected_status, identity_whiten, inf_minus_inf_case,
                                  verdict_batch, whitened_by_loops, whitened_fused_by_loops)
from tests.test_points_batch_nogpu import _FakeDeviceTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_points_batch_whitened", "misslap_points_batch_candidates_whitened")
TAIL = ("const void *, int64_t, int64_t, int64_t, const void *, int64_t, int64_t, int64_t, const void *, int64_t, int64_t, "
        "int64_t, int64_t, ")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "#define MISSLAP_ABI_VERSION 2\n" in header and built_lib.misslap_abi_version() == 2
    assert "#define MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS 4\n" in header
    assert _lib.POINTS_BATCH_MAX_WHITEN_COORDS == 4 and sslap_amd.points_batch.MAX_WHITEN_COORDS == 4
    # the plain entry points keep their signatures
    assert len(_lib.SYMBOLS["misslap_solve_points_batch_whitened"][1]) == len(_lib.SYMBOLS["misslap_solve_points_batch"][1]) + 5
    assert len(_lib.SYMBOLS["misslap_points_batch_candidates_whitened"][1]) == \
        len(_lib.SYMBOLS["misslap_points_batch_candidates"][1]) + 5


def test_the_header_is_c99_with_the_new_prototypes():
    prog = ['#include "misslap.h"', 'int main(void){',
            'int (*f)(int64_t, int64_t, int64_t, int64_t, ' + TAIL,
            '         const int32_t *, int32_t, const double *, const misslap_options *, void *, void *,',
            '         int64_t, const double *, int64_t, int32_t *, double *, double *, int32_t, int32_t *, int32_t *,',
            '         misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_points_batch_whitened;',
            'int (*g)(int64_t, int64_t, int64_t, int64_t, ' + TAIL,
            '         int64_t, const int32_t *, const double *, int64_t, const misslap_options *, void *, int32_t *,',
            '         double *, int32_t *, int32_t *) = misslap_points_batch_candidates_whitened;',
            'return (f == 0) + (g == 0) + (MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS != 4);}']
    for std in ("c99", "c11"):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write("\n".join(prog))
            subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Werror", "-pedantic", "-c", "-I",
                                   os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t.o")])


def test_build_sees_the_new_header():
    from sslap_amd import build
    unit = open(os.path.join(build.CSRC, "misslap.hip")).read()
    for name in re.findall(r'#include "([a-z_0-9]+\.hpp)"', unit):
        assert name in build.SOURCES, name
    order = re.findall(r'#include "([a-z_0-9]+\.hpp)"', unit)
    mine = ["kernels_points_whiten.hpp", "abi_points_whiten.hpp"]
    # behind what existed: no kernel above is instantiated or scheduled differently for them
    assert order[order.index(mine[0]):][:2] == mine and order.index(mine[0]) > order.index("abi_points_candidates.hpp")
    for name in mine:
        assert name in build.SOURCES and os.path.exists(os.path.join(build.CSRC, name)), name


# ---- the definition

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_the_definition_is_the_loop_and_not_the_fused_chain(dtype, D):
    rng = np.random.default_rng([12, D])
    B, N, M = 3, 7, 6
    x, y = draw("uniform", (B, N, D), dtype, rng), draw("uniform", (B, M, D), dtype, rng)
    w = draw_whiten("uniform", (B, N, D, D), dtype, rng)
    got = points_to_dense(x, y, whiten=w)
    assert got.dtype == np.float64 and got.shape == (B, N, M) and got.flags.c_contiguous
    assert np.array_equal(bits(got), bits(whitened_by_loops(x, y, w)))
    assert np.isfinite(got).all() and not np.signbit(got).any()
    shapes = np.array([[7, 6], [1, 1], [4, 5]])
    with_shapes = points_to_dense(x, y, shapes, whiten=w)
    assert np.array_equal(bits(with_shapes), bits(whitened_by_loops(x, y, w, shapes)))
    assert np.isposinf(with_shapes[1, 1:]).all() and np.isposinf(with_shapes[2, :, 5:]).all()
    zeroed = np.where(np.isnan(w), 0, w).astype(dtype)
    differ = int((bits(whitened_fused_by_loops(x, y, zeroed)) != bits(got)).sum())
    if D == 1:
        assert differ == 0
    elif dtype == "float64":
        assert differ >= 1, differ
    import torch
    assert np.array_equal(bits(points_to_dense(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(shapes),
                                               whiten=torch.from_numpy(w))), bits(with_shapes))
    # whiten=None is the plain definition, untouched
    assert np.array_equal(bits(points_to_dense(x, y, shapes, whiten=None)), bits(dense_by_loops(x, y, shapes)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_the_identity_gives_the_plain_cost_bit_for_bit(dtype, D):
    rng = np.random.default_rng([13, D])
    x, y = draw("uniform", (2, 9, D), dtype, rng), draw("uniform", (2, 8, D), dtype, rng)
    got = points_to_dense(x, y, whiten=identity_whiten(2, 9, D, dtype))
    assert np.array_equal(bits(got), bits(points_to_dense(x, y)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_the_upper_triangle_and_rows_beyond_the_shape_are_never_read(dtype, D):
    rng = np.random.default_rng([14, D])
    B, N, M = 3, 6, 5
    x, y = draw("grid", (B, N, D), dtype, rng), draw("grid", (B, M, D), dtype, rng)
    shapes = np.array([[6, 5], [2, 3], [4, 1]])
    w = draw_whiten("grid", (B, N, D, D), dtype, rng)
    for b, (n, _) in enumerate(shapes):
        w[b, n:] = np.nan
    clean = np.where(np.isnan(w), 0, w).astype(dtype)
    got = points_to_dense(x, y, shapes, whiten=w)  # (a NaN that entered an operation would reach a cost)
    assert np.array_equal(bits(got), bits(points_to_dense(x, y, shapes, whiten=clean)))
    assert np.isfinite(got[0]).all() and not np.signbit(got).any()
    a, z = points_to_ell(x, y, 4, shapes, limit=30.0, whiten=w), points_to_ell(x, y, 4, shapes, limit=30.0, whiten=clean)
    for key in a:
        assert np.array_equal(a[key].view(np.uint8), z[key].view(np.uint8)), key


def test_edge_values_of_the_chain():
    x = np.array([[[1.0, 2.0], [1.0, 2.0], [1e100, 0.0], [0.0, 0.0]]])
    y = np.array([[[0.0, 0.0], [-1e100, 0.0]]])
    w = np.zeros((1, 4, 2, 2))
    w[0, :, 0, 0] = w[0, :, 1, 1] = 1.0
    w[0, 0, 1, 0] = np.nan       # a matrix element that is read: NaN
    w[0, 1, 0, 0] = np.inf       # ... and an infinite one
    w[0, 2, 0, 0] = 1e100        # plain overflow: z = 1e200 or 2e200 is finite, z * z = +inf
    c = points_to_dense(x, y, whiten=w)
    assert np.isnan(c[0, 0]).all() and not np.isfinite(c[0, 1]).any()
    assert np.isposinf(c[0, 2]).all()
    assert np.array_equal(bits(c[0, 3, :1]), bits(np.array([0.0])))  # +0.0, never -0.0
    assert c[0, 3, 1] == 1e200
    # the new trap: finite inputs, a NaN cost (two products overflow to +inf and -inf)
    xi, yi, wi = inf_minus_inf_case()
    assert np.isfinite(xi).all() and np.isfinite(wi[0, 0][np.tril_indices(2)]).all()
    assert np.isnan(points_to_dense(xi, yi, whiten=wi)).all()
    assert np.isnan(whitened_by_loops(xi, yi, wi)).all()


def test_the_definition_rejects_what_the_call_rejects():
    x, y = np.zeros((2, 3, 2)), np.zeros((2, 4, 2))
    for bad in (np.zeros((2, 3, 2)), np.zeros((2, 3, 2, 2), dtype=np.float32), np.zeros((2, 3, 3, 3)),
                np.zeros((1, 3, 2, 2)), np.zeros((2, 4, 2, 2))):
        with pytest.raises(ValueError, match="whiten"):
            points_to_dense(x, y, whiten=bad)
    with pytest.raises(ValueError, match="MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS"):
        points_to_dense(np.zeros((1, 2, 5)), np.zeros((1, 2, 5)), whiten=np.zeros((1, 2, 5, 5)))


# ---- the front end: every whole-call error raises before the library is reached

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    """The library is never reached: loading it, and the builder's launch on device tensors, raise _NoFFI."""
    def no_load(*args, **kw):
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(sslap_amd.points_batch, "_candidates_launch", no_load)


X = np.arange(24, dtype=np.float64).reshape(2, 4, 3)
Y = np.arange(30, dtype=np.float64).reshape(2, 5, 3) / 7
W = np.ones((2, 4, 3, 3))


@pytest.mark.parametrize("call", ["solve", "candidates", "route"])
def test_whole_call_errors_are_raised_before_the_library(no_ffi, call):
    import torch

    def f(x=X, y=Y, whiten=W, **kw):
        if call == "solve":
            return auction_solve_points_batch(x, y, whiten=whiten, **kw)
        if call == "candidates":
            return points_candidates(x, y, 4, whiten=whiten, **kw)
        return auction_solve_points_batch(x, y, whiten=whiten, candidates=4, **kw)

    with pytest.raises(ValueError, match="4 dimensions"):
        f(whiten=W[0])
    with pytest.raises(ValueError, match="dtype of x and y, float64, got float32"):
        f(whiten=W.astype(np.float32))
    for bad in (np.ones((2, 4, 3, 2)), np.ones((1, 4, 3, 3)), np.ones((2, 5, 3, 3)), np.ones((2, 4, 2, 2))):
        with pytest.raises(ValueError, match="whiten must have shape"):
            f(whiten=bad)
    with pytest.raises(TypeError, match="whiten must be a numpy array"):
        f(whiten=_FakeDeviceTensor(W.shape, torch.float64))
    with pytest.raises(TypeError, match="whiten must be a numpy array"):
        f(whiten=W.tolist())
    x5, y5 = np.zeros((2, 4, 5)), np.zeros((2, 5, 5))
    with pytest.raises(ValueError, match="MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS"):
        f(x=x5, y=y5, whiten=np.ones((2, 4, 5, 5)))
    fx, fy = _FakeDeviceTensor(X.shape, torch.float64), _FakeDeviceTensor(Y.shape, torch.float64)
    with pytest.raises(TypeError, match="whiten must be a tensor on the device"):
        f(x=fx, y=fy, whiten=W)
    with pytest.raises(ValueError, match="whiten is on cuda:1, x on cuda:0"):
        f(x=fx, y=fy, whiten=_FakeDeviceTensor(W.shape, torch.float64, index=1))
    with pytest.raises(ValueError, match="whiten has strides .*a stride must be >= 0"):
        f(x=fx, y=fy, whiten=_FakeDeviceTensor(W.shape, torch.float64, (36, 9, -3, 1)))
    with pytest.raises(ValueError, match="dtype of x and y, float64, got float32"):
        f(x=fx, y=fy, whiten=_FakeDeviceTensor(W.shape, torch.float32))
    # a good call reaches the library
    with pytest.raises(_NoFFI):
        if call == "solve":
            f()
        else:  # (one matrix for the call, expanded: strides of 0)
            f(x=fx, y=fy, whiten=_FakeDeviceTensor(W.shape, torch.float64, (0, 0, 3, 1)))


def test_reverse_finish_with_whiten_needs_the_list_route(no_ffi):
    import torch
    with pytest.raises(ValueError, match="candidates=K"):
        auction_solve_points_batch(X, Y, whiten=W, outside=1.0, finish="reverse")
    fx, fy, fw = (_FakeDeviceTensor(a.shape, torch.float64) for a in (X, Y, W))
    with pytest.raises(ValueError, match="candidates=K"):
        auction_solve_points_batch(fx, fy, whiten=fw, finish="reverse")
    with pytest.raises(_NoFFI):  # ... which takes it
        auction_solve_points_batch(fx, fy, whiten=fw, finish="reverse", candidates=4)


def test_the_status_text_of_code_3_names_the_matrix():
    from sslap_amd._batch import _STATUS_ERRORS
    res = dict(stack=(4, 5), whitened=True)
    text = str(_STATUS_ERRORS["points"](res, 1, _lib.BATCH_STATUS_INFINITE_VALUE, 4, 5, -1))
    assert text.startswith("problem 1: ") and "whitening matrix" in text and "W_i" in text
    plain = str(_STATUS_ERRORS["points"](dict(stack=(4, 5)), 1, _lib.BATCH_STATUS_INFINITE_VALUE, 4, 5, -1))
    assert "whitening" not in plain and "|x_i - y_j|^2" in plain


# ---- the C entry points

def test_c_entry_points_validate_the_matrix(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    x, y, w = np.zeros((1, 2, 3)), np.ones((1, 2, 3)), np.ones((1, 2, 3, 3))
    sol, status = np.empty((1, 2), dtype=np.int32), np.empty(1, dtype=np.int32)
    prices = np.empty((1, 2))
    err = built_lib.misslap_last_error

    def solve(D=3, wp=w.ctypes.data, ws=(18, 9, 3, 1), opts=o, B=1):
        return built_lib.misslap_solve_points_batch_whitened(
            B, 2, 2, D, x.ctypes.data, 2 * D, D, 1, y.ctypes.data, 2 * D, D, 1, wp, *ws, None, 0, None, C.byref(opts), None,
            None, 0, None, 0, sol.ctypes.data, prices.ctypes.data, None, 0, status.ctypes.data, None, None, None)

    assert solve(wp=None) == _lib.ERR_INVALID and b"null w" in err()
    assert solve(ws=(18, 9, 1, 3)) == _lib.ERR_INVALID and b"a strided w is a device array" in err()
    assert solve(ws=(0, 0, 3, 1)) == _lib.ERR_INVALID and b"a strided w is a device array" in err()
    assert solve(ws=(18, 9, -3, 1)) == _lib.ERR_INVALID and b"a stride must be >= 0" in err()
    assert solve(ws=(2**62, 9, 3, 1), B=2) == _lib.ERR_INVALID and b"62 bits" in err()
    assert solve(D=5, ws=(50, 25, 5, 1)) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS" in err()
    assert solve(D=9) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_COORDS" in err()

    od = _lib.Options()
    od.struct_size = C.sizeof(_lib.Options)
    od.input_on_device = 1
    out = (np.empty(8, dtype=np.int32), np.empty(8), np.empty(2, dtype=np.int32), np.empty(1, dtype=np.int32))

    def cand(D=3, wp=w.ctypes.data, ws=(18, 9, 3, 1), K=4):
        return built_lib.misslap_points_batch_candidates_whitened(
            1, 2, 2, D, x.ctypes.data, 2 * D, D, 1, y.ctypes.data, 2 * D, D, 1, wp, *ws, K, None, None, 0, C.byref(od), None,
            *(a.ctypes.data for a in out))

    assert cand(wp=None) == _lib.ERR_INVALID and b"null w" in err()
    assert cand(D=5, ws=(50, 25, 5, 1)) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS" in err()
    assert cand(ws=(18, 9, 3, -1)) == _lib.ERR_INVALID and b"a stride must be >= 0" in err()
    assert cand(K=65) == _lib.ERR_INVALID and b"MISSLAP_POINTS_CANDIDATES_MAX_K" in err()


# ---- the gate: outside in the units of the whitened cost

def test_the_optimum_over_the_in_gate_pairs_is_the_optimum_with_outside():
    """400 draws, none skipped: integer coordinates and integer triangles (exact costs), D 1 .. 4, n, m <= 8 and an
    integer outside value per row.  The full problem -- every pair, or the row's outside value -- and the problem
    without the pairs dearer than their row's outside value have the same optimum: outside is the chi-square gate."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(31)
    pruned = unmatched = 0
    for t in range(400):
        D, n, m = int(rng.integers(1, 5)), int(rng.integers(1, 9)), int(rng.integers(1, 9))
        x = rng.integers(0, 8, (1, n, D)).astype(np.float64)
        y = rng.integers(0, 8, (1, m, D)).astype(np.float64)
        w = draw_whiten("grid", (1, n, D, D), "float64", rng)
        outside = rng.integers(0, 1 + int(rng.integers(1, 200)), n).astype(np.float64)
        cost = points_to_dense(x, y, whiten=w)[0]
        assert (cost == np.round(cost)).all()
        big = 1e9
        virt = np.full((n, n), big)
        virt[np.arange(n), np.arange(n)] = outside
        full = np.concatenate([cost, virt], axis=1)
        gated = np.concatenate([np.where(cost <= outside[:, None], cost, big), virt], axis=1)
        (r, c), (r2, c2) = lsa(full), lsa(gated)
        assert float(full[r, c].sum()) == float(gated[r2, c2].sum()), t
        pruned += int((cost > outside[:, None]).sum())
        unmatched += int((c2 >= m).sum())
    assert pruned > 1000 and unmatched > 100


# ---- points_to_ell(whiten=) against a brute-force restatement

def _ell_by_brute_force(cost, shapes, k, limit):
    B, N, M = cost.shape
    cols, vals = np.full((B, N, k), -1, dtype=np.int32), np.zeros((B, N, k))
    counts, rows = np.zeros((B, N), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        n, m = (int(v) for v in shapes[b])
        if not (1 <= n <= N and 1 <= m <= M):
            continue
        rows[b] = n
        for i in range(n):
            cand = [(-1.0 if not np.isfinite(cost[b, i, j]) else cost[b, i, j], j) for j in range(m)
                    if not np.isfinite(cost[b, i, j]) or cost[b, i, j] <= limit[b, i]]
            counts[b, i] = len(cand)
            kept = sorted(j for _, j in sorted(cand)[:k])
            for s, j in enumerate(kept):
                cols[b, i, s], vals[b, i, s] = j, cost[b, i, j] if np.isfinite(cost[b, i, j]) else np.inf
    return dict(cols=cols, vals=vals, counts=counts, rows=rows)


@pytest.mark.parametrize("dtype", DTYPES)
def test_points_to_ell_with_whiten_is_the_brute_force_lists(dtype):
    v = verdict_batch(dtype, D=2)
    x, y, w, shapes = v["x"], v["y"], v["w"], v["shapes"]
    B, N = x.shape[:2]
    cost = points_to_dense(x, y, shapes, whiten=w)
    rng = np.random.default_rng(6)
    limit = rng.uniform(0.2, 2.0, (B, N))
    for k in (1, 3, 11):
        got = points_to_ell(x, y, k, shapes, limit, whiten=w)
        want = _ell_by_brute_force(cost, shapes, k, limit)
        for key in ("cols", "counts", "rows"):
            assert np.array_equal(got[key], want[key]), (k, key)
        assert np.array_equal(bits(got["vals"]), bits(want["vals"])), k
    # non-finite costs are keyed first and stored as +inf; the statuses are the definition's
    status, _ = expected_status(x, y, w, shapes, outside=v["outside"])
    bad = [b for b, kind in enumerate(v["kinds"]) if kind in ("nan_triangle", "inf_w000", "overflow", "inf_minus_inf",
                                                              "nan_coord")]
    got = points_to_ell(x, y, 3, shapes, 0.0, whiten=w)
    for b in bad:
        assert status[b] == 3 and np.isposinf(got["vals"][b]).any(), v["kinds"][b]
    for b, kind in enumerate(v["kinds"]):
        if kind in ("ok", "nan_upper_only", "nan_rows_beyond"):
            assert status[b] == 0 and np.isfinite(got["vals"][b]).all(), kind
