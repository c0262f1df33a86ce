"""The outside mode of auction_solve_ell_batch (misslap_solve_ell_batch_outside) without a GPU: the definition
(`ell_to_packed(outside=)` against a plain double loop), the front end's checks and its resolution of `fast`, the C entry
point's argument errors, the workspace size, and the optimality of the definition: on the augmented problem the oracle's
single phase (fast=True) reaches the optimum of scipy's linear_sum_assignment on every draw.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_ell_batch, ell_to_packed
from tests._batch_shapes import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_ell_batch_outside", "misslap_ell_batch_outside_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name


# ---- ell_to_packed(outside=) is the definition

def packed_by_loops(cols, vals, rows, outside):
    """The entries of rows 0 .. rows[b] - 1 in row order, within a row in slot order, holes dropped, and behind the
    slots of row i the entry (i, m_b + i) with the row's outside value; m_b = max real column + 1 (0 without entries)."""
    B, N, K = cols.shape
    out = []
    for b in range(B):
        n = N if rows is None else int(rows[b])
        m = 0
        for i in range(n):
            for k in range(K):
                if cols[b, i, k] >= 0:
                    m = max(m, int(cols[b, i, k]) + 1)
        loc, val = [], []
        for i in range(n):
            for k in range(K):
                if cols[b, i, k] >= 0:
                    loc.append((i, int(cols[b, i, k])))
                    val.append(float(vals[b, i, k]))
            loc.append((i, m + i))
            o = outside if np.ndim(outside) == 0 else outside[b] if np.ndim(outside) == 1 else outside[b, i]
            val.append(float(o))
        out.append((np.array(loc, dtype=np.int32).reshape(-1, 2), np.array(val, dtype=np.float64)))
    return out


def _stack():
    rng = np.random.default_rng(5)
    B, N, K = 5, 6, 7
    cols = rng.integers(0, 9, (B, N, K)).astype(np.int64)
    vals = rng.uniform(0, 10, (B, N, K))
    cols[0, :, :2] = -1                      # holes in front
    cols[1, :, 2:5] = (-1, -7, -(2**40))     # ... in the middle
    cols[2] = -3                             # a problem of holes only
    cols[3][rng.random((N, K)) < 0.5] = -1   # ... anywhere
    cols[4, 2] = -1                          # an empty row
    vals[cols < 0] = np.nan
    return cols, vals, np.array([6, 3, 2, 6, 4], dtype=np.int32)


@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("vtype", [np.float64, np.float32])
@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
@pytest.mark.parametrize("with_rows", [False, True])
def test_ell_to_packed_with_outside_is_the_double_loop(itype, vtype, form, with_rows):
    cols, vals, rows = _stack()
    cols = np.maximum(cols, -(2**31)).astype(itype)
    vals = vals.astype(vtype)
    B, N, K = cols.shape
    rng = np.random.default_rng(7)
    outside = {"scalar": 2.5, "per_problem": rng.uniform(0, 10, B), "per_row": rng.uniform(0, 10, (B, N))}[form]
    r = rows if with_rows else None
    got, want = ell_to_packed(cols, vals, r, outside=outside), packed_by_loops(cols, vals, r, outside)
    assert len(got) == len(want) == B
    for b, ((gl, gv), (wl, wv)) in enumerate(zip(got, want)):
        n = int(rows[b]) if with_rows else N
        assert gl.dtype == np.int32 and gv.dtype == np.float64 and gl.shape == wl.shape and gl.flags.c_contiguous
        assert np.array_equal(gl, wl) and np.array_equal(bits(gv), bits(wv)), b
        real = cols[b, :n][cols[b, :n] >= 0]
        m = int(real.max()) + 1 if real.size else 0
        last = np.flatnonzero(np.diff(np.append(gl[:, 0], n)))  # the last stored entry of every row
        assert np.array_equal(gl[last], np.stack([np.arange(n), m + np.arange(n)], axis=1)), b
    assert got[2][0].shape[0] == (2 if with_rows else N) and (got[2][0][:, 1] == got[2][0][:, 0]).all()  # holes only: m = 0
    # without outside nothing changes
    for (gl, gv), (wl, wv) in zip(ell_to_packed(cols, vals, r), ell_to_packed(cols, vals, r, outside=None)):
        assert np.array_equal(gl, wl) and np.array_equal(bits(gv), bits(wv))
    with pytest.raises(ValueError, match="outside must"):
        ell_to_packed(cols, vals, outside=np.zeros(B + 1))


# ---- the front end: checks before the FFI, and the resolution of `fast`

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


class _FakeDeviceTensor:
    is_cuda = True

    def data_ptr(self):
        return 0


COLS = np.array([[[0, 1, -1], [1, -1, 0]], [[2, 0, 1], [-1, -1, 1]]], dtype=np.int32)
VALS = np.arange(12, dtype=np.float64).reshape(2, 2, 3)


def test_outside_is_checked_before_the_ffi(no_ffi):
    f = auction_solve_ell_batch
    for bad in (float("nan"), float("inf"), -np.inf, np.float64("nan")):
        with pytest.raises(ValueError, match="outside must be finite"):
            f(COLS, VALS, outside=bad)
    for bad in (np.zeros(2, dtype=np.float32), np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="outside must be float64"):
            f(COLS, VALS, outside=bad)
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((2, 2, 1)), np.zeros((1, 2)), np.zeros(())):
        with pytest.raises(ValueError, match="outside must have shape"):
            f(COLS, VALS, outside=bad)
    with pytest.raises(TypeError, match="outside on the device"):  # a device tensor with host input: the wrong side
        f(COLS, VALS, outside=_FakeDeviceTensor())
    for bad in ("1.0", [1.0, 2.0], object(), True):
        with pytest.raises(TypeError, match="outside must be a float"):
            f(COLS, VALS, outside=bad)
    # what belongs to one problem or one row does not raise: the library is reached
    for ok in (0.0, 3, np.float32(1.5), np.array([1.0, np.nan]), np.full((2, 2), np.inf)):
        with pytest.raises(_NoFFI):
            f(COLS, VALS, outside=ok)


class _Recorder:
    """Stands in for the library: records what the front end passes and fills nothing."""

    def __init__(self):
        self.calls = []

    def _solve(self, name, fast_at, opts_at):
        def call(*args):
            opts = args[opts_at]._obj
            self.calls.append(dict(name=name, fast=args[fast_at], eps_start=opts.eps_start, maximize=opts.maximize,
                                   max_iter=opts.max_iter, args=args))
            if name.endswith("outside") and args[16] == 0:  # (read now: the array lives as long as the call)
                self.calls[-1]["outside"] = np.ctypeslib.as_array(C.cast(args[15], C.POINTER(C.c_double)), (2,)).copy()
            raise _NoFFI()
        return call

    def __getattr__(self, name):
        if name == "misslap_solve_ell_batch":
            return self._solve(name, 7, 11)
        if name == "misslap_solve_ell_batch_outside":
            return self._solve(name, 7, 10)
        raise AttributeError(name)


def _record(monkeypatch, **kw):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with pytest.raises(_NoFFI):
        auction_solve_ell_batch(COLS, VALS, **kw)
    (call,) = rec.calls
    return call


def test_fast_is_resolved_in_the_front_end(monkeypatch):
    # without outside: today's call and today's options, whether fast is left alone or given
    for kw, fast, eps in ((dict(), 0, 0.0), (dict(fast=False), 0, 0.0), (dict(fast=True), 1, 0.0),
                          (dict(eps_start=0.5), 0, 0.5), (dict(fast=True, eps_start=0.25), 1, 0.25), (dict(fast=None), 0, 0.0)):
        c = _record(monkeypatch, **kw)
        assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_ell_batch", fast, eps), kw
        assert c["args"][10] == 1 and c["max_iter"] == 1000000 and c["maximize"] == 0  # cardinality_check, as always
    # with outside: a single phase unless eps_start > 0 was given; explicit settings pass through
    for kw, fast, eps in ((dict(), 1, 0.0), (dict(eps_start=0.5), 0, 0.5), (dict(eps_start=1e-3), 0, float(np.float32(1e-3))),
                          (dict(fast=False), 0, 0.0), (dict(fast=True, eps_start=0.5), 1, 0.5), (dict(fast=True), 1, 0.0),
                          (dict(eps_start=0.0), 1, 0.0)):
        c = _record(monkeypatch, outside=1.0, problem="max", **kw)
        assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_ell_batch_outside", fast, eps), kw
        assert c["maximize"] == 1
    # the scalar travels as one value per problem (outside_ld = 0), the (B, N) form with outside_ld = N
    c = _record(monkeypatch, outside=2.0)
    assert c["args"][16] == 0
    assert np.array_equal(c["outside"], [2.0, 2.0])
    assert _record(monkeypatch, outside=np.array([1.0, 2.0]))["args"][16] == 0
    assert _record(monkeypatch, outside=np.ones((2, 2)))["args"][16] == 2


# ---- the C entry point and the workspace

def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_ell_batch_outside_workspace_bytes
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for B, N, K, M in ((1, 1, 1, 1), (2, 7, 3, 5), (64, cap, 16, cap), (100000, 256, 129, 40), (2**31 - 1, 1, 1, 1)):
        a, b = f(B, N, K, M, 0), f(B, N, K, M, 1)
        assert a > 0 and a % 256 == 0 and b % 256 == 0, (B, N, K, M)
        assert b >= a + 8 * B * (M + N)  # the staged starting prices of the augmented problems
        assert a == f(B, N, K, 1, 0)     # without prices the bound on the columns costs nothing
    assert f(1024, 64, 8, 64, 0) >= 1024 * 32  # a check record per problem
    for bad in ((0, 4, 4, 4), (2**31, 4, 4, 4), (1, 0, 4, 4), (1, cap + 1, 4, 4), (1, 4, 0, 4), (1, 2, 2**30, 4),
                (1, 4, 4, 0), (1, 4, 4, cap + 1), (1, 4, 4, -1)):
        assert f(*bad, 1) == -1, bad


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    cols = np.array([[[0, -1], [1, 0]]], dtype=np.int32)
    vals = np.array([[[1.0, 9.0], [2.0, 3.0]]])
    outside = np.array([[4.0, 5.0, 6.0]])
    sol, status = np.empty((1, 2), dtype=np.int32), np.empty(1, dtype=np.int32)
    oprices = np.empty((1, 2))
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, N=2, K=2, Mmax=2, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0, out=outside.ctypes.data,
             ld=0, prices=None, p_ld=0):
        return built_lib.misslap_solve_ell_batch_outside(
            B, N, K, cols.ctypes.data, 0, vals.ctypes.data, None, 1, prices, p_ld, C.byref(opts), None, work, nwork, Mmax,
            out, ld, sol.ctypes.data, None, oprices.ctypes.data, on_dev, st, None, C.cast(metas, C.c_void_p), None)

    err = built_lib.misslap_last_error
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for ld in (1, -1, -2048):  # outside_ld: 0 or >= N
        assert call(ld=ld) == _lib.ERR_INVALID and b"outside_ld" in err(), ld
    assert call(out=None) == _lib.ERR_INVALID and b"outside" in err()
    assert call(N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_SPARSE_BATCH_MAX_DIM" in err()
    assert call(Mmax=cap + 1) == _lib.ERR_INVALID and b"Mmax" in err()
    assert call(Mmax=0) == _lib.ERR_INVALID and call(B=0) == _lib.ERR_INVALID
    assert call(K=0) == _lib.ERR_INVALID and b"K must be" in err()
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    assert call(prices=vals.ctypes.data, p_ld=0) == _lib.ERR_INVALID and b"prices_ld" in err()
    need = built_lib.misslap_ell_batch_outside_workspace_bytes(1, 2, 2, 2, 0)
    dev = _lib.Options()
    C.memmove(C.byref(dev), C.byref(o), C.sizeof(o))
    dev.input_on_device = 1
    assert call(work=4096, nwork=need, on_dev=1) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1, opts=dev) == _lib.ERR_INVALID and b"workspace" in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1, opts=dev) == _lib.ERR_INVALID  # misaligned
    for ld in (0, 2, 3):  # valid host arguments: only the GPU can be missing
        rc = call(ld=ld)
        assert rc in (0, _lib.ERR_NO_DEVICE), err()
        if rc:
            assert b"no CPU fallback" in err()


# ---- the definition is optimal under the default the front end chooses

DRAWS = 600


def _draw(rng, t):
    n, m, K = (int(x) for x in (rng.integers(1, 45), rng.integers(1, 45), rng.integers(1, 9)))
    cols = np.stack([rng.permutation(max(m, K))[:K] for _ in range(n)]).astype(np.int64)
    cols[cols >= m] = -1
    cols[rng.random((n, K)) < 0.25] = -1
    vals = rng.integers(0, 20, (n, K)).astype(np.float64)
    outside = rng.integers(0, 20, n).astype(np.float64) if rng.random() < 0.5 else float(rng.integers(0, 20))
    return n, m, cols, vals, outside, ("min", "max")[t % 2]


def test_single_phase_on_the_augmented_problem_is_optimal():
    """600 draws (integer values, so eps = 1 / n < the gap between two objectives): the oracle with fast=True on
    ell_to_packed(outside=) reports eCE = 1 and its objective is linear_sum_assignment's on the augmented matrix,
    missing entries at +-1e6, within 1e-9.  Every draw counts."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(1)
    seen = dict(min=0, max=0, unmatched=0, matched=0, tall=0)
    for t in range(DRAWS):
        n, m, cols, vals, outside, problem = _draw(rng, t)
        o = np.broadcast_to(np.asarray(outside, dtype=np.float64), (n,))
        (loc, val), = ell_to_packed(cols[None], vals[None], outside=np.ascontiguousarray(o)[None])
        mb = int(cols.max()) + 1 if (cols >= 0).any() else 0
        assert loc.shape[0] == int((cols >= 0).sum()) + n and mb <= m
        res = orc.auction_solve(loc=loc, val=val.copy(), size=(mb + n, n), problem=problem, fast=True)
        assert res["meta"]["eCE"] == 1, t
        sol = np.asarray(res["sol"])
        assert (sol >= 0).all() and len(set(sol.tolist())) == n, t
        missing = 1e6 if problem == "min" else -1e6
        full = np.full((n, mb + n), missing)
        for (i, j), v in zip(loc, val):  # (a row's columns are distinct: no entry is stored twice)
            full[i, j] = v
        ri, ci = lsa(full, maximize=problem == "max")
        best = float(full[ri, ci].sum())
        assert abs(res["extra"]["obj_f64"] - best) <= 1e-9, (t, problem, res["extra"]["obj_f64"], best)
        seen[problem] += 1
        seen["unmatched"] += int((sol >= mb).sum())
        seen["matched"] += int((sol < mb).sum())
        seen["tall"] += n > mb
    assert seen["min"] == seen["max"] == DRAWS // 2
    assert seen["unmatched"] > 0 and seen["matched"] > 0 and seen["tall"] > 0  # both answers occur, and n_b > m_b too
