"""The outside mode of auction_solve_batch (misslap_solve_dense_batch_outside) without a GPU: the definition
(`dense_to_augmented` against a plain double loop), the front end's checks and its resolution of `fast`, the C entry
point's argument errors, the workspace size, and the optimality of the definition: on the augmented matrix the oracle's
single phase (fast=True) reaches the optimum of scipy's linear_sum_assignment on every draw.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sslap_amd
from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_batch, dense_to_augmented
from tests._batch_shapes import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_dense_batch_outside", "misslap_dense_batch_outside_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "dense_to_augmented" in sslap_amd.__all__ and sslap_amd.dense_to_augmented is dense_to_augmented
    codes = dict(re.findall(r"#define MISSLAP_BATCH_STATUS_([A-Z_]+) (\d+)", header))
    assert int(codes["BAD_OUTSIDE"]) == _lib.BATCH_STATUS_BAD_OUTSIDE == 15
    assert sorted(int(v) for v in codes.values()) == list(range(16))  # directly behind the others, none reused


# ---- dense_to_augmented is the definition

def augmented_by_loops(mats, shapes, outside):
    """aug_b[i][j] = mats[b][i][j] for j < m_b; aug_b[i][m_b + k] = row i's outside value for k == i, else -1."""
    B, N, M = mats.shape
    out = []
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        aug = np.empty((n, m + n), dtype=np.float64)
        for i in range(n):
            for j in range(m):
                aug[i, j] = float(mats[b, i, j])
            for k in range(n):
                o = outside if np.ndim(outside) == 0 else outside[b] if np.ndim(outside) == 1 else outside[b, i]
                aug[i, m + k] = float(o) if k == i else -1.0
        out.append(aug)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
@pytest.mark.parametrize("with_shapes", [False, True])
def test_dense_to_augmented_is_the_double_loop(dtype, form, with_shapes):
    rng = np.random.default_rng(5)
    B, N, M = 4, 6, 5
    mats = rng.uniform(0, 10, (B, N, M))
    mats[rng.random(mats.shape) < 0.4] = -1.0
    mats[1, 2] = np.nan  # a row without a valid entry
    mats = mats.astype(dtype)
    shapes = np.array([[6, 5], [3, 5], [1, 1], [6, 2]]) if with_shapes else None
    outside = {"scalar": 2.5, "per_problem": rng.uniform(0, 10, B), "per_row": rng.uniform(0, 10, (B, N))}[form]
    got, want = dense_to_augmented(mats, shapes, outside=outside), augmented_by_loops(mats, shapes, outside)
    assert len(got) == len(want) == B
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float64 and g.shape == w.shape and g.flags.c_contiguous, b
        assert np.array_equal(bits(g), bits(w)), b
        n = g.shape[0]
        assert g.shape[1] - n == (M if shapes is None else shapes[b][1])
    with pytest.raises(ValueError, match="outside must"):
        dense_to_augmented(mats, shapes, outside=np.zeros(B + 1))


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


MATS = np.array([[[1.0, -1.0, 3.0], [2.0, 5.0, -1.0]], [[-1.0, -1.0, -1.0], [0.0, 1.0, 2.0]]])


@pytest.mark.parametrize("errors", ["raise", "status"])
def test_outside_is_checked_before_the_ffi(no_ffi, errors):
    def f(**kw):
        return auction_solve_batch(MATS, errors=errors, **kw)
    for bad in (float("nan"), float("inf"), -np.inf, np.float64("nan")):
        with pytest.raises(ValueError, match="outside must be finite"):
            f(outside=bad)
    for bad in (-1.0, -1e-300, np.float64(-3)):
        with pytest.raises(ValueError, match="outside must be >= 0"):
            f(outside=bad)
    for bad in (np.zeros(2, dtype=np.float32), np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="outside must be float64"):
            f(outside=bad)
    for bad in (np.zeros(3), np.zeros((2, 3)), np.zeros((2, 2, 1)), np.zeros((1, 2)), np.zeros(())):
        with pytest.raises(ValueError, match="outside must have shape"):
            f(outside=bad)
    with pytest.raises(TypeError, match="outside on the device needs mats on the device"):
        f(outside=_FakeDeviceTensor())
    for bad in ("1.0", [1.0, 2.0], object(), True):
        with pytest.raises(TypeError, match="outside must be a float"):
            f(outside=bad)
    # the whole-call checks of the status mode come first, in their order
    with pytest.raises(ValueError, match="shapes must be"):
        f(outside=-1.0, shapes=np.zeros((3, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="eps_start is NaN"):
        f(outside=-1.0, eps_start=float("nan"))
    with pytest.raises(ValueError, match="prices must have shape"):
        f(outside=-1.0, prices=np.zeros((2, 4)))
    # what belongs to one problem or one row does not raise: the library is reached
    for ok in (0.0, -0.0, 3, np.float32(1.5), np.array([1.0, np.nan]), np.full((2, 2), np.inf), np.array([-1.0, 2.0])):
        with pytest.raises(_NoFFI):
            f(outside=ok)
    with pytest.raises(_NoFFI):  # cardinality_check is accepted and has no effect
        f(outside=1.0, cardinality_check=False)


class _Recorder:
    """Stands in for the library: records what the front end passes and fills nothing."""
    AT = {"misslap_solve_dense_batch": (5, 8), "misslap_solve_dense_batch_status": (5, 8),
          "misslap_solve_dense_batch_outside": (5, 7)}  # (the fast / eps array argument, the options)

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in self.AT:
            raise AttributeError(name)
        fast_at, opts_at = self.AT[name]

        def call(*args):
            opts = args[opts_at]._obj
            fast = args[fast_at]
            if name == "misslap_solve_dense_batch" and fast is not None:  # per-problem eps: (read now, while it lives)
                fast = np.ctypeslib.as_array(C.cast(fast, C.POINTER(C.c_float)), (2,)).copy().tolist()
            self.calls.append(dict(name=name, fast=fast, eps_start=opts.eps_start, maximize=opts.maximize,
                                   max_iter=opts.max_iter, mat_dtype=opts.mat_dtype, args=args))
            if name.endswith("outside") and args[12] == 0:
                self.calls[-1]["outside"] = np.ctypeslib.as_array(C.cast(args[11], C.POINTER(C.c_double)), (2,)).copy()
            raise _NoFFI()
        return call


def _record(monkeypatch, **kw):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with pytest.raises(_NoFFI):
        auction_solve_batch(MATS, **kw)
    (call,) = rec.calls
    return call


def test_fast_is_resolved_in_the_front_end(monkeypatch):
    half = [0.5, 0.5]  # (float)(1 / n_b) with n_b = 2
    # without outside: today's call and today's options, whether fast is left alone or given
    for kw, fast, eps in ((dict(), 0, 0.0), (dict(fast=False), 0, 0.0), (dict(fast=True), 1, 0.0), (dict(fast=None), 0, 0.0),
                          (dict(eps_start=0.5), 0, 0.5), (dict(fast=True, eps_start=0.25), 1, 0.25),
                          (dict(fast=False, eps_start=0.25), 0, 0.25), (dict(fast=None, eps_start=0.25), 0, 0.25)):
        c = _record(monkeypatch, **kw)  # the default mode: per-problem eps or none
        assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_dense_batch", half if fast else None, eps), kw
        assert c["args"][7] == 1 and c["max_iter"] == 1000000 and c["maximize"] == 0 and c["mat_dtype"] == 0
        c = _record(monkeypatch, errors="status", **kw)
        assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_dense_batch_status", fast, eps), kw
        assert c["args"][7] == 1 and c["max_iter"] == 1000000 and c["maximize"] == 0 and c["mat_dtype"] == 0
    # with outside: a single phase unless eps_start > 0 was given; explicit settings pass through; both modes run it
    for errors in ("raise", "status"):
        for kw, fast, eps in ((dict(), 1, 0.0), (dict(eps_start=0.5), 0, 0.5), (dict(eps_start=1e-3), 0, float(np.float32(1e-3))),
                              (dict(fast=False), 0, 0.0), (dict(fast=True, eps_start=0.5), 1, 0.5), (dict(fast=True), 1, 0.0),
                              (dict(eps_start=0.0), 1, 0.0), (dict(fast=None, eps_start=-1.0), 1, -1.0)):
            c = _record(monkeypatch, outside=1.0, problem="max", errors=errors, cardinality_check=errors == "raise", **kw)
            assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_dense_batch_outside", fast, eps), kw
            assert c["maximize"] == 1
    # the scalar travels as one value per problem (outside_ld = 0), the (B, N) form with outside_ld = N
    c = _record(monkeypatch, outside=2.0)
    assert c["args"][12] == 0 and np.array_equal(c["outside"], [2.0, 2.0])
    assert _record(monkeypatch, outside=np.array([1.0, 2.0]))["args"][12] == 0
    assert _record(monkeypatch, outside=np.ones((2, 2)))["args"][12] == 2
    # outside stays float64 whatever the stack's type is
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with pytest.raises(_NoFFI):
        auction_solve_batch(MATS.astype(np.float16), mat_dtype="float16", outside=np.array([1.0, 2.0]))
    assert rec.calls[0]["mat_dtype"] == _lib.DTYPE_F16 and np.array_equal(rec.calls[0]["outside"], [1.0, 2.0])


# ---- the C entry point and the workspace

def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_dense_batch_outside_workspace_bytes
    cap = _lib.DENSE_BATCH_MAX_DIM
    for B, N, M in ((1, 1, 1), (2, 7, 5), (64, cap, cap), (100000, 256, 40), (2**31 - 1, 1, 1)):
        a, b = f(B, N, M, 0), f(B, N, M, 1)
        assert a > 0 and a % 256 == 0 and b % 256 == 0, (B, N, M)
        assert b >= a + 8 * B * (M + N)  # the staged starting prices of the augmented problems
        assert a == f(B, 1, 1, 0)        # without prices the size of a problem costs nothing
    assert f(1024, 64, 64, 0) >= 1024 * (32 + 8)  # a check record and a sanitised shape per problem
    for bad in ((0, 4, 4), (2**31, 4, 4), (1, 0, 4), (1, cap + 1, 4), (1, 4, 0), (1, 4, cap + 1), (1, -1, 4)):
        assert f(*bad, 1) == -1, bad


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    mat = np.array([[[1.0, -1.0], [2.0, 3.0]]])
    outside = np.array([[4.0, 5.0, 6.0]])
    shapes = np.array([[2, 1]], dtype=np.int32)
    sol, status = np.empty((1, 2), dtype=np.int32), np.empty(1, dtype=np.int32)
    oprices = np.empty((1, 2))
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, N=2, M=2, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0, out=outside.ctypes.data, ld=0,
             shp=None, m=mat.ctypes.data):
        return built_lib.misslap_solve_dense_batch_outside(
            B, N, M, m, shp, 1, None, C.byref(opts), None, work, nwork, out, ld, sol.ctypes.data, None,
            oprices.ctypes.data, on_dev, st, None, C.cast(metas, C.c_void_p), None)

    err = built_lib.misslap_last_error
    cap = _lib.DENSE_BATCH_MAX_DIM
    for ld in (1, -1, -1024):  # outside_ld: 0 or >= N
        assert call(ld=ld) == _lib.ERR_INVALID and b"outside_ld" in err(), ld
    assert call(out=None) == _lib.ERR_INVALID and b"outside" in err()
    assert call(m=None) == _lib.ERR_INVALID and b"mat" in err()
    assert call(N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_DENSE_BATCH_MAX_DIM" in err()
    assert call(M=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_DENSE_BATCH_MAX_DIM" in err()
    assert call(M=0) == _lib.ERR_INVALID and call(B=0) == _lib.ERR_INVALID
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    bad_shape = np.array([[3, 1]], dtype=np.int32)  # host shapes are checked on the host, as in the status call
    assert call(shp=bad_shape.ctypes.data) == _lib.ERR_INVALID and b"problem 0: shape (3, 1)" in err()
    tuned = _lib.Options()
    C.memmove(C.byref(tuned), C.byref(o), C.sizeof(o))
    tuned.tail_threshold = 5
    assert call(opts=tuned) == _lib.ERR_INVALID and b"misslap_solve_dense_batch_outside takes" in err()
    need = built_lib.misslap_dense_batch_outside_workspace_bytes(1, 2, 2, 0)
    dev = _lib.Options()
    C.memmove(C.byref(dev), C.byref(o), C.sizeof(o))
    dev.input_on_device = 1
    assert call(work=4096, nwork=need, on_dev=1) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1, opts=dev) == _lib.ERR_INVALID and b"workspace" in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1, opts=dev) == _lib.ERR_INVALID  # misaligned
    for ld, shp in ((0, None), (2, None), (3, shapes.ctypes.data)):  # valid host arguments: only the GPU can be missing
        rc = call(ld=ld, shp=shp)
        assert rc in (0, _lib.ERR_NO_DEVICE), err()
        if rc:
            assert b"no CPU fallback" in err()


# ---- the definition is optimal under the default the front end chooses

DRAWS = 400


def _draw(rng, t):
    """Dense n x m with n, m < 45, integer values 0 .. 19, half the entries gated to -1, a fully gated row in every 7th
    draw, and integer outside values (per row, or one for the problem)."""
    n, m = (int(x) for x in rng.integers(1, 45, 2))
    mat = rng.integers(0, 20, (n, m)).astype(np.float64)
    mat[rng.random((n, m)) < 0.5] = -1.0
    gated = t % 7 == 0
    if gated:
        mat[int(rng.integers(0, n))] = -1.0
    outside = rng.integers(0, 20, n).astype(np.float64) if rng.random() < 0.5 else float(rng.integers(0, 20))
    return n, m, mat, outside, ("min", "max")[t % 2], gated


def test_single_phase_on_the_augmented_matrix_is_optimal():
    """400 draws (integer values, so eps = 1 / n < the gap between two objectives): the oracle with fast=True on
    dense_to_augmented reports eCE = 1 and its objective is linear_sum_assignment's on the augmented matrix, missing
    entries at +-1e6, within 1e-9.  Every draw counts."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(3)
    seen = dict(min=0, max=0, unmatched=0, matched=0, tall=0, gated=0)
    for t in range(DRAWS):
        n, m, mat, outside, problem, gated = _draw(rng, t)
        o = outside if isinstance(outside, float) else outside[None]
        (aug,) = dense_to_augmented(mat[None], outside=o)
        assert aug.shape == (n, m + n)
        res = orc.auction_solve(mat=aug, problem=problem, fast=True, cardinality_check=False)
        assert res["meta"]["eCE"] == 1, t
        sol = np.asarray(res["sol"])
        assert (sol >= 0).all() and len(set(sol.tolist())) == n, t
        assert (sol[sol >= m] == np.flatnonzero(sol >= m) + m).all(), t  # an outside object is its own row's
        full = np.where(aug >= 0, aug, 1e6 if problem == "min" else -1e6)
        ri, ci = lsa(full, maximize=problem == "max")
        best = float(full[ri, ci].sum())
        assert abs(res["extra"]["obj_f64"] - best) <= 1e-9, (t, problem, res["extra"]["obj_f64"], best)
        seen[problem] += 1
        seen["unmatched"] += int((sol >= m).sum())
        seen["matched"] += int((sol < m).sum())
        seen["tall"] += n > m
        seen["gated"] += gated
    assert seen["min"] == seen["max"] == DRAWS // 2
    assert seen["unmatched"] > 0 and seen["matched"] > 0 and seen["tall"] > 0 and seen["gated"] > 0
