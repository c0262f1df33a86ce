"""auction_solve_points_batch (misslap_solve_points_batch) without a GPU: the entry points are declared, bound and
exported; the sizing function; the definition (`points_to_dense` against a plain loop, and against the fused chain it
must not be); the front end's whole-call checks; the C entry point's argument errors; the CPU side of the verdict table
against the dense call's; and the optimality of the definition with `outside` through the oracle.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_points_batch, dense_to_augmented, points_to_dense
from tests._batch_shapes import bits
from tests._points_fixture import (BAD_OUTSIDE, DTYPES, dense_by_loops, draw, expected_status, fused_by_loops,
                                   verdict_batch)
from tests._status_fixture import expected_status as dense_status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_points_batch", "misslap_points_batch_workspace_bytes")
CAP = 2048


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "#define MISSLAP_ABI_VERSION 2\n" in header and built_lib.misslap_abi_version() == 2
    for name in ("auction_solve_points_batch", "points_to_dense"):
        assert name in sslap_amd.__all__ and callable(getattr(sslap_amd, name)), name
    assert sslap_amd.auction_solve_points_batch is auction_solve_points_batch
    assert _lib.POINTS_BATCH_MAX_DIM == CAP and _lib.POINTS_BATCH_MAX_COORDS == 8
    from sslap_amd._batch import _STATUS_ERRORS
    assert "points" in _STATUS_ERRORS


def test_the_header_is_c99():
    prog = ['#include "misslap.h"', 'int main(void){',
            'int (*f)(int64_t, int64_t, int64_t, int64_t, const void *, int64_t, int64_t, int64_t, const void *, int64_t,',
            '         int64_t, int64_t, const int32_t *, int32_t, const double *, const misslap_options *, void *, void *,',
            '         int64_t, const double *, int64_t, int32_t *, double *, double *, int32_t, int32_t *, int32_t *,',
            '         misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_points_batch;',
            'int64_t (*g)(int64_t, int64_t, int64_t, int32_t, int32_t) = misslap_points_batch_workspace_bytes;',
            'return (f == 0) + (g == 0) + (MISSLAP_POINTS_BATCH_MAX_DIM != 2048) + (MISSLAP_POINTS_BATCH_MAX_COORDS != 8);}']
    for std in ("c99", "c11"):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write("\n".join(prog))
            subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Werror", "-pedantic", "-c", "-I",
                                   os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t.o")])


def test_build_sees_every_header_of_the_translation_unit():
    from sslap_amd import build
    unit = open(os.path.join(build.CSRC, "misslap.hip")).read()
    for name in re.findall(r'#include "([a-z_0-9]+\.hpp)"', unit):
        assert name in build.SOURCES, name
    for name in ("kernels_list_finish.hpp", "abi_list_finish.hpp", "kernels_points_batch.hpp", "abi_points_batch.hpp"):
        assert name in build.SOURCES and os.path.exists(os.path.join(build.CSRC, name)), name


# ---- the sizing function

def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_points_batch_workspace_bytes
    for B, N, M in ((1, 1, 1), (2, 7, 5), (64, CAP, CAP), (100000, 256, 40), (2**31 - 1, 1, 1)):
        sizes = {(p, o): f(B, N, M, p, o) for p in (0, 1) for o in (0, 1)}
        assert all(s > 0 and s % 256 == 0 for s in sizes.values()), (B, N, M)
        # the carve: check records and sanitised shapes always; the staged augmented prices with both only
        assert sizes[0, 0] == sizes[1, 0] == sizes[0, 1] == f(B, 1, 1, 0, 0)
        assert sizes[1, 1] >= sizes[0, 0] + 8 * B * (M + N)
        assert sizes[1, 1] < sizes[0, 0] + 8 * B * (M + N) + 256
    assert f(1024, 64, 64, 0, 0) >= 1024 * (16 + 8)  # a check record and a sanitised shape per problem
    for bad in ((0, 4, 4), (2**31, 4, 4), (1, 0, 4), (1, CAP + 1, 4), (1, 4, 0), (1, 4, CAP + 1), (1, -1, 4)):
        assert f(*bad, 1, 1) == -1, bad


# ---- points_to_dense is the definition

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_points_to_dense_is_the_loop_and_not_the_fused_chain(dtype, D):
    rng = np.random.default_rng([11, D])
    B, N, M = 3, 7, 9
    x, y = draw("uniform", (B, N, D), dtype, rng), draw("uniform", (B, M, D), dtype, rng)
    got = points_to_dense(x, y)
    assert got.dtype == np.float64 and got.shape == (B, N, M) and got.flags.c_contiguous
    assert np.array_equal(bits(got), bits(dense_by_loops(x, y)))
    assert not np.signbit(got).any()
    shapes = np.array([[7, 9], [1, 1], [4, 8]])
    with_shapes = points_to_dense(x, y, shapes)
    assert np.array_equal(bits(with_shapes), bits(dense_by_loops(x, y, shapes)))
    assert np.isposinf(with_shapes[1, 1:]).all() and np.isposinf(with_shapes[2, :, 8:]).all()
    # the chain a contracting compiler would make is another function (exact rational arithmetic, one rounding per fma)
    fused = fused_by_loops(x, y)
    differ = int((bits(fused) != bits(got)).sum())
    if D == 1:
        assert differ == 0
    elif dtype == "float64":
        assert differ >= 1, differ
    import torch
    assert np.array_equal(bits(points_to_dense(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(shapes))),
                          bits(with_shapes))


def test_points_to_dense_edge_values():
    x = np.array([[[0.0, -0.0], [1e200, 0.0], [np.nan, 0.0], [np.inf, 1.0]]])
    y = np.array([[[-0.0, 0.0], [-1e200, 0.0], [np.inf, 1.0]]])
    c = points_to_dense(x, y)
    assert np.array_equal(bits(c[0, 0, :1]), bits(np.array([0.0])))  # +0.0, never -0.0
    assert np.isposinf(c[0, 1, 1]) and np.isnan(c[0, 2]).all() and np.isnan(c[0, 3, 2]) and np.isposinf(c[0, 3, 0])
    half = np.zeros((1, 2, 2), dtype=np.float16)
    for bad in ((half.astype(np.float32), y), (half, half), (x[0], y[0]), (x, y[:, :, :1])):
        with pytest.raises(ValueError):
            points_to_dense(*bad)


# ---- the front end: every whole-call error raises before the library is reached

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


class _FakeDeviceTensor:
    """What the front end asks of a device tensor before it reaches the library."""
    is_cuda = True

    def __init__(self, shape, dtype, strides=None, index=0):
        import torch
        self.shape, self.dtype, self.device = tuple(shape), dtype, torch.device("cuda", index)
        self._strides = strides if strides is not None else tuple(int(np.prod(shape[k + 1:])) for k in range(len(shape)))

    def data_ptr(self):
        return 0

    def dim(self):
        return len(self.shape)

    def stride(self):
        return self._strides


X = np.arange(24, dtype=np.float64).reshape(2, 4, 3)
Y = np.arange(30, dtype=np.float64).reshape(2, 5, 3) / 7


@pytest.mark.parametrize("errors", ["raise", "status"])
def test_whole_call_errors_raise_before_the_ffi(no_ffi, errors):
    import torch

    def f(x=X, y=Y, **kw):
        return auction_solve_points_batch(x, y, errors=errors, **kw)
    with pytest.raises(ValueError, match="one dtype"):
        f(y=Y.astype(np.float32))
    for dt in (np.float16, np.int64):
        with pytest.raises(ValueError, match="float64 or float32"):
            f(x=X.astype(dt), y=Y.astype(dt))
    with pytest.raises(ValueError, match="at most 8"):
        f(x=np.zeros((1, 2, 9)), y=np.zeros((1, 2, 9)))
    with pytest.raises(ValueError, match="at most 2048 x 2048"):
        f(x=np.zeros((1, CAP + 1, 1)), y=np.zeros((1, 2, 1)))
    with pytest.raises(ValueError, match="at most 2048 x 2048"):
        f(x=np.zeros((1, 2, 1)), y=np.zeros((1, CAP + 1, 1)))
    with pytest.raises(ValueError, match="B and D must agree"):
        f(y=Y[:1])
    with pytest.raises(ValueError, match="B and D must agree"):
        f(y=Y[:, :, :2])
    with pytest.raises(ValueError, match="3 dimensions"):
        f(x=X[0], y=Y[0])
    with pytest.raises(ValueError, match="empty"):
        f(x=X[:, :0], y=Y)
    with pytest.raises(TypeError, match="both be numpy arrays or both tensors"):
        f(y=_FakeDeviceTensor(Y.shape, torch.float64))
    with pytest.raises(TypeError, match="numpy arrays or tensors"):
        f(x=X.tolist())
    with pytest.raises(TypeError, match="numpy arrays or tensors"):
        f(x=torch.from_numpy(X), y=torch.from_numpy(Y))  # (host tensors are not taken)
    fx, fy = _FakeDeviceTensor(X.shape, torch.float64), _FakeDeviceTensor(Y.shape, torch.float64)
    with pytest.raises(ValueError, match="a stride must be >= 0"):
        f(x=_FakeDeviceTensor(X.shape, torch.float64, (12, -3, 1)), y=fy)
    with pytest.raises(ValueError, match="a stride must be >= 0"):
        f(x=fx, y=_FakeDeviceTensor(Y.shape, torch.float64, (15, 3, -1)))
    with pytest.raises(ValueError, match="x is on cuda:0, y on cuda:1"):
        f(x=fx, y=_FakeDeviceTensor(Y.shape, torch.float64, index=1))
    with pytest.raises(ValueError, match="one dtype"):
        f(x=fx, y=_FakeDeviceTensor(Y.shape, torch.float32))
    with pytest.raises(ValueError, match="float64 or float32"):
        f(x=_FakeDeviceTensor(X.shape, torch.bfloat16), y=_FakeDeviceTensor(Y.shape, torch.bfloat16))
    # the keywords of auction_solve_batch, with its checks
    with pytest.raises(ValueError, match="errors must be"):
        auction_solve_points_batch(X, Y, errors="ignore")
    with pytest.raises(ValueError, match="shapes must be"):
        f(shapes=np.zeros((3, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="outside 1 .. 4 x 1 .. 5"):
        f(shapes=np.array([[4, 5], [5, 5]]))
    with pytest.raises(ValueError, match="eps_start is NaN"):
        f(eps_start=float("nan"))
    with pytest.raises(ValueError, match="prices must have shape"):
        f(prices=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        f(prices=np.zeros((2, 5), dtype=np.float32))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="outside must be finite"):
            f(outside=bad)
    with pytest.raises(ValueError, match="outside must be >= 0"):
        f(outside=-1.0)
    with pytest.raises(ValueError, match="outside must have shape"):
        f(outside=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="outside must be float64"):
        f(outside=np.zeros(2, dtype=np.float32))
    with pytest.raises(TypeError, match="outside on the device needs x / y on the device"):
        f(outside=_FakeDeviceTensor((2,), torch.float64))
    with pytest.raises(TypeError, match="prices on the device need x / y on the device"):
        f(prices=_FakeDeviceTensor((2, 5), torch.float64))
    with pytest.raises(TypeError, match="shapes on the device need x / y on the device"):
        f(shapes=_FakeDeviceTensor((2, 2), torch.int32))
    for unknown in ("finish", "cardinality_check", "mat_dtype", "entries"):
        with pytest.raises(TypeError, match=unknown):
            f(**{unknown: None})
    # what belongs to one problem does not raise: the library is reached
    for ok in (dict(), dict(outside=-0.0), dict(outside=np.array([1.0, np.nan])), dict(outside=np.full((2, 4), np.inf)),
               dict(prices=np.full((2, 5), np.nan)), dict(x=X.astype(np.float32), y=Y.astype(np.float32)),
               dict(x=np.full_like(X, np.nan)), dict(shapes=np.array([[4, 2], [1, 5]]))):
        with pytest.raises(_NoFFI):
            f(**ok)


class _Recorder:
    """Stands in for the library: records what the front end passes and fills nothing."""
    def __init__(self):
        self.calls = []

    def misslap_solve_points_batch(self, *args):
        opts = args[15]._obj
        self.calls.append(dict(args=args, fast=args[13], eps_start=opts.eps_start, maximize=opts.maximize,
                               max_iter=opts.max_iter, mat_dtype=opts.mat_dtype))
        raise _NoFFI()


def _record(monkeypatch, x=X, y=Y, **kw):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with pytest.raises(_NoFFI):
        auction_solve_points_batch(x, y, **kw)
    (call,) = rec.calls
    return call


def test_the_call_as_the_library_gets_it(monkeypatch):
    assert len(_lib.SYMBOLS["misslap_solve_points_batch"][1]) == 29
    c = _record(monkeypatch)
    assert len(c["args"]) == 29
    assert c["args"][:4] == (2, 4, 5, 3) and c["args"][5:8] == (12, 3, 1) and c["args"][9:12] == (15, 3, 1)
    assert (c["fast"], c["eps_start"], c["maximize"], c["max_iter"], c["mat_dtype"]) == (0, 0.0, 0, 1000000, _lib.DTYPE_F64)
    assert c["args"][12] is None and c["args"][14] is None and c["args"][19] is None and c["args"][20] == 0
    assert c["args"][23] is None and c["args"][24] == 0  # no outside: no outside_prices; host outputs
    c = _record(monkeypatch, x=X.astype(np.float32), y=Y.astype(np.float32), problem="max", max_iter=7)
    assert (c["maximize"], c["max_iter"], c["mat_dtype"]) == (1, 7, _lib.DTYPE_F32)
    # fast=None: False without outside, True with it unless eps_start > 0; explicit settings pass through
    for kw, fast, eps in ((dict(), 0, 0.0), (dict(fast=True), 1, 0.0), (dict(eps_start=0.5), 0, 0.5),
                          (dict(outside=1.0), 1, 0.0), (dict(outside=1.0, eps_start=0.5), 0, 0.5),
                          (dict(outside=1.0, fast=False), 0, 0.0), (dict(outside=1.0, fast=True, eps_start=0.25), 1, 0.25),
                          (dict(outside=1.0, eps_start=-1.0), 1, -1.0)):
        for errors in ("raise", "status"):
            c = _record(monkeypatch, errors=errors, **kw)
            assert (c["fast"], c["eps_start"]) == (fast, eps), kw
    # the three forms of outside: one value per problem (outside_ld 0) or per row (outside_ld N)
    c = _record(monkeypatch, outside=2.0)
    assert c["args"][20] == 0 and c["args"][23] is not None
    assert np.array_equal(np.ctypeslib.as_array(C.cast(c["args"][19], C.POINTER(C.c_double)), (2,)), [2.0, 2.0])
    assert _record(monkeypatch, outside=np.array([1.0, 2.0]))["args"][20] == 0
    assert _record(monkeypatch, outside=np.ones((2, 4)))["args"][20] == 4


# ---- the C entry point

def test_c_entry_point_validates_then_needs_a_device(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    x, y = np.zeros((1, 2, 3)), np.ones((1, 2, 3))
    outside = np.array([[4.0, 5.0]])
    sol, status = np.empty((1, 2), dtype=np.int32), np.empty(1, dtype=np.int32)
    prices, oprices = np.empty((1, 2)), np.empty((1, 2))
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, N=2, M=2, D=3, xp=x.ctypes.data, xs=(6, 3, 1), yp=y.ctypes.data, ys=(6, 3, 1), shp=None, opts=o,
             work=None, nwork=0, out=None, ld=0, st=status.ctypes.data, on_dev=0, sp=sol.ctypes.data):
        return built_lib.misslap_solve_points_batch(
            B, N, M, D, xp, *xs, yp, *ys, shp, 0, None, C.byref(opts), None, work, nwork, out, ld, sp, prices.ctypes.data,
            oprices.ctypes.data, on_dev, st, None, C.cast(metas, C.c_void_p), None)

    err = built_lib.misslap_last_error
    assert call(N=CAP + 1) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_DIM" in err()
    assert call(M=CAP + 1) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_DIM" in err()
    assert call(M=0) == _lib.ERR_INVALID and call(B=0) == _lib.ERR_INVALID and call(N=-1) == _lib.ERR_INVALID
    for D in (0, 9, -1):
        assert call(D=D) == _lib.ERR_INVALID and b"MISSLAP_POINTS_BATCH_MAX_COORDS" in err(), D
    assert call(xp=None) == _lib.ERR_INVALID and b"null x" in err()
    assert call(yp=None) == _lib.ERR_INVALID and call(sp=None) == _lib.ERR_INVALID and call(st=None) == _lib.ERR_INVALID
    for ld in (1, -1):
        assert call(out=outside.ctypes.data, ld=ld) == _lib.ERR_INVALID and b"outside_ld" in err(), ld
    assert call(xs=(6, -3, 1)) == _lib.ERR_INVALID and b"a stride must be >= 0" in err()
    assert call(ys=(6, 3, -1)) == _lib.ERR_INVALID and b"a stride must be >= 0" in err()
    assert call(xs=(2**62, 3, 1), B=2) == _lib.ERR_INVALID and b"62 bits" in err()
    assert call(ys=(6, 2**62, 1)) == _lib.ERR_INVALID and b"62 bits" in err()
    assert call(xs=(6, 1, 2)) == _lib.ERR_INVALID and b"a strided point set is a device array" in err()
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16, _lib.DTYPE_F64 | _lib.DENSE_ENTRIES_FINITE, 77):
        o2 = _lib.Options()
        o2.struct_size = C.sizeof(_lib.Options)
        o2.mat_dtype = dt
        assert call(opts=o2) == _lib.ERR_INVALID and b"mat_dtype" in err(), dt
    o3 = _lib.Options()
    o3.struct_size = C.sizeof(_lib.Options)
    o3.tail_threshold = 5
    assert call(opts=o3) == _lib.ERR_INVALID and b"every other option must be 0" in err()
    # with a workspace every array is on the device; a workspace too small or misaligned is refused
    work = np.empty(4096, dtype=np.uint8)
    assert call(work=work.ctypes.data, nwork=4096) == _lib.ERR_INVALID and b"with a workspace" in err()
    od = _lib.Options()
    od.struct_size = C.sizeof(_lib.Options)
    od.input_on_device = 1
    need = built_lib.misslap_points_batch_workspace_bytes(1, 2, 2, 0, 0)
    base = (work.ctypes.data + 255) & ~255
    assert call(opts=od, work=base, nwork=need - 1, on_dev=1) == _lib.ERR_INVALID and b"misslap_points_batch_workspace_bytes" in err()
    assert call(opts=od, work=base + 8, nwork=4096, on_dev=1) == _lib.ERR_INVALID and b"256-byte aligned" in err()
    # host shapes are checked before a device is touched
    bad = np.array([[3, 2]], dtype=np.int32)
    assert call(shp=bad.ctypes.data) == _lib.ERR_INVALID and b"shape (3, 2) outside" in err()
    # valid host arguments: only the GPU can be missing
    for kw in (dict(), dict(out=outside.ctypes.data, ld=0), dict(out=outside.ctypes.data, ld=2)):
        rc = call(**kw)
        assert rc in (0, _lib.ERR_NO_DEVICE), err()
        if rc:
            assert b"no CPU fallback" in err()


# ---- the verdict table on the CPU

@pytest.mark.parametrize("dtype", DTYPES)
def test_expected_status_agrees_with_the_dense_call_where_it_can_express_the_problem(built_lib, dtype):
    """Without outside and without a NaN cost (which the dense stack reads as "no edge"), points_to_dense's stack has the
    dense call's verdicts: +inf is INFINITE_VALUE there too, and its matcher finds min(n, m) on a complete graph."""
    v = verdict_batch(dtype)
    x, y, shapes, prices = v["x"], v["y"], v["shapes"], v["prices"]
    status, size = expected_status(x, y, shapes, prices)
    cost = points_to_dense(x, y, shapes)
    want, wsize = dense_status(np.where(np.isnan(cost), np.inf, cost), shapes, prices)  # NaN -> +inf: expressible
    assert np.array_equal(status, want), (status, want)
    assert np.array_equal(size, wsize), (size, wsize)
    by_kind = dict(zip(v["kinds"], status))
    assert [by_kind[k] for k in ("nan_coord", "inf_coord", "overflow", "n_gt_m", "shape_0_5", "shape_N1_1", "price_nan",
                                 "price_neg", "nan_and_n_gt_m", "inf_outside")] == [3, 3, 3, 4, 7, 7, 5, 6, 3, 0]
    assert all(s == 0 for k, s in zip(v["kinds"], status) if k == "ok")
    # with outside: BAD_OUTSIDE first, +inf outside is INFINITE_VALUE, n > m is solved, the matcher has nothing to say
    status, size = expected_status(x, y, shapes, prices, v["outside"])
    by_kind = dict(zip(v["kinds"], status))
    assert by_kind["bad_outside"] == BAD_OUTSIDE and by_kind["inf_outside"] == 3 and by_kind["n_gt_m"] == 0
    assert by_kind["nan_and_n_gt_m"] == 3 and (size == -1).all()
    assert all(s == 0 for k, s in zip(v["kinds"], status) if k == "ok")


# ---- the definition is worth solving: with outside, a single phase reaches the optimum

def test_fast_on_the_augmented_definition_reaches_scipys_optimum():
    linear_sum_assignment = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(17)
    for t in range(100):
        n, m, D = int(rng.integers(1, 9)), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        x = rng.integers(0, 12, (1, n, D)).astype(np.float64)
        y = rng.integers(0, 12, (1, m, D)).astype(np.float64)
        outside = float(rng.integers(0, 40))
        (aug,) = dense_to_augmented(points_to_dense(x, y), outside=outside)
        res = orc.auction_solve(mat=aug, problem="min", fast=True, cardinality_check=False)
        assert res["meta"]["eCE"] == 1, t
        sol = np.asarray(res["sol"])
        got = float(aug[np.arange(n), sol].sum())
        full = np.where(aug >= 0, aug, 1e9)
        r, c = linear_sum_assignment(full)
        assert got == float(full[r, c].sum()), (t, got, float(full[r, c].sum()))  # (integers: n * eps < 1 is exact)
