"""The ELL batch (auction_solve_ell_batch, misslap_solve_ell_batch) without a GPU: the two entry points are declared, listed
as additions, bound and exported, the prototypes are plain C99, the workspace size is answered on the host,
ell_to_packed is the double loop of the definition, the whole-call argument errors raise before the library is reached,
and the mixed batch the GPU test runs on holds a problem of every status code of the call."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_ell_batch, ell_to_packed
from tests import _ell_fixture as fxt
from tests._batch_shapes import META_KEYS, bits, sparse_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_ell_batch", "misslap_ell_batch_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    import sslap_amd
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "#define MISSLAP_ABI_VERSION 2\n" in header and built_lib.misslap_abi_version() == 2
    for name in ("auction_solve_ell_batch", "ell_to_packed"):
        assert name in sslap_amd.__all__ and callable(getattr(sslap_amd, name)), name


def test_prototypes_compile_as_c99():
    prog = ['#include "misslap.h"', 'int main(void){',
            'int (*f)(int64_t, int64_t, int64_t, const void *, int32_t, const void *, const int32_t *, int32_t,',
            '         const double *, int64_t, int32_t, const misslap_options *, void *, void *, int64_t, int64_t,',
            '         int32_t *, double *, int32_t, int32_t *, int32_t *, misslap_dense_batch_meta *,',
            '         misslap_dense_batch_info *) = misslap_solve_ell_batch;',
            'int64_t (*g)(int64_t, int64_t, int64_t, int32_t, int32_t) = misslap_ell_batch_workspace_bytes;',
            'return (f == 0) + (g == 0) + (MISSLAP_ABI_VERSION != 2);}']
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "t.c"), os.path.join(d, "t.o")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"),
                               src, "-o", obj])


def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_ell_batch_workspace_bytes
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for B, N, K in ((1, 1, 1), (2, 7, 3), (64, cap, 16), (100000, 256, 129), (1, cap, (2**31 - 129) // cap), (2**31 - 1, 1, 1)):
        for guard in (0, 1):
            got = f(B, N, K, 0, guard)
            assert got > 0 and got % 256 == 0, (B, N, K, guard, got)
        assert f(B, N, K, 0, 0) < f(B, N, K, 0, 1)  # the cardinalities
        assert f(B, N, K, 1, 1) == f(B, N, K, 0, 1)
    assert f(1024, 64, 8, 0, 1) >= 1024 * 32 + 4 * 1024  # a check record and a cardinality per problem
    by_b = [f(B, 64, 8, 0, 1) for B in (1, 2, 63, 64, 65, 1024, 100000)]
    assert all(a <= b for a, b in zip(by_b, by_b[1:])) and by_b[0] < by_b[-1]
    for bad in ((0, 4, 4), (-1, 4, 4), (2**31, 4, 4), (1, 0, 4), (1, -3, 4), (1, cap + 1, 4), (1, 4, 0), (1, 4, -1),
                (1, cap, (2**31 - 129) // cap + 1), (1, 2, 2**30), (1, 1, 2**31 - 127), (1, 3, 2**62)):
        assert f(*bad, 0, 1) == -1, bad
    assert f(1, 1, 2**31 - 129, 0, 1) > 0  # N * K exactly at the cap


# ---- ell_to_packed is the definition

def _cases():
    rng = np.random.default_rng(5)
    B, N, K = 5, 6, 7
    cols = rng.integers(0, 9, (B, N, K)).astype(np.int64)
    vals = rng.uniform(0, 10, (B, N, K))
    cols[0, :, :2] = -1                      # holes in front
    cols[1, :, 2:5] = (-1, -7, -(2**40))     # ... in the middle
    cols[2, :, 5:] = -2                      # ... at the end
    cols[3][rng.random((N, K)) < 0.5] = -1   # ... anywhere (a row may lose every entry)
    cols[4, 2] = -1                          # an empty row
    vals[cols < 0] = np.nan
    return cols, vals, np.array([6, 3, 1, 6, 4], dtype=np.int32)


@pytest.mark.parametrize("itype", [np.int32, np.int64])
@pytest.mark.parametrize("vtype", [np.float64, np.float32])
@pytest.mark.parametrize("with_rows", [False, True])
def test_ell_to_packed_is_the_double_loop(itype, vtype, with_rows):
    cols, vals, rows = _cases()
    cols = np.maximum(cols, -(2**31)).astype(itype)
    vals = vals.astype(vtype)
    assert (cols[:4] < 0).any(axis=2).all() and not (cols[4, 2] >= 0).any()
    r = rows if with_rows else None
    got, want = ell_to_packed(cols, vals, r), fxt.packed_by_loops(cols, vals, r)
    assert len(got) == len(want) == cols.shape[0]
    for (gl, gv), (wl, wv) in zip(got, want):
        assert gl.dtype == np.int32 and gv.dtype == np.float64 and gl.shape == wl.shape and gl.flags.c_contiguous
        assert np.array_equal(gl, wl) and np.array_equal(bits(gv), bits(wv))
    if vtype is np.float32:  # widened, not rounded again: every value is the float32 value exactly
        assert all(np.array_equal(gv, gv.astype(np.float32).astype(np.float64)) for _, gv in got)
    if with_rows:  # rows beyond rows[b] contribute nothing
        assert [int(gl[:, 0].max()) + 1 for gl, _ in got[:3]] == [6, 3, 1]
    with pytest.raises(ValueError, match="one shape"):
        ell_to_packed(cols, vals[:, :, :3])


def test_oracle_on_the_packed_form_equals_the_oracle_on_a_hand_packed_copy():
    rng = np.random.default_rng(6)
    n, m, k, K = 12, 15, 4, 9
    loc, val = sparse_problem(rng, n, m, k, "ints")
    cols, vals = fxt.widen(loc, val, n, K, rng, N=n + 3)
    cols[n:] = 3  # rows beyond rows[b] hold entries that must not be seen
    with np.errstate(over="ignore"):  # (a hole's 1e300 has no float32: it is never interpreted)
        v32 = vals[None].astype(np.float32)
    (pl, pv), = ell_to_packed(cols[None].astype(np.int64), v32, rows=[n])
    assert np.array_equal(pl, loc) and np.array_equal(bits(pv), bits(val))  # (0 .. 4 are exact in float32)
    size = (int(loc[:, 1].max()) + 1, n)
    for problem in ("min", "max"):
        a = orc.auction_solve(loc=pl, val=pv.copy(), size=size, problem=problem, fast=True)
        b = orc.auction_solve(loc=loc, val=val.copy(), size=size, problem=problem, fast=True)
        assert np.array_equal(a["sol"], b["sol"]) and a["extra"]["obj_f64"] == b["extra"]["obj_f64"]
        assert all(a["meta"][k] == b["meta"][k] for k in META_KEYS)
        assert a["meta"]["soln_found"] in (0, 1) and (a["sol"] >= 0).all()


# ---- whole-call errors raise before the library is reached

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


class _FakeDeviceTensor:
    """Looks like a tensor on the device to the front-end's first check, which is all a mixed call gets to."""
    is_cuda = True

    def data_ptr(self):
        return 0


def test_whole_call_errors_raise_before_ffi(no_ffi):
    cols = np.array([[[0, 1, -1], [1, -1, 0]], [[2, 0, 1], [-1, -1, 1]]], dtype=np.int32)
    vals = np.arange(12, dtype=np.float64).reshape(2, 2, 3)
    f = auction_solve_ell_batch
    with pytest.raises(ValueError, match="errors must be"):
        f(cols, vals, errors="bogus")
    with pytest.raises(ValueError, match="cols must be int32 or int64"):
        f(cols.astype(np.int16), vals)
    with pytest.raises(ValueError, match="cols must be int32 or int64"):
        f(cols.astype(np.float64), vals)
    with pytest.raises(ValueError, match="vals must be float64 or float32"):
        f(cols, vals.astype(np.float16))
    with pytest.raises(ValueError, match="vals must be float64 or float32"):
        f(cols, cols)
    with pytest.raises(ValueError, match="3 dimensions"):
        f(cols[0], vals[0])
    with pytest.raises(ValueError, match="3 dimensions"):
        f(cols[None], vals[None])
    with pytest.raises(ValueError, match="vals"):
        f(cols, vals[:, :, :2])
    with pytest.raises(ValueError, match="vals"):
        f(cols, vals[:1])
    with pytest.raises(ValueError, match="empty stack"):
        f(cols[:, :0], vals[:, :0])
    with pytest.raises(TypeError, match="both"):
        f(cols, _FakeDeviceTensor())
    with pytest.raises(TypeError, match="both"):
        f(_FakeDeviceTensor(), vals)
    with pytest.raises(TypeError, match="both"):
        f(cols.tolist(), vals)
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for n_cols in (0, -1, cap + 1, 2.5, "a", (3,)):
        with pytest.raises(ValueError, match="n_cols must be"):
            f(cols, vals, n_cols=n_cols)
    with pytest.raises(ValueError, match="MISSLAP_SPARSE_BATCH_MAX_DIM"):
        f(np.zeros((1, cap + 1, 1), dtype=np.int32), np.zeros((1, cap + 1, 1)))
    for rows in (np.array([2]), np.array([[2, 2]]), np.array([2, 2, 2]), np.array([1.0, 2.0]), 2):
        with pytest.raises(ValueError, match="rows must be"):
            f(cols, vals, rows=rows)
    with pytest.raises(TypeError, match="rows on the device"):
        f(cols, vals, rows=_FakeDeviceTensor())
    with pytest.raises(ValueError, match="NaN"):
        f(cols, vals, eps_start=float("nan"))
    with pytest.raises(ValueError, match="prices must have shape"):
        f(cols, vals, prices=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="prices must have shape"):
        f(cols, vals, prices=np.zeros(2))
    with pytest.raises(ValueError, match="dtype"):
        f(cols, vals, prices=np.zeros((2, 4), dtype=np.float32))
    with pytest.raises(TypeError, match="prices"):
        f(cols, vals, prices=[[0.0] * 3] * 2)
    # what belongs to one problem does not raise: the library is reached, in either mode
    for errors in ("raise", "status"):
        with pytest.raises(_NoFFI):
            f(cols, vals, rows=np.array([0, 9]), n_cols=1, prices=np.zeros((2, 1)), fast=True, errors=errors)
        with pytest.raises(_NoFFI):
            f(cols.astype(np.int64), vals.astype(np.float32), errors=errors)
    with pytest.raises(_NoFFI):
        f(cols, vals)


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    """Argument errors come before any device is touched; valid arguments reach the device (MISSLAP_ERR_NO_DEVICE here)."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    cols = np.array([[[0, -1], [1, 0]]], dtype=np.int32)
    vals = np.array([[[1.0, 9.0], [2.0, 3.0]]])
    sol = np.empty((1, 2), dtype=np.int32)
    status = np.empty(1, dtype=np.int32)
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, N=2, K=2, Mmax=2, meta=metas, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0, prices=None,
             p_ld=0, c=cols.ctypes.data):
        return built_lib.misslap_solve_ell_batch(B, N, K, c, 0, vals.ctypes.data, None, 0, prices, p_ld, 1, C.byref(opts),
                                                 None, work, nwork, Mmax, sol.ctypes.data, None, on_dev, st, None,
                                                 C.cast(meta, C.c_void_p), None)

    err = built_lib.misslap_last_error
    cap = _lib.SPARSE_BATCH_MAX_DIM
    assert call(N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_SPARSE_BATCH_MAX_DIM" in err()
    assert call(Mmax=cap + 1) == _lib.ERR_INVALID and b"Mmax" in err()
    assert call(Mmax=0) == _lib.ERR_INVALID
    assert call(B=0) == _lib.ERR_INVALID
    assert call(K=0) == _lib.ERR_INVALID and b"K must be" in err()
    assert call(K=2**30) == _lib.ERR_INVALID and b"N * K" in err()
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    assert call(c=None) == _lib.ERR_INVALID and b"cols" in err()
    assert call(prices=vals.ctypes.data, p_ld=0) == _lib.ERR_INVALID and b"prices_ld" in err()
    blank = (_lib.DenseBatchMeta * 1)()
    assert call(meta=blank) == _lib.ERR_INVALID and b"struct_size" in err()

    def with_(**fields):
        o2 = _lib.Options()
        C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
        for k, v in fields.items():
            setattr(o2, k, v)
        return o2
    assert call(opts=with_(tiled_min_K=5)) == _lib.ERR_INVALID and b"every other option" in err()
    for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        assert call(opts=with_(mat_dtype=dt)) == _lib.ERR_INVALID and b"MISSLAP_DTYPE_F32" in err()
    # with a workspace: every array on the device, the workspace large enough and aligned
    need = built_lib.misslap_ell_batch_workspace_bytes(1, 2, 2, 0, 1)
    dev = with_(input_on_device=1)
    assert call(work=4096, nwork=need, on_dev=1) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need, on_dev=0, opts=dev) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1, opts=dev) == _lib.ERR_INVALID and b"workspace" in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1, opts=dev) == _lib.ERR_INVALID  # misaligned
    for opts in (o, with_(mat_dtype=_lib.DTYPE_F32)):  # (F32 reads the same bytes as 4 floats per row: still finite)
        rc = call(opts=opts)  # valid host arguments: only the GPU can be missing
        assert rc in (0, _lib.ERR_NO_DEVICE), err()
        if rc:
            assert b"no CPU fallback" in err()


# ---- the mixed batch of the GPU verdict test

def test_mixed_fixture_holds_every_status_code():
    fx = fxt.mixed_batch()
    cols, vals, rows, prices, kinds = fx["cols"], fx["vals"], fx["rows"], fx["prices"], fx["kinds"]
    B, N, K = cols.shape
    assert (N, K, prices.shape[1]) == (fxt.MIXED_N, fxt.MIXED_K, fxt.MIXED_P)
    status, size, counts = fxt.expected_status(cols, vals, rows, fxt.MIXED_COLS, prices)
    assert np.array_equal(status, kinds)  # every planted defect is the FIRST check its problem fails
    assert (kinds[0::2] == 0).all() and (kinds[1::2] != 0).all()  # condemned problems between healthy ones
    assert set(status) == set(fxt.ORDER) | {0} and len(fxt.ORDER) == 8
    for code in fxt.ORDER:
        assert (status == code).sum() >= 2, code
    # the codes are the header's
    for name in ("OK", "EMPTY_ROW", "INFINITE_VALUE", "INFEASIBLE", "PRICE_NOT_FINITE", "PRICE_NEGATIVE", "BAD_SHAPE",
                 "TOO_LARGE", "PRICES_TOO_NARROW"):
        assert getattr(fxt, name) == getattr(_lib, "BATCH_STATUS_" + name), name
    # the healthy problems have status 0 for the oracle too: it solves each of them completely
    packed = ell_to_packed(cols, vals, rows.clip(0, N))
    for b in np.flatnonzero(status == 0):
        loc, val = packed[b]
        n, m, nnz = counts[b]
        assert (n, m, nnz) == (rows[b], loc[:, 1].max() + 1, len(val)) and size[b] == n
        got = orc.auction_solve(loc=loc, val=val.copy(), size=(int(m), int(n)), cardinality_check=False)
        assert (got["sol"] >= 0).all() and len(set(got["sol"])) == n, b
    # the guard's word: an infeasible problem is matched short, nothing is said where the guard does not run
    bad = status == fxt.INFEASIBLE
    assert (size[bad] >= 0).all() and (size[bad] < rows[bad]).all()
    for code in (fxt.BAD_SHAPE, fxt.EMPTY_ROW, fxt.TOO_LARGE):
        assert (size[status == code] == -1).all(), code
    assert (counts[status == fxt.BAD_SHAPE] == 0).all()
    # a later defect shows once the first check is out of the way
    nocheck, nosize, _ = fxt.expected_status(cols, vals, rows, fxt.MIXED_COLS, prices, cardinality_check=False)
    assert (nosize == -1).all() and set(nocheck[bad]) == {0, fxt.PRICE_NOT_FINITE}
    assert np.array_equal(nocheck[~bad], status[~bad])
    wide = fxt.expected_status(cols, vals, rows, fxt.CAP, prices)[0]
    over = np.flatnonzero(wide != status)
    assert len(over) >= 2 and (status[over] == fxt.TOO_LARGE).all() and set(wide[over]) == {fxt.PRICES_TOO_NARROW}
    noprice = fxt.expected_status(cols, vals, rows, fxt.MIXED_COLS, None)[0]
    assert set(noprice[np.isin(status, (fxt.PRICES_TOO_NARROW, fxt.PRICE_NOT_FINITE, fxt.PRICE_NEGATIVE))]) == {0}
    # holes hold NaN, infinities and columns of any negative value; rows beyond rows[b] hold +inf at column INT_MAX; a
    # healthy problem's prices beyond its own columns are NaN or negative
    ok = np.flatnonzero(status == 0)
    holes = cols[ok] < 0
    assert np.isnan(vals[ok][holes]).any() and np.isinf(vals[ok][holes]).any() and len(np.unique(cols[ok][holes])) >= 3
    b = int(ok[np.argmin(rows[ok])])
    assert rows[b] < N and (cols[b, rows[b]:] == fxt.INT_MAX).all() and np.isinf(vals[b, rows[b]:]).all()
    assert all(not np.isfinite(prices[b, counts[b, 1]:]).all() or np.signbit(prices[b, counts[b, 1]:]).any() for b in ok)
    assert int(cols.max()) == 2**31 + 5
