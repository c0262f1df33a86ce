"""The sparse batch's status mode without a GPU: the entry points are declared, bound and exported, the new status
constants agree between the header and the binding and leave codes 0..7 alone, the workspace size is answered on the host,
the whole-call argument errors of auction_solve_sparse_batch(errors="status") raise before the library is reached, and the
mixed batch the GPU test runs on holds a problem of every sparse status code."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_sparse_batch
from tests import _sparse_status_fixture as fxt
from tests._sparse_status_fixture import DIMS, ORDER, expected_status, mixed_batch, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD = ("OK", "TOO_FEW_VALUES", "EMPTY_ROW", "INFINITE_VALUE", "INFEASIBLE", "PRICE_NOT_FINITE", "PRICE_NEGATIVE",
       "BAD_SHAPE")
NEW = ("NO_ENTRIES", "DIVISION_BY_ZERO", "NEGATIVE_INDEX", "ROWS_UNSORTED", "ROW_GAP", "TOO_LARGE", "PRICES_TOO_NARROW")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in ("misslap_solve_sparse_batch_status", "misslap_sparse_batch_workspace_bytes"):
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert f"#define MISSLAP_ABI_VERSION 2\n" in header


def test_status_constants_match_the_header():
    names = OLD + NEW
    prog = ['#include <stdio.h>', '#include "misslap.h"', 'int main(void){']
    prog += [f'printf("{n} %d\\n", MISSLAP_BATCH_STATUS_{n});' for n in names]
    prog += ['int (*f)(int64_t, const int32_t *, const double *, const int64_t *, const int64_t *, const int64_t *, int32_t,',
             '         const double *, int64_t, int32_t, const misslap_options *, void *, void *, int64_t, int64_t, int64_t,',
             '         int32_t *, double *, int32_t, int32_t *, int32_t *, misslap_dense_batch_meta *,',
             '         misslap_dense_batch_info *) = misslap_solve_sparse_batch_status;',
             'int64_t (*g)(int64_t, int64_t, int32_t, int32_t) = misslap_sparse_batch_workspace_bytes;',
             'return (f == 0) + (g == 0);}']
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "t.c"), os.path.join(d, "t.o")
        open(src, "w").write("\n".join(prog))
        # the prototypes: compiled as plain C, not linked
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"),
                               src, "-o", obj])
        # the values: printed by a program that names no library symbol
        open(src, "w").write("\n".join(prog[:3 + len(names)] + ["return 0;}"]))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src,
                               "-o", exe])
        out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert [int(out[n]) for n in OLD] == list(range(8))  # codes 0..7 keep their values
    assert [int(out[n]) for n in NEW] == list(range(8, 15))  # appended, each under its own name
    for n in names:
        assert getattr(_lib, "BATCH_STATUS_" + n) == int(out[n]), n
        if hasattr(fxt, n):
            assert getattr(fxt, n) == int(out[n]), n  # the fixture's own numbering
    assert sorted(ORDER) == sorted(int(out[n]) for n in names if n not in ("OK", "EMPTY_ROW", "BAD_SHAPE"))


def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_sparse_batch_workspace_bytes
    by_b = [f(B, 1000, 0, 1) for B in (1, 2, 63, 64, 65, 1024, 100000)]
    assert by_b[0] > 0 and all(a <= b for a, b in zip(by_b, by_b[1:])) and by_b[0] < by_b[-1]
    by_nnz = [f(64, z, 0, 1) for z in (0, 1, 63, 64, 65, 1000, 10**6, 10**9)]
    assert by_nnz[0] > 0 and all(a <= b for a, b in zip(by_nnz, by_nnz[1:])) and by_nnz[0] < by_nnz[-1]
    assert f(1024, 5000, 0, 0) < f(1024, 5000, 0, 1)  # the cardinalities
    # a check record, a row start per entry and one more per problem, a cardinality
    assert f(1024, 5000, 1, 1) >= 1024 * 32 + 4 * (5000 + 1024) + 4 * 1024
    assert f(1024, 5000, 1, 1) % 256 == 0
    for bad in ((0, 4), (-1, 4), (2**31, 4), (1, -1)):
        assert f(*bad, 0, 1) == -1, bad


class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


def test_whole_call_errors_still_raise_before_ffi(no_ffi):
    loc = np.array([[0, 0], [1, 1], [0, 0]], dtype=np.int32)
    val = np.array([1.0, 2.0, 3.0])
    off = np.array([0, 2, 3])
    st = dict(errors="status")
    with pytest.raises(ValueError, match="errors must be"):
        auction_solve_sparse_batch(loc, val, off, errors="bogus")
    with pytest.raises(ValueError, match="dims"):
        auction_solve_sparse_batch(loc, val, off, dims=(4, 4))  # the default mode takes none
    with pytest.raises(ValueError, match="int32"):
        auction_solve_sparse_batch(loc.astype(np.int64), val, off, **st)
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_sparse_batch(loc, val.astype(np.float32), off, **st)
    with pytest.raises(ValueError, match=r"shape \(nnz, 2\)"):
        auction_solve_sparse_batch(loc.ravel(), val, off, **st)
    with pytest.raises(ValueError, match="entries"):
        auction_solve_sparse_batch(loc, val[:2], off, **st)
    with pytest.raises(ValueError, match="offsets"):
        auction_solve_sparse_batch(loc, val, np.array([0, 2]), **st)
    with pytest.raises(ValueError, match="non-decreasing"):
        auction_solve_sparse_batch(loc, val, np.array([0, 3, 2, 3]), **st)
    with pytest.raises(ValueError, match="sizes"):
        auction_solve_sparse_batch(loc, val, off, sizes=np.ones((3, 2), dtype=int), **st)
    with pytest.raises(ValueError, match="prices must have shape"):
        auction_solve_sparse_batch(loc, val, off, prices=np.zeros((3, 2)), **st)
    with pytest.raises(ValueError, match="prices must have shape"):
        auction_solve_sparse_batch(loc, val, off, prices=np.zeros(2), **st)
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_sparse_batch(loc, val, off, prices=np.zeros((2, 2), dtype=np.float32), **st)
    with pytest.raises(TypeError, match="prices"):
        auction_solve_sparse_batch(loc, val, off, prices=[[0.0, 0.0]] * 2, **st)
    with pytest.raises(ValueError, match="NaN"):
        auction_solve_sparse_batch(loc, val, off, eps_start=float("nan"), **st)
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for dims in ((0, 4), (4, cap + 1), (4,), 4, (4, 4, 4), (2.5, 4), ("a", 4)):
        with pytest.raises(ValueError, match="dims must be"):
            auction_solve_sparse_batch(loc, val, off, dims=dims, **st)
    # what belongs to one problem does not raise: valid arguments reach the library, prices narrower than a problem too
    with pytest.raises(_NoFFI):
        auction_solve_sparse_batch(loc, val, off, dims=(cap, 1), sizes=np.array([[2, 2], [1, 0]]), fast=True,
                                   prices=np.zeros((2, 1)), **st)
    with pytest.raises(_NoFFI):
        auction_solve_sparse_batch([(loc[:2], val[:2]), (loc[2:], val[2:])], **st)
    with pytest.raises(_NoFFI):  # ... and the default mode is still the default
        auction_solve_sparse_batch(loc, val, off)


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    """Argument errors come before any device is touched; valid arguments reach the device (MISSLAP_ERR_NO_DEVICE here)."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    loc = np.array([[0, 0], [1, 1]], dtype=np.int32)
    val = np.array([1.0, 2.0])
    off = np.array([0, 2], dtype=np.int64)
    sol = np.empty((1, 2), dtype=np.int32)
    status = np.empty(1, dtype=np.int32)
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, offsets=off, Nmax=2, Mmax=2, meta=metas, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0,
             off_dev=None, prices=None, p_ld=0):
        return built_lib.misslap_solve_sparse_batch_status(
            B, loc.ctypes.data, val.ctypes.data, offsets.ctypes.data, off_dev, None, 0, prices, p_ld, 1, C.byref(opts), None,
            work, nwork, Nmax, Mmax, sol.ctypes.data, None, on_dev, st, None, C.cast(meta, C.c_void_p), None)

    err = built_lib.misslap_last_error
    cap = _lib.SPARSE_BATCH_MAX_DIM
    assert call(Nmax=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_SPARSE_BATCH_MAX_DIM" in err()
    assert call(Mmax=0) == _lib.ERR_INVALID
    assert call(B=0) == _lib.ERR_INVALID
    assert call(offsets=np.array([1, 2], dtype=np.int64)) == _lib.ERR_INVALID and b"offsets[0]" in err()
    assert call(B=2, offsets=np.array([0, 2, 1], dtype=np.int64)) == _lib.ERR_INVALID and b"non-decreasing" in err()
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    assert call(prices=val.ctypes.data, p_ld=0) == _lib.ERR_INVALID and b"prices_ld" in err()
    blank = (_lib.DenseBatchMeta * 1)()
    assert call(meta=blank) == _lib.ERR_INVALID and b"struct_size" in err()
    o2 = _lib.Options()
    C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
    o2.tiled_min_K = 5
    assert call(opts=o2) == _lib.ERR_INVALID and b"every other option" in err()
    # with a workspace: every array on the device, a device copy of offsets, the workspace large enough and aligned
    o3 = _lib.Options()
    C.memmove(C.byref(o3), C.byref(o), C.sizeof(o))
    o3.input_on_device = 1
    need = built_lib.misslap_sparse_batch_workspace_bytes(1, 2, 0, 1)
    assert call(work=4096, nwork=need, on_dev=1, off_dev=8192) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need, on_dev=1, opts=o3) == _lib.ERR_INVALID and b"device copy of offsets" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1, off_dev=8192, opts=o3) == _lib.ERR_INVALID and b"workspace" in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1, off_dev=8192, opts=o3) == _lib.ERR_INVALID  # misaligned
    rc = call()  # valid host arguments: only the GPU can be missing
    assert rc in (0, _lib.ERR_NO_DEVICE), err()
    if rc:
        assert b"no CPU fallback" in err()
    else:
        assert status[0] == 0 and metas[0].n_rows == 2


def test_mixed_fixture_holds_every_status_code():
    fx = mixed_batch()
    probs, sizes, prices, kinds = fx["probs"], fx["sizes"], fx["prices"], fx["kinds"]
    B = len(probs)
    status, size = expected_status(probs, sizes, prices, fast=True, dims=DIMS)
    assert np.array_equal(status, kinds)  # every planted defect is the FIRST check its problem fails
    assert (kinds[0::2] == 0).all() and (kinds[1::2] != 0).all()
    for code in ORDER:
        assert (status == code).sum() >= 2, code  # plain, and with a later check failing too
    assert (status == 0).sum() * 2 == B
    # the guard's word: every healthy problem is matched completely, an infeasible one is not, and nothing is said of a
    # graph that is not clean or beyond the cap
    ok = status == 0
    n = np.array([int(p[0][:, 0].max()) + 1 if len(p[0]) else 0 for p in probs])
    assert (size[ok] == n[ok]).all() and (size[status == fxt.INFEASIBLE] < n[status == fxt.INFEASIBLE]).all()
    for code in (fxt.NO_ENTRIES, fxt.NEGATIVE_INDEX, fxt.ROWS_UNSORTED, fxt.ROW_GAP):
        assert (size[status == code] == -1).all(), code
    # without the guard an infeasible problem falls through to a later check, or to a solve
    nocheck, nosize = expected_status(probs, sizes, prices, fast=True, cardinality_check=False, dims=DIMS)
    assert not (nocheck == fxt.INFEASIBLE).any() and (nosize == -1).all()
    assert set(nocheck[status == fxt.INFEASIBLE]) == {0, fxt.INFINITE_VALUE}
    assert np.array_equal(nocheck[status != fxt.INFEASIBLE], status[status != fxt.INFEASIBLE])
    # without `fast` N = 0 divides nothing: those problems are healthy, or fail their second defect
    slow = expected_status(probs, sizes, prices, dims=DIMS)[0]
    assert set(slow[status == fxt.DIVISION_BY_ZERO]) == {0, fxt.NEGATIVE_INDEX}
    assert np.array_equal(slow[status != fxt.DIVISION_BY_ZERO], status[status != fxt.DIVISION_BY_ZERO])
    # without dims only the cap is too large: a problem beyond DIMS is then too wide for the prices
    wide = expected_status(probs, sizes, prices, fast=True)[0]
    over = [b for b in range(B) if len(probs[b][0]) and status[b] == fxt.TOO_LARGE and probs[b][0][:, 1].max() < fxt.CAP]
    assert len(over) >= 2 and (wide[over] == fxt.PRICES_TOO_NARROW).all()
    assert all(probs[b][0][:, 1].max() >= DIMS[1] for b in over)  # indices that would leave the carve
    assert np.array_equal(np.delete(wide, over), np.delete(status, over))
    # without sizes the reference's N is the max row: nothing has too few values or divides by zero
    free = expected_status(probs, None, prices, fast=True, dims=DIMS)[0]
    assert not np.isin(free, (fxt.TOO_FEW_VALUES, fxt.DIVISION_BY_ZERO)).any()
    # the padded packing keeps the problems where offsets say, between +inf values at indices beyond every carve
    loc, val, off = pack(probs, pad=64)
    assert np.isinf(val[:64]).all() and np.isinf(val[-64:]).all() and (loc[:64] == fxt.INT_MAX).all()
    assert off[0] == 0 and off[-1] == len(val) - 128
    for b in (0, 1, B - 1):
        assert np.array_equal(loc[64:-64][off[b]:off[b + 1]], probs[b][0])
