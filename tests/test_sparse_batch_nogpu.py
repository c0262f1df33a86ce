"""Sparse batch without a GPU: the entry point is declared, bound and exported, the header still compiles as plain C,
auction_solve_sparse_batch validates its arguments before any call into the library, and the C entry point rejects bad
arguments before it touches a device."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, auction_solve_sparse_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    assert "misslap_solve_sparse_batch" in set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    assert "misslap_solve_sparse_batch" in _lib.SYMBOLS
    assert getattr(built_lib, "misslap_solve_sparse_batch") is not None
    assert re.search(r"#define MISSLAP_ABI_VERSION 2\b", header)
    cap = int(re.search(r"#define MISSLAP_SPARSE_BATCH_MAX_DIM (\d+)", header).group(1))
    assert cap == _lib.SPARSE_BATCH_MAX_DIM == 2048
    assert "auction_solve_sparse_batch" in sslap_amd.__all__


def test_header_compiles_as_plain_c():
    prog = ['#include "misslap.h"', 'int main(void){',
            'misslap_dense_batch_meta m = {0}; m.struct_size = (int32_t)sizeof m;',
            'int (*f)(int64_t, const int32_t *, const double *, const int64_t *, const int64_t *, const float *,',
            '         const double *, int64_t, int32_t, const misslap_options *, int32_t *, int64_t, double *, int64_t,',
            '         int32_t, misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_sparse_batch;',
            'return (f == 0) + (MISSLAP_SPARSE_BATCH_MAX_DIM != 2048);}']
    for std in ("c99", "c11"):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write("\n".join(prog))
            subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Werror", "-pedantic", "-c", "-I",
                                   os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t.o")])


class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


def _ok():
    loc = np.array([[0, 0], [0, 1], [1, 1], [0, 0], [1, 0], [1, 1]], dtype=np.int32)
    val = np.arange(6, dtype=np.float64)
    return loc, val, np.array([0, 3, 6])


def test_arguments_are_validated_before_ffi(no_ffi):
    loc, val, off = _ok()
    with pytest.raises(ValueError, match="int32"):
        auction_solve_sparse_batch(loc.astype(np.int64), val, off)
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_sparse_batch(loc, val.astype(np.float32), off)
    with pytest.raises(ValueError, match="shape"):
        auction_solve_sparse_batch(loc.reshape(-1), val, off)
    with pytest.raises(ValueError, match="entries"):
        auction_solve_sparse_batch(loc, val[:5], off)
    with pytest.raises(TypeError):
        auction_solve_sparse_batch(loc.tolist(), val, off)
    with pytest.raises(ValueError, match="offsets is required"):
        auction_solve_sparse_batch(loc, val)
    with pytest.raises(ValueError, match="offsets"):
        auction_solve_sparse_batch(loc, val, np.array([0, 3, 5]))  # does not end at nnz
    with pytest.raises(ValueError, match="offsets"):
        auction_solve_sparse_batch(loc, val, np.array([1, 3, 6]))  # does not start at 0
    with pytest.raises(ValueError, match="non-decreasing"):
        auction_solve_sparse_batch(loc, val, np.array([0, 4, 3, 6]))
    with pytest.raises(ValueError, match="offsets"):
        auction_solve_sparse_batch(loc, val, np.array([0.0, 3.0, 6.0]))
    with pytest.raises(ValueError, match="offsets"):
        auction_solve_sparse_batch(loc, val, np.array([6]))
    with pytest.raises(ValueError, match="sizes"):
        auction_solve_sparse_batch(loc, val, off, sizes=np.ones((3, 2), dtype=int))
    with pytest.raises(ValueError, match="sizes"):
        auction_solve_sparse_batch(loc, val, off, sizes=np.ones((2, 2)))  # not integers
    with pytest.raises(ValueError, match="prices"):
        auction_solve_sparse_batch(loc, val, off, prices=np.zeros((2, 1)))  # fewer columns than the problems have
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_sparse_batch(loc, val, off, prices=np.zeros((2, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        auction_solve_sparse_batch(loc, val, off, prices=[[0.0] * 2] * 2)
    with pytest.raises(ValueError, match="NaN"):
        auction_solve_sparse_batch(loc, val, off, eps_start=float("nan"))
    with pytest.raises(ZeroDivisionError, match="problem 0"):  # from_sparse's N of a one-row problem is 0
        auction_solve_sparse_batch(np.array([[0, 0], [1, 1]], dtype=np.int32), np.ones(2), [0, 1, 2], fast=True)
    with pytest.raises(TypeError, match="no val / offsets"):
        auction_solve_sparse_batch([(loc[:3], val[:3])], val)
    with pytest.raises(ValueError, match="problem 1"):
        auction_solve_sparse_batch([(loc[:3], val[:3]), (loc[3:], val[3:].astype(np.float32))])
    with pytest.raises(_NoFFI):  # valid arguments do reach the library
        auction_solve_sparse_batch(loc, val, off, sizes=np.array([[2, 1], [2, 1]]), prices=np.zeros((2, 3)), fast=True)
    with pytest.raises(_NoFFI):
        auction_solve_sparse_batch([(loc[:3].astype(np.int64), val[:3]), (loc[3:], val[3:])])


def test_caller_arrays_are_not_written_before_the_call(no_ffi):
    loc, val, off = _ok()
    before = (loc.copy(), val.copy())
    with pytest.raises(_NoFFI):
        auction_solve_sparse_batch(loc, val, off, problem="min")
    assert np.array_equal(loc, before[0]) and np.array_equal(val, before[1])


def test_bad_arguments_of_the_c_entry_point(built_lib):
    """Rejected before any device is touched: B, null pointers, offsets, options it does not take, the meta stride."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    loc, val, off = _ok()
    off = off.astype(np.int64)
    sol = np.empty((2, 2), dtype=np.int32)

    def call(B=2, loc=loc.ctypes.data, val=val.ctypes.data, off=off.ctypes.data, sol=sol.ctypes.data, sol_ld=2,
             meta=None, opts=o):
        return built_lib.misslap_solve_sparse_batch(B, loc, val, off, None, None, None, 0, 0, C.byref(opts), sol, sol_ld,
                                                    None, 0, 0, meta, None)

    def err():
        return built_lib.misslap_last_error().decode()

    assert call(B=0) == _lib.ERR_INVALID and "B = 0" in err()
    assert call(B=-3) == _lib.ERR_INVALID
    for kw in (dict(loc=None), dict(val=None), dict(off=None), dict(sol=None)):
        assert call(**kw) == _lib.ERR_INVALID and "null" in err(), kw
    bad = np.array([0, 4, 3], dtype=np.int64)
    assert call(off=bad.ctypes.data) == _lib.ERR_INVALID and "non-decreasing" in err()
    bad = np.array([1, 3, 6], dtype=np.int64)
    assert call(off=bad.ctypes.data) == _lib.ERR_INVALID and "offsets[0]" in err()
    assert call(sol_ld=0) == _lib.ERR_INVALID and "sol_ld" in err()
    metas = (_lib.DenseBatchMeta * 2)()
    assert call(meta=metas) == _lib.ERR_INVALID and "struct_size" in err()
    for field, v in (("tiled_min_K", 5), ("profile", 1), ("cand_mode", 1), ("shard_world", 2)):
        o2 = _lib.Options()
        C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
        setattr(o2, field, v)
        assert call(opts=o2) == _lib.ERR_INVALID and "every other option" in err(), field
