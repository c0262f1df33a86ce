"""The dense batch's status mode without a GPU: the entry points are declared, bound and exported, the status constants
agree between the header and the binding, the workspace size is answered on the host, the whole-call argument errors
of auction_solve_batch(errors="status") raise before the library is reached, and the mixed batch the GPU test runs on
holds a problem of every status code."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, auction_solve_batch
from tests._status_fixture import N_CODES, expected_status, mixed_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("OK", "TOO_FEW_VALUES", "EMPTY_ROW", "INFINITE_VALUE", "INFEASIBLE", "PRICE_NOT_FINITE", "PRICE_NEGATIVE",
         "BAD_SHAPE")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in ("misslap_solve_dense_batch_status", "misslap_dense_batch_workspace_bytes"):
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    for name in ("raise_for_status", "batch_meta_to_host"):
        assert name in sslap_amd.__all__ and callable(getattr(sslap_amd, name))


def test_status_constants_match_the_header():
    prog = ['#include <stdio.h>', '#include "misslap.h"', 'int main(void){']
    prog += [f'printf("{n} %d\\n", MISSLAP_BATCH_STATUS_{n});' for n in NAMES]
    prog += ['int (*f)(int64_t, int64_t, int64_t, const double *, const int32_t *, int32_t, const double *, int32_t,',
             '         const misslap_options *, void *, void *, int64_t, int32_t *, double *, int32_t, int32_t *, int32_t *,',
             '         misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_dense_batch_status;',
             'int64_t (*g)(int64_t, int64_t, int64_t, int32_t, int32_t) = misslap_dense_batch_workspace_bytes;',
             'return (f == 0) + (g == 0);}']
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "t.c"), os.path.join(d, "t.o")
        open(src, "w").write("\n".join(prog))
        # the prototypes: compiled as plain C, not linked
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"),
                               src, "-o", obj])
        # the values: printed by a program that names no library symbol
        open(src, "w").write("\n".join(prog[:3 + len(NAMES)] + ["return 0;}"]))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src,
                               "-o", exe])
        out = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines())
    assert [int(out[n]) for n in NAMES] == list(range(8))
    for n in NAMES:
        assert getattr(_lib, "BATCH_STATUS_" + n) == int(out[n]), n


def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_dense_batch_workspace_bytes
    cap = _lib.DENSE_BATCH_MAX_DIM
    sizes = [f(B, 64, 64, 0, 1) for B in (1, 2, 63, 64, 65, 1024, 100000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert f(1024, 64, 64, 0, 0) < f(1024, 64, 64, 0, 1)  # the cardinalities
    assert f(1024, 64, 64, 0, 1) >= 1024 * (32 + 8 + 4)  # a check record, a shape and a cardinality per problem
    assert f(1, cap, cap, 1, 1) > 0
    for bad in ((0, 4, 4), (1, cap + 1, 4), (1, 4, cap + 1), (1, 0, 4), (-1, 4, 4)):
        assert f(*bad, 0, 1) == -1, bad


class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


def test_whole_call_errors_still_raise_before_ffi(no_ffi):
    ok = np.ones((2, 3, 4))
    with pytest.raises(ValueError, match="errors must be"):
        auction_solve_batch(ok, errors="bogus")
    st = dict(errors="status")
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_batch(ok.astype(np.float32), **st)
    with pytest.raises(ValueError, match="3 dimensions"):
        auction_solve_batch(np.ones((3, 4)), **st)
    with pytest.raises(TypeError):
        auction_solve_batch([[[1.0]]], **st)
    with pytest.raises(ValueError, match="from_matrix / solve_batch"):
        auction_solve_batch(np.ones((1, 2, _lib.DENSE_BATCH_MAX_DIM + 1)), **st)
    with pytest.raises(ValueError, match="problem 1: shape"):
        auction_solve_batch(ok, shapes=np.array([[3, 4], [4, 4]]), **st)
    with pytest.raises(ValueError, match="shapes"):
        auction_solve_batch(ok, shapes=np.ones((3, 2), dtype=int), **st)
    with pytest.raises(ValueError, match="shape"):
        auction_solve_batch(ok, prices=np.zeros((2, 3)), **st)
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_batch(ok, prices=np.zeros((2, 4), dtype=np.float32), **st)
    with pytest.raises(ValueError, match="NaN"):
        auction_solve_batch(ok, eps_start=float("nan"), **st)
    with pytest.raises(_NoFFI):  # valid arguments do reach the library
        auction_solve_batch(ok, shapes=np.array([[3, 4], [1, 1]]), prices=np.zeros((2, 4)), fast=True, **st)
    with pytest.raises(_NoFFI):  # ... and the default mode is still the default
        auction_solve_batch(ok)


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    """Argument errors come before any device is touched; valid arguments reach the device (MISSLAP_ERR_NO_DEVICE here)."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    m = np.ones((1, 2, 2))
    sol = np.empty((1, 2), dtype=np.int32)
    status = np.empty(1, dtype=np.int32)
    metas = (_lib.DenseBatchMeta * 1)()

    def call(B=1, N=2, M=2, shapes=None, meta=None, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0):
        return built_lib.misslap_solve_dense_batch_status(B, N, M, m.ctypes.data, shapes, 0, None, 1, C.byref(opts), None,
                                                          work, nwork, sol.ctypes.data, None, on_dev, st, None,
                                                          None if meta is None else C.cast(meta, C.c_void_p), None)

    cap = _lib.DENSE_BATCH_MAX_DIM
    assert call(N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_DENSE_BATCH_MAX_DIM" in built_lib.misslap_last_error()
    assert call(M=cap + 1) == _lib.ERR_INVALID
    assert call(B=0) == _lib.ERR_INVALID
    assert call(st=None) == _lib.ERR_INVALID and b"status" in built_lib.misslap_last_error()
    bad = np.array([[2, 3]], dtype=np.int32)
    assert call(shapes=bad.ctypes.data) == _lib.ERR_INVALID and b"problem 0" in built_lib.misslap_last_error()
    assert call(meta=metas) == _lib.ERR_INVALID and b"struct_size" in built_lib.misslap_last_error()
    o2 = _lib.Options()
    C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
    o2.tiled_min_K = 5
    assert call(opts=o2) == _lib.ERR_INVALID and b"every other option" in built_lib.misslap_last_error()
    # with a workspace: every array on the device, the workspace large enough and aligned
    o3 = _lib.Options()
    C.memmove(C.byref(o3), C.byref(o), C.sizeof(o))
    o3.input_on_device = 1
    need = built_lib.misslap_dense_batch_workspace_bytes(1, 2, 2, 0, 1)
    assert call(work=4096, nwork=need, on_dev=1, meta=metas) == _lib.ERR_INVALID  # (input_on_device not set)
    assert b"on the device" in built_lib.misslap_last_error()
    assert call(work=4096, nwork=need - 1, on_dev=1, meta=metas, opts=o3) == _lib.ERR_INVALID
    assert b"workspace" in built_lib.misslap_last_error()
    assert call(work=4096 + 8, nwork=need, on_dev=1, meta=metas, opts=o3) == _lib.ERR_INVALID  # misaligned
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)
    rc = call(meta=metas)  # valid host arguments: only the GPU can be missing
    assert rc in (0, _lib.ERR_NO_DEVICE), built_lib.misslap_last_error()
    if rc:
        assert b"no CPU fallback" in built_lib.misslap_last_error()
    else:
        assert status[0] == 0 and metas[0].n_rows == 2


def test_mixed_fixture_holds_every_status_code(built_lib):
    fx = mixed_batch()
    mats, shapes, prices, kinds = fx["mats"], fx["shapes"], fx["prices"], fx["kinds"]
    B = mats.shape[0]
    assert B >= 96 + B // (2 * N_CODES) + 1  # at least 96 problems are left when the shapes of code 7 are taken out
    status, size = expected_status(mats, shapes, prices)
    assert np.array_equal(status, kinds)  # every planted defect is the FIRST check its problem fails
    for code in range(1, N_CODES + 1):
        assert (status == code).sum() >= 2, code  # plain, and with a later check failing too
    assert (status == 0).sum() * 2 >= B
    assert np.array_equal(size[status == 7], np.full((status == 7).sum(), -1))
    ok = status == 0
    assert (size[ok] == shapes[ok, 0]).all() and (size[status == 4] < shapes[status == 4, 0]).all()
    # without the guard an infeasible problem falls through to its prices, or to a solve
    nocheck, nosize = expected_status(mats, shapes, prices, cardinality_check=False)
    assert not (nocheck == 4).any() and (nosize == -1).all()
    assert set(nocheck[status == 4]) == {0, 6}
    # a batch below the device guard's threshold of the default mode keeps every kind
    small = expected_status(mats[:60], shapes[:60], prices[:60])[0]
    assert set(small) == set(range(N_CODES + 1))
