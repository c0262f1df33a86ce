"""Dense batch without a GPU: the entry point is declared and exported, the new structs' ctypes layout matches the header,
the header still compiles as plain C, and auction_solve_batch validates its arguments before any call into the
library."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, auction_solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    assert "misslap_solve_dense_batch" in set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    assert "misslap_solve_dense_batch" in _lib.SYMBOLS
    assert getattr(built_lib, "misslap_solve_dense_batch") is not None
    assert re.search(r"#define MISSLAP_ABI_VERSION 2\b", header)
    cap = int(re.search(r"#define MISSLAP_DENSE_BATCH_MAX_DIM (\d+)", header).group(1))
    assert cap == _lib.DENSE_BATCH_MAX_DIM >= 1024
    assert "auction_solve_batch" in sslap_amd.__all__


def _compile_and_run(prog, std):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(prog))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                               src, "-o", exe])
        return subprocess.check_output([exe], text=True)


def test_struct_layouts_match_header():
    types = {"misslap_dense_batch_meta": _lib.DenseBatchMeta, "misslap_dense_batch_info": _lib.DenseBatchInfo}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "misslap.h"', 'int main(void){']
    for s, t in types.items():
        prog.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in t._fields_:
            prog.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    prog.append("return 0;}")
    out = dict(line.split() for line in _compile_and_run(prog, "c99").splitlines())
    for s, t in types.items():
        assert int(out[s]) == C.sizeof(t), s
        for f, _ in t._fields_:
            assert int(out[f"{s}.{f}"]) == getattr(t, f).offset, (s, f)


def test_header_compiles_as_plain_c():
    prog = ['#include "misslap.h"', 'int main(void){',
            'misslap_dense_batch_meta m = {0}; m.struct_size = (int32_t)sizeof m;',
            'int (*f)(int64_t, int64_t, int64_t, const double *, const int32_t *, const float *, const double *, int32_t,',
            '         const misslap_options *, int32_t *, double *, int32_t, misslap_dense_batch_meta *,',
            '         misslap_dense_batch_info *) = misslap_solve_dense_batch;',
            'return (f == 0) + (m.struct_size != 80);}']
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I",
                               os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t.o")])


class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


def test_arguments_are_validated_before_ffi(no_ffi):
    ok = np.ones((2, 3, 4))
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_batch(ok.astype(np.float32))
    with pytest.raises(ValueError, match="3 dimensions"):
        auction_solve_batch(np.ones((3, 4)))
    with pytest.raises(ValueError, match="3 dimensions"):
        auction_solve_batch(np.ones((1, 2, 3, 4)))
    with pytest.raises(TypeError):
        auction_solve_batch([[[1.0]]])
    with pytest.raises(ValueError, match="from_matrix / solve_batch"):
        auction_solve_batch(np.ones((1, 2, _lib.DENSE_BATCH_MAX_DIM + 1)))
    with pytest.raises(ValueError, match="from_matrix / solve_batch"):
        auction_solve_batch(np.ones((1, _lib.DENSE_BATCH_MAX_DIM + 1, 2)))
    with pytest.raises(ValueError, match="empty"):
        auction_solve_batch(np.ones((0, 3, 4)))
    with pytest.raises(ValueError, match="shapes"):
        auction_solve_batch(ok, shapes=np.ones((3, 2), dtype=int))
    with pytest.raises(ValueError, match="shapes"):
        auction_solve_batch(ok, shapes=np.ones((2, 2)))  # not integers
    with pytest.raises(ValueError, match="problem 1: shape"):
        auction_solve_batch(ok, shapes=np.array([[3, 4], [4, 4]]))
    with pytest.raises(ValueError, match="problem 0: shape"):
        auction_solve_batch(ok, shapes=np.array([[3, 0], [3, 4]]))
    with pytest.raises(ValueError, match="shape"):
        auction_solve_batch(ok, prices=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_batch(ok, prices=np.zeros((2, 4), dtype=np.float32))
    with pytest.raises(TypeError):
        auction_solve_batch(ok, prices=[[0.0] * 4] * 2)
    with pytest.raises(ValueError, match="NaN"):
        auction_solve_batch(ok, eps_start=float("nan"))
    with pytest.raises(_NoFFI):  # valid arguments do reach the library
        auction_solve_batch(ok, shapes=np.array([[3, 4], [1, 1]]), prices=np.zeros((2, 4)), fast=True)


def test_caller_array_is_not_written_before_the_call(no_ffi):
    m = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    before = m.copy()
    with pytest.raises(_NoFFI):
        auction_solve_batch(m, problem="min")
    assert np.array_equal(m, before)


def test_bad_arguments_of_the_c_entry_point(built_lib):
    """Rejected before any device is touched (the cap, shapes, the meta stride, options it does not take)."""
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    m = np.ones((1, 2, 2))
    sol = np.empty((1, 2), dtype=np.int32)

    def call(B=1, N=2, M=2, shapes=None, meta=None, opts=o):
        return built_lib.misslap_solve_dense_batch(B, N, M, m.ctypes.data, shapes, None, None, 0, C.byref(opts),
                                                   sol.ctypes.data, None, 0, meta, None)

    cap = _lib.DENSE_BATCH_MAX_DIM
    assert call(N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_DENSE_BATCH_MAX_DIM" in built_lib.misslap_last_error()
    assert call(M=cap + 1) == _lib.ERR_INVALID
    assert call(B=0) == _lib.ERR_INVALID
    bad = np.array([[2, 3]], dtype=np.int32)
    assert call(shapes=bad.ctypes.data) == _lib.ERR_INVALID and b"problem 0" in built_lib.misslap_last_error()
    metas = (_lib.DenseBatchMeta * 1)()
    assert call(meta=metas) == _lib.ERR_INVALID and b"struct_size" in built_lib.misslap_last_error()
    o2 = _lib.Options()
    C.memmove(C.byref(o2), C.byref(o), C.sizeof(o))
    o2.tiled_min_K = 5
    assert call(opts=o2) == _lib.ERR_INVALID and b"every other option" in built_lib.misslap_last_error()
