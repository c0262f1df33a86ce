"""Matching batch without a GPU: the entry points are declared, bound and exported, the header still compiles as plain
C, and hopcroft_solve_batch validates its arguments before any call into the library."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import _lib, hopcroft_solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("misslap_matching_batch", "misslap_matching_dense_batch")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in ENTRY_POINTS:
        assert name in declared
        assert name in _lib.SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r"#define MISSLAP_ABI_VERSION 2\b", header)
    cap = int(re.search(r"#define MISSLAP_MATCHING_BATCH_MAX_DIM (\d+)", header).group(1))
    assert cap == _lib.MATCHING_BATCH_MAX_DIM == 2048
    assert "hopcroft_solve_batch" in sslap_amd.__all__
    assert sslap_amd.hopcroft_solve_batch is hopcroft_solve_batch


def test_info_struct_layout_matches_header():
    import ctypes as C
    info = _lib.MatchingBatchInfo
    assert info.struct_size.offset == 0  # leading struct_size, so the struct can grow
    assert C.sizeof(info) == 40
    assert info.check_ms.offset == 16 and info.wall_ms.offset == 32


def test_header_compiles_as_plain_c():
    prog = ['#include "misslap.h"', '#include <stddef.h>', 'int main(void){',
            'misslap_matching_batch_info i = {0}; i.struct_size = (int32_t)sizeof i;',
            'int (*f)(int64_t, const int32_t *, const int64_t *, const misslap_options *, int32_t *, int32_t *, int32_t *,',
            '         int32_t *, int64_t, int32_t *, int64_t, int32_t, misslap_matching_batch_info *) = misslap_matching_batch;',
            'int (*g)(int64_t, int64_t, int64_t, const double *, const int32_t *, const misslap_options *, int32_t *,',
            '         int32_t *, int32_t *, int32_t *, int64_t, int32_t *, int64_t, int32_t,',
            '         misslap_matching_batch_info *) = misslap_matching_dense_batch;',
            'return (f == 0) + (g == 0) + (MISSLAP_MATCHING_BATCH_MAX_DIM != 2048) + (sizeof i != 40)',
            '       + (offsetof(misslap_matching_batch_info, check_ms) != 16);}']
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


def test_arguments_are_validated_before_ffi(no_ffi):
    loc = np.array([[0, 0], [0, 1], [1, 1], [0, 0]], dtype=np.int32)
    off = np.array([0, 3, 4])
    mats = np.ones((2, 3, 4))
    with pytest.raises(ValueError, match="exactly one"):
        hopcroft_solve_batch()
    with pytest.raises(ValueError, match="exactly one"):
        hopcroft_solve_batch(loc, off, mats=mats)
    with pytest.raises(ValueError, match="offsets is required"):
        hopcroft_solve_batch(loc)
    with pytest.raises(ValueError, match="shape"):
        hopcroft_solve_batch(loc.reshape(-1), off)
    with pytest.raises(ValueError, match="integer"):
        hopcroft_solve_batch(loc.astype(np.float64), off)
    with pytest.raises(ValueError, match="end at nnz"):
        hopcroft_solve_batch(loc, np.array([0, 3, 5]))
    with pytest.raises(ValueError, match="start at 0"):
        hopcroft_solve_batch(loc, np.array([1, 3, 4]))
    with pytest.raises(ValueError, match="non-decreasing"):
        hopcroft_solve_batch(loc, np.array([0, 3, 2, 4]))
    with pytest.raises(ValueError, match="length B"):
        hopcroft_solve_batch(loc, np.array([0]))
    with pytest.raises(TypeError, match="shapes goes with mats"):
        hopcroft_solve_batch(loc, off, shapes=np.array([[1, 1], [1, 1]]))
    with pytest.raises(TypeError, match="takes no offsets"):
        hopcroft_solve_batch([loc], off)
    with pytest.raises(TypeError):
        hopcroft_solve_batch([loc.tolist()])
    with pytest.raises(ValueError, match="graph 1"):
        hopcroft_solve_batch([loc, loc.astype(np.float32)])
    with pytest.raises(ValueError, match="no graphs"):
        hopcroft_solve_batch([])
    with pytest.raises(TypeError):
        hopcroft_solve_batch(loc.tolist(), off)
    with pytest.raises(TypeError, match="offsets goes with loc"):
        hopcroft_solve_batch(mats=mats, offsets=off)
    with pytest.raises(ValueError, match="dtype"):
        hopcroft_solve_batch(mats=mats.astype(np.float32))
    with pytest.raises(ValueError, match="3 dimensions"):
        hopcroft_solve_batch(mats=mats[0])
    with pytest.raises(ValueError, match="empty"):
        hopcroft_solve_batch(mats=np.ones((0, 3, 4)))
    with pytest.raises(ValueError, match="shapes must be"):
        hopcroft_solve_batch(mats=mats, shapes=np.array([[1, 1]]))
    with pytest.raises(ValueError, match=r"graph 1: shape \(4, 1\) outside"):
        hopcroft_solve_batch(mats=mats, shapes=np.array([[1, 1], [4, 1]]))
    with pytest.raises(ValueError, match=r"graph 0: 2049 x 4 exceeds MISSLAP_MATCHING_BATCH_MAX_DIM \(2048\)"):
        hopcroft_solve_batch(mats=np.ones((1, 2049, 4)))
    with pytest.raises(TypeError):
        hopcroft_solve_batch(mats=mats.tolist())
    # every call above failed before the library was loaded; a valid call reaches it
    with pytest.raises(_NoFFI):
        hopcroft_solve_batch(loc, off)
    with pytest.raises(_NoFFI):
        hopcroft_solve_batch(mats=mats, shapes=np.array([[3, 4], [1, 2]]))
