"""Warm-started re-solve without a GPU: the new C entry points are declared and exported, fail cleanly on bad handles, and
the Python front-end validates its arguments before any call into the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sslap_amd import AuctionSolver, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("misslap_get_prices", "misslap_update_values", "misslap_update_dense", "misslap_resolve")


def test_new_symbols_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
    assert re.search(r"#define MISSLAP_ABI_VERSION 2\b", header)


def test_new_calls_fail_cleanly_on_a_null_handle(built_lib):
    p = np.zeros(4)
    d = C.c_double(0.0)
    assert built_lib.misslap_get_prices(None, p.ctypes.data, 0) == _lib.ERR_INVALID
    assert built_lib.misslap_update_values(None, p.ctypes.data, 4, 0, None, C.byref(d)) == _lib.ERR_INVALID
    assert built_lib.misslap_update_dense(None, p.ctypes.data, 0, None, C.byref(d)) == _lib.ERR_INVALID
    assert built_lib.misslap_resolve(None, p.ctypes.data, 0, 0.0, None, None) == _lib.ERR_INVALID
    assert b"null" in built_lib.misslap_last_error()


class _NoFFI(Exception):
    pass


@pytest.fixture
def fake_solver(monkeypatch):
    """A solver object with dimensions but no handle; any call into the library raises _NoFFI."""
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)
    s = AuctionSolver.__new__(AuctionSolver)
    s._h, s.num_rows, s.num_cols, s.nnz = None, 3, 4, 6
    s.meta, s.gpu = {}, {}
    return s


def test_resolve_validates_prices_before_ffi(fake_solver):
    s = fake_solver
    for bad in (-1.0, np.nan, np.inf, -np.inf, -0.0):
        p = np.ones(4)
        p[2] = bad
        with pytest.raises(ValueError):
            s.resolve(prices=p)
    with pytest.raises(ValueError, match="shape"):
        s.resolve(prices=np.ones(5))
    with pytest.raises(ValueError, match="shape"):
        s.resolve(prices=np.ones((2, 2)))
    with pytest.raises(ValueError, match="dtype"):
        s.resolve(prices=np.ones(4, dtype=np.float32))
    with pytest.raises(TypeError):
        s.resolve(prices=[1.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="NaN"):
        s.resolve(eps_start=float("nan"))
    with pytest.raises(_NoFFI):  # valid arguments do reach the library
        s.resolve(prices=np.ones(4), eps_start=0.5)


def test_update_values_validates_before_ffi(fake_solver):
    s = fake_solver
    with pytest.raises(ValueError, match="dtype"):
        s.update_values(np.ones(6, dtype=np.float32))
    with pytest.raises(ValueError, match="6 entries"):
        s.update_values(np.ones(5))
    with pytest.raises(ValueError, match="NaN"):
        s.update_values(np.array([1.0, 2, 3, np.nan, 5, 6]))
    with pytest.raises(ValueError, match="NaN"):
        s.update_values(np.array([1.0, 2, 3, np.inf, 5, 6]))
    with pytest.raises(ValueError, match="from_matrix"):
        s.update_values(np.ones((3, 4)))  # not a from_matrix solver
    with pytest.raises(ValueError, match="dimensions"):
        s.update_values(np.ones((1, 2, 3)))
    with pytest.raises(TypeError):
        s.update_values([1.0] * 6)
    s._dense_shape = (3, 4)
    with pytest.raises(ValueError, match="shape"):
        s.update_values(np.ones((4, 3)))
    with pytest.raises(ValueError, match="inf"):
        s.update_values(np.full((3, 4), np.inf))
    with pytest.raises(_NoFFI):
        s.update_values(np.ones((3, 4)))
    with pytest.raises(_NoFFI):
        s.update_values(np.ones(6))
