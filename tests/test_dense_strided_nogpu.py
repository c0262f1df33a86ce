"""Strided dense stacks without a GPU: the three strided entry points are declared, bound and exported, they reject a
negative stride, an extent beyond 62 bits and a host stack before any device is touched, and the front end keeps its
checks of dtype, rank and size on a strided device tensor and hands its strides on.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sslap_amd import _batch, _lib, auction_solve_batch, hopcroft_solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_dense_batch_status_strided", "misslap_solve_dense_batch_outside_strided",
         "misslap_matching_dense_batch_strided")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
        # the contiguous call's arguments with the three strides behind B, N, M
        base = _lib.SYMBOLS[name[:-len("_strided")]]
        assert _lib.SYMBOLS[name] == (base[0], base[1][:3] + [C.c_int64] * 3 + base[1][3:]), name


@pytest.fixture
def calls(built_lib):
    """name -> f(sB, sN, sM, B=.., N=.., M=.., on_device=..): the entry point on a 2 x 3 x 4 stack, every other argument
    valid.  mat is a host array: no call here may get as far as reading it."""
    mat = np.ones((2, 3, 4))
    sol, status = np.empty((2, 3), dtype=np.int32), np.empty(2, dtype=np.int32)
    outside = np.ones(2)
    size, rows, cols = (np.empty(2, dtype=np.int32) for _ in range(3))
    metas = (_lib.DenseBatchMeta * 2)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def options(on_device):
        o = _lib.Options()
        o.struct_size = C.sizeof(_lib.Options)
        o.max_iter = 10
        o.input_on_device = on_device
        return o

    def status_call(sB, sN, sM, B=2, N=3, M=4, on_device=1):
        return built_lib.misslap_solve_dense_batch_status_strided(
            B, N, M, sB, sN, sM, mat.ctypes.data, None, 0, None, 1, C.byref(options(on_device)), None, None, 0,
            sol.ctypes.data, None, 0, status.ctypes.data, None, C.cast(metas, C.c_void_p), None)

    def outside_call(sB, sN, sM, B=2, N=3, M=4, on_device=1):
        return built_lib.misslap_solve_dense_batch_outside_strided(
            B, N, M, sB, sN, sM, mat.ctypes.data, None, 1, None, C.byref(options(on_device)), None, None, 0,
            outside.ctypes.data, 0, sol.ctypes.data, None, None, 0, status.ctypes.data, None, C.cast(metas, C.c_void_p),
            None)

    def matching_call(sB, sN, sM, B=2, N=3, M=4, on_device=1):
        return built_lib.misslap_matching_dense_batch_strided(
            B, N, M, sB, sN, sM, mat.ctypes.data, None, C.byref(options(on_device)), size.ctypes.data, rows.ctypes.data,
            cols.ctypes.data, None, 0, None, 0, 0, None)

    return dict(zip(NAMES, (status_call, outside_call, matching_call)))


@pytest.mark.parametrize("name", NAMES)
def test_bad_strides_are_rejected_before_any_device_is_touched(calls, built_lib, name):
    call, err = calls[name], built_lib.misslap_last_error
    for strides in ((-1, 4, 1), (12, -4, 1), (12, 4, -1), (-2**63, 4, 1)):
        assert call(*strides) == _lib.ERR_INVALID, strides
        assert name.encode() in err() and b"stride must be >= 0" in err(), err()
    # (B - 1) sB + (N - 1) sN + (M - 1) sM: the last element's offset must fit 62 bits
    top = 2**62
    for strides in ((top, 4, 1), (12, top // 2, 1), (12, 4, top // 3 + 1), (2**63 - 1, 2**63 - 1, 2**63 - 1),
                    (top - 11, 4, 1)):
        assert call(*strides) == _lib.ERR_INVALID, strides
        assert name.encode() in err() and b"62 bits" in err(), err()
    # a host stack has no strides
    assert call(1, 8, 2, on_device=0) == _lib.ERR_INVALID and b"device array" in err()
    # the checks of the contiguous call still come first
    assert call(12, 4, 1, B=0) == _lib.ERR_INVALID and b"stride" not in err()
    if "matching" not in name:
        cap = _lib.DENSE_BATCH_MAX_DIM
        assert call(12, 4, 1, N=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_DENSE_BATCH_MAX_DIM" in err()


class _FakeDeviceTensor:
    """What the front end reads of a device tensor before the library is called, over a numpy view."""
    is_cuda = True

    def __init__(self, a, dtype):
        import torch
        self._a, self.dtype, self.shape = a, getattr(torch, dtype), a.shape

    def dim(self):
        return self._a.ndim

    def stride(self):
        return tuple(s // self._a.itemsize for s in self._a.strides)

    def is_contiguous(self):
        return self._a.flags.c_contiguous

    def data_ptr(self):
        raise AssertionError("the stack must not be touched")


def test_front_end_checks_a_strided_tensor_and_hands_its_strides_on():
    buf = np.zeros((4, 6, 10))
    views = {"transposed": buf.transpose(0, 2, 1), "cols": buf[:, :, 3:8], "rows": buf[:, 1:4], "batch": buf[::2],
             "generic": buf[:, ::2, ::3], "expanded": np.broadcast_to(buf[0], (5, 6, 10))}
    want = {"transposed": (60, 1, 10), "cols": (60, 10, 1), "rows": (60, 10, 1), "batch": (120, 10, 1),
            "generic": (60, 20, 3), "expanded": (0, 10, 1)}
    for key, v in views.items():
        t = _FakeDeviceTensor(v, "float64")
        B, N, M, on_device, dtype = _batch._check_stack(t, "float64")  # no "must be contiguous" any more
        assert (B, N, M) == v.shape and on_device and dtype == _lib.DTYPE_F64, key
        assert _batch._stack_strides(t, on_device) == want[key], key
    # a contiguous tensor and a numpy array take the calls they always took
    assert _batch._stack_strides(_FakeDeviceTensor(buf, "float64"), True) is None
    assert _batch._stack_strides(views["transposed"], False) is None
    # the existing errors, on strided input
    strided = _FakeDeviceTensor(views["transposed"], "float32")
    for f in (auction_solve_batch, lambda m, **kw: hopcroft_solve_batch(mats=m, **kw)):
        with pytest.raises(ValueError, match="mats must be float64"):
            f(strided)
        with pytest.raises(ValueError, match="mat_dtype is float16"):
            f(strided, mat_dtype="float16")
        with pytest.raises(ValueError, match="3 dimensions"):
            f(_FakeDeviceTensor(buf[0].T, "float64"))
        with pytest.raises(ValueError, match="empty stack"):
            f(_FakeDeviceTensor(buf[:, :0].transpose(0, 2, 1), "float64"))
    with pytest.raises(ValueError, match="at most"):
        auction_solve_batch(_FakeDeviceTensor(np.broadcast_to(buf[:1, :1, :1], (1, 2, 1025)), "float64"))
