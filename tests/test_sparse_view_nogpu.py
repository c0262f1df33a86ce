"""The sparse batch on a view of the packed arrays (misslap_solve_sparse_batch_status_view / _outside_view) without a GPU:
the three entry points are declared, bound and exported and their prototypes compile as C99; every whole-call error of
the C entry points comes before a device is touched; the workspace function; and the front end's choice between the
contiguous and the view entry points, with its checks of device offsets, sizes, loc and val, on faked device tensors.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from sslap_amd import _batch, _lib, auction_solve_sparse_batch
from sslap_amd import sparse_batch as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_sparse_batch_status_view", "misslap_solve_sparse_batch_outside_view",
         "misslap_sparse_batch_view_workspace_bytes")
CAP = _lib.SPARSE_BATCH_MAX_DIM


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    # the view forms: (B, nnz, loc, loc_int64, stride_e, stride_c, val, offsets_dev) for (B, loc, val, offsets, offsets_dev)
    head = [C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    for name in NAMES[:2]:
        base = _lib.SYMBOLS[name[:-len("_view")]]
        assert _lib.SYMBOLS[name] == (base[0], head + base[1][5:]), name
    # no new status code: the view's unusable slice is BAD_SHAPE
    codes = dict(re.findall(r"#define MISSLAP_BATCH_STATUS_([A-Z_]+) (\d+)", header))
    assert sorted(int(v) for v in codes.values()) == list(range(16)) and int(codes["BAD_SHAPE"]) == 7


def test_prototypes_compile_as_c99():
    prog = ['#include "misslap.h"', 'int main(void){',
            'int (*f)(int64_t, int64_t, const void *, int32_t, int64_t, int64_t, const void *, const int64_t *, const int64_t *,',
            '         int32_t, const double *, int64_t, int32_t, const misslap_options *, void *, void *, int64_t, int64_t,',
            '         int64_t, int32_t *, double *, int32_t, int32_t *, int32_t *, misslap_dense_batch_meta *,',
            '         misslap_dense_batch_info *) = misslap_solve_sparse_batch_status_view;',
            'int (*g)(int64_t, int64_t, const void *, int32_t, int64_t, int64_t, const void *, const int64_t *, const int64_t *,',
            '         int32_t, const double *, int64_t, const misslap_options *, void *, void *, int64_t, int64_t, int64_t,',
            '         const double *, int64_t, int32_t *, double *, double *, int32_t, int32_t *, int32_t *,',
            '         misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_sparse_batch_outside_view;',
            'int64_t (*h)(int64_t, int64_t, int64_t, int32_t, int32_t) = misslap_sparse_batch_view_workspace_bytes;',
            'return (f == 0) + (g == 0) + (h == 0) + (MISSLAP_BATCH_STATUS_BAD_SHAPE != 7);}']
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "t.c"), os.path.join(d, "t.o")
        open(src, "w").write("\n".join(prog))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", "-I", os.path.join(ROOT, "include"),
                               src, "-o", obj])


# ---- the workspace function

def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_sparse_batch_view_workspace_bytes
    for B, nnz, N in ((1, 0, 1), (2, 7, 5), (64, 10**6, CAP), (100000, 3 * 10**6, 40), (2**31 - 1, 2**40, 1)):
        for guard in (0, 1):
            w = f(B, nnz, N, 0, guard)
            assert w > 0 and w % 256 == 0, (B, nnz, N)
            # a check record (32 bytes) and Nmax + 1 row starts per problem, and the guard's cardinalities
            assert w >= 32 * B + 4 * B * (N + 1) + (4 * B if guard else 0), (B, nnz, N, guard)
            assert f(B, nnz, N, 1, guard) >= w  # has_prices
            assert f(B, nnz + 1000, N, 0, guard) >= w  # monotone in nnz ...
            if B < 2**31 - 1:
                assert f(B + 1, nnz, N, 0, guard) >= w  # ... in B ...
            if N < CAP:
                assert f(B, nnz, N + 1, 0, guard) >= w  # ... and in Nmax
        assert f(B, nnz, N, 0, 1) >= f(B, nnz, N, 0, 0) + 4 * B
    assert f(8, 100, 64, 0, 1) > f(8, 100, 8, 0, 1) and f(80, 100, 8, 0, 1) > f(8, 100, 8, 0, 1)
    for bad in ((0, 4, 4), (2**31, 4, 4), (-1, 4, 4), (1, -1, 4), (1, 2**57, 4), (1, 4, 0), (1, 4, CAP + 1), (1, 4, -3)):
        assert f(*bad, 0, 1) == -1, bad


# ---- the C entry points: every whole-call error before a device is touched

def _options(**fields):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    o.input_on_device = 1
    for k, v in fields.items():
        setattr(o, k, v)
    return o


@pytest.fixture
def calls(built_lib):
    """name -> f(**overrides): the entry point on two problems of 3 entries in all, every other argument valid.  The
    arrays are host arrays: no call here may get as far as reading them."""
    loc = np.array([[0, 1], [1, 0], [0, 0]], dtype=np.int64)
    val = np.array([1.0, 2.0, 3.0])
    off = np.array([0, 2, 3], dtype=np.int64)
    outside = np.array([4.0, 5.0])
    sol, status = np.empty((2, 3), dtype=np.int32), np.empty(2, dtype=np.int32)
    oprices = np.empty((2, 3))
    metas = (_lib.DenseBatchMeta * 2)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)
    base = dict(B=2, nnz=3, lo=loc.ctypes.data, wide=1, se=2, sc=1, va=val.ctypes.data, off=off.ctypes.data, p=None, p_ld=0,
                opts=None, work=None, nwork=0, Nmax=3, Mmax=2, so=sol.ctypes.data, on_dev=0, st=status.ctypes.data,
                out=outside.ctypes.data, ld=0)

    def status_call(**kw):
        a = dict(base, **kw)
        return built_lib.misslap_solve_sparse_batch_status_view(
            a["B"], a["nnz"], a["lo"], a["wide"], a["se"], a["sc"], a["va"], a["off"], None, 0, a["p"], a["p_ld"], 1,
            C.byref(a["opts"] or _options()), None, a["work"], a["nwork"], a["Nmax"], a["Mmax"], a["so"], None, a["on_dev"],
            a["st"], None, C.cast(metas, C.c_void_p), None)

    def outside_call(**kw):
        a = dict(base, **kw)
        return built_lib.misslap_solve_sparse_batch_outside_view(
            a["B"], a["nnz"], a["lo"], a["wide"], a["se"], a["sc"], a["va"], a["off"], None, 1, a["p"], a["p_ld"],
            C.byref(a["opts"] or _options()), None, a["work"], a["nwork"], a["Nmax"], a["Mmax"], a["out"], a["ld"], a["so"],
            None, oprices.ctypes.data, a["on_dev"], a["st"], None, C.cast(metas, C.c_void_p), None)

    return dict(zip(NAMES[:2], (status_call, outside_call))), val


@pytest.mark.parametrize("name", NAMES[:2])
def test_whole_call_errors_come_before_any_device_is_touched(calls, built_lib, name):
    (by_name, val), err = calls, built_lib.misslap_last_error
    call = by_name[name]
    for strides in ((-1, 1), (2, -1), (-2**63, 1), (2, -2**63)):
        assert call(se=strides[0], sc=strides[1]) == _lib.ERR_INVALID, strides
        assert name.encode() in err() and b"stride must be >= 0" in err(), err()
    # (nnz - 1) * stride_e + stride_c: the last element's offset must fit 62 bits
    top = 2**62
    for nnz, se, sc in ((3, top // 2, 1), (3, 2, top), (2, top - 1, 1), (2**56, 2**6, 64), (3, 2**63 - 1, 2**63 - 1),
                        (1, 0, top)):
        assert call(nnz=nnz, se=se, sc=sc) == _lib.ERR_INVALID, (nnz, se, sc)
        assert name.encode() in err() and b"62 bits" in err(), err()
    for dtype in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
        assert call(opts=_options(mat_dtype=dtype)) == _lib.ERR_INVALID and b"float64 or float32" in err(), dtype
    assert call(opts=_options(input_on_device=0)) == _lib.ERR_INVALID and b"device arrays: set input_on_device" in err()
    assert call(lo=None) == _lib.ERR_INVALID and b"null loc" in err()
    assert call(va=None) == _lib.ERR_INVALID and b"null loc / val" in err()
    assert call(off=None) == _lib.ERR_INVALID and b"offsets_dev" in err()
    assert call(so=None) == _lib.ERR_INVALID and b"sol" in err()
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    for dims in (dict(Nmax=0), dict(Nmax=CAP + 1), dict(Mmax=0), dict(Mmax=CAP + 1), dict(Nmax=-1)):
        assert call(**dims) == _lib.ERR_INVALID and b"MISSLAP_SPARSE_BATCH_MAX_DIM" in err(), dims
    assert call(B=0) == _lib.ERR_INVALID and call(B=2**31) == _lib.ERR_INVALID
    assert call(nnz=-1) == _lib.ERR_INVALID and b"nnz" in err()
    assert call(p=val.ctypes.data, p_ld=0) == _lib.ERR_INVALID and b"prices_ld" in err()
    assert call(opts=_options(tail_threshold=5)) == _lib.ERR_INVALID and (name + " takes").encode() in err()
    if name.endswith("outside_view"):
        assert call(out=None) == _lib.ERR_INVALID and b"null outside" in err()
        for ld in (1, 2, -1):
            assert call(ld=ld) == _lib.ERR_INVALID and b"outside_ld" in err(), ld
        sizing, need = "misslap_sparse_batch_outside_workspace_bytes", \
            built_lib.misslap_sparse_batch_outside_workspace_bytes(2, 3, 2, 0)
    else:
        sizing, need = NAMES[2], built_lib.misslap_sparse_batch_view_workspace_bytes(2, 3, 3, 0, 1)
    # a workspace: out_on_device, its size, its alignment
    assert call(work=4096, nwork=need, on_dev=0) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1) == _lib.ERR_INVALID and sizing.encode() in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1) == _lib.ERR_INVALID and sizing.encode() in err()
    # valid arguments: only the GPU can be missing.  nnz = 0 takes a null loc / val, and int32 / float32 are taken
    for kw in (dict(), dict(nnz=0, lo=None, va=None), dict(wide=0, opts=_options(mat_dtype=_lib.DTYPE_F32)),
               dict(se=3, sc=1), dict(se=1, sc=3), dict(se=0, sc=0), dict(work=4096, nwork=need, on_dev=1)):
        assert call(**kw) == _lib.ERR_NO_DEVICE, (kw, err())
        assert b"no CPU fallback" in err()


# ---- the front end, on faked device tensors

class _Device:
    def __init__(self, index):
        self.index = index

    def __eq__(self, other):
        return isinstance(other, _Device) and other.index == self.index

    def __ne__(self, other):
        return not self == other

    def __repr__(self):
        return f"cuda:{self.index}"


class _FakeDeviceTensor:
    """What the front end reads of a device tensor before the library is called, over a numpy view."""
    is_cuda = True

    def __init__(self, a, dtype=None, device=0):
        import torch
        self._a, self.shape, self.device = a, a.shape, _Device(device)
        self.dtype = getattr(torch, dtype or a.dtype.name)

    def dim(self):
        return self._a.ndim

    def stride(self):
        return tuple(s // self._a.itemsize for s in self._a.strides)

    def is_contiguous(self):
        return self._a.flags.c_contiguous

    def data_ptr(self):
        return self._a.__array_interface__["data"][0]


NNZ = 5
OFF = np.array([0, 3, 5])


def _inputs(index="int64", layout="compact", values="float64"):
    if layout == "compact":
        loc = np.zeros((NNZ, 2), dtype=index)
    elif layout == "wide":  # idx[:, 1:] of an (nnz, 3) nonzero()
        loc = np.zeros((NNZ, 3), dtype=index)[:, 1:]
    else:  # coo.indices()[1:].t()
        loc = np.zeros((3, NNZ), dtype=index)[1:].T
    return _FakeDeviceTensor(loc), _FakeDeviceTensor(np.zeros(NNZ, dtype=values))


def test_which_entry_point_a_call_takes():
    # contiguous int32 / float64 with host offsets: the calls it always took
    lo, va = _inputs("int32")
    B, nnz, off, on_device, view = sb._check_input(lo, va, OFF)
    assert (B, nnz, on_device, view) == (2, NNZ, True, None) and off.dtype == np.int64 and np.array_equal(off, OFF)
    # ... and so do numpy arrays
    assert sb._check_input(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ), OFF)[3:] == (False, None)
    # everything else: the view entry points, with the tensor's own strides, its index and value types
    d_off = _FakeDeviceTensor(OFF.astype(np.int64))
    want = {"compact": (2, 1), "wide": (3, 1), "transposed": (1, NNZ)}
    for index in ("int32", "int64"):
        for layout, strides in want.items():
            for values, dtype in (("float64", _lib.DTYPE_F64), ("float32", _lib.DTYPE_F32)):
                for offsets in (OFF, d_off):
                    lo, va = _inputs(index, layout, values)
                    B, nnz, off, on_device, view = sb._check_input(lo, va, offsets)
                    plain = index == "int32" and layout == "compact" and values == "float64" and offsets is OFF
                    assert (B, nnz, on_device) == (2, NNZ, True) and (view is None) == plain, (index, layout, values)
                    if plain:
                        continue
                    assert view == dict(int64=index == "int64", strides=strides, dtype=dtype), (index, layout, values)
                    assert off is offsets or np.array_equal(off, OFF)
                    # the head of the view call: B, nnz, loc where it lies, the flag, the strides, val, offsets
                    head = sb._view_head(B, nnz, lo, va, view, d_off)
                    assert head == (2, NNZ, lo.data_ptr(), int(index == "int64"), *strides, va.data_ptr(), d_off.data_ptr())
    # device offsets alone force the view path
    lo, va = _inputs("int32")
    assert sb._check_input(lo, va, d_off)[4] == dict(int64=False, strides=(2, 1), dtype=_lib.DTYPE_F64)
    lo, va = _inputs("int64", "wide")
    assert lo.data_ptr() == lo._a.base.__array_interface__["data"][0] + 8  # the view's first element, not the buffer's


def test_device_offsets_and_sizes_are_checked():
    f = auction_solve_sparse_batch
    lo, va = _inputs()
    d_off = _FakeDeviceTensor(OFF.astype(np.int64))
    # no wait may hide in the call: device offsets need dims, in both modes that take them
    for kw in (dict(errors="status"), dict(outside=1.0), dict(outside=1.0, errors="status")):
        with pytest.raises(ValueError, match=r"offsets on the device need dims=\(Nmax, Mmax\)"):
            f(lo, va, d_off, **kw)
    # the default mode reads offsets on the host
    with pytest.raises(TypeError, match="offsets on the device are taken with errors='status' or with outside="):
        f(lo, va, d_off)
    for bad in (_FakeDeviceTensor(OFF.astype(np.int64), device=1), _FakeDeviceTensor(OFF.astype(np.int32)),
                _FakeDeviceTensor(OFF.astype(np.float64)), _FakeDeviceTensor(np.zeros((3, 1), dtype=np.int64)),
                _FakeDeviceTensor(np.zeros(1, dtype=np.int64)), _FakeDeviceTensor(np.zeros(6, dtype=np.int64)[::2])):
        with pytest.raises(ValueError, match=r"device offsets must be a contiguous int64 tensor of shape \(B \+ 1,\)"):
            f(lo, va, bad, errors="status", dims=(4, 4))
    # device offsets with host loc / val: the wrong side, as before
    with pytest.raises(TypeError, match="offsets must be a host array"):
        f(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ), d_off, errors="status", dims=(4, 4))
    with pytest.raises(TypeError, match="offsets must be a host array"):
        _batch._check_offsets(d_off, NNZ, "")
    for bad in (_FakeDeviceTensor(np.zeros((2, 2), dtype=np.int64), device=1), _FakeDeviceTensor(np.zeros((2, 2), dtype=np.int32)),
                _FakeDeviceTensor(np.zeros((3, 2), dtype=np.int64)), _FakeDeviceTensor(np.zeros((2, 4), dtype=np.int64)[:, ::2])):
        with pytest.raises(ValueError, match=r"device sizes must be a contiguous int64 tensor of shape \(2, 2\)"):
            f(lo, va, d_off, sizes=bad, errors="status", dims=(4, 4))
    with pytest.raises(TypeError, match="sizes on the device need loc / val on the device"):
        f(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ), OFF, sizes=_FakeDeviceTensor(np.zeros((2, 2), dtype=np.int64)))
    good = _FakeDeviceTensor(np.zeros((2, 2), dtype=np.int64))
    assert sb._check_sizes(good, 2, _Device(0)) is good


def test_loc_and_val_are_checked():
    f = auction_solve_sparse_batch
    lo, va = _inputs()
    with pytest.raises(ValueError, match="val must be float64 or float32, got torch.float16"):
        f(lo, _FakeDeviceTensor(np.zeros(NNZ, dtype=np.float16)), OFF, errors="status")
    with pytest.raises(ValueError, match="val must be float64 or float32, got torch.bfloat16"):
        f(lo, _FakeDeviceTensor(np.zeros(NNZ, dtype=np.float16), "bfloat16"), OFF, errors="status")
    with pytest.raises(ValueError, match="loc must be int32 or int64, got torch.int16"):
        f(_FakeDeviceTensor(np.zeros((NNZ, 2), dtype=np.int16)), va, OFF, errors="status")
    with pytest.raises(ValueError, match="a device val tensor must be contiguous"):
        f(lo, _FakeDeviceTensor(np.zeros(2 * NNZ)[::2]), OFF, errors="status")
    with pytest.raises(ValueError, match=r"loc must have shape \(nnz, 2\)"):
        f(_FakeDeviceTensor(np.zeros((NNZ, 3), dtype=np.int64)), va, OFF, errors="status")
    with pytest.raises(ValueError, match="loc holds 5 entries, val 4"):
        f(lo, _FakeDeviceTensor(np.zeros(4)), OFF, errors="status")
    with pytest.raises(ValueError, match="loc is on cuda:0, val on cuda:1"):
        f(lo, _FakeDeviceTensor(np.zeros(NNZ), device=1), OFF, errors="status")
    # host numpy arrays keep every rule and text they had
    with pytest.raises(ValueError, match="^loc must be int32, got int64$"):
        f(np.zeros((NNZ, 2), dtype=np.int64), np.zeros(NNZ), OFF)
    with pytest.raises(ValueError, match="^Buffer dtype mismatch, expected 'DTYPE_t' but got 'float'$"):
        f(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ, dtype=np.float32), OFF)
    with pytest.raises(ValueError, match=r"^offsets must start at 0 and end at nnz = 5, got 0 \.\. 4$"):
        f(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ), [0, 3, 4], errors="status")
    with pytest.raises(ValueError, match=r"^offsets must be non-decreasing \(offsets\[1\] > offsets\[2\]\)$"):
        f(np.zeros((NNZ, 2), dtype=np.int32), np.zeros(NNZ), [0, 4, 3, 5], errors="status")
    with pytest.raises(TypeError, match="loc and val must both be numpy arrays or both tensors on the device"):
        f(lo, np.zeros(NNZ), OFF)


def test_the_text_of_an_unusable_slice():
    """raise_for_status names the offsets behind code 7, in the plain mode and, where the slice is the reason, in the
    outside mode; a bad sizes row keeps its own text."""
    from sslap_amd import raise_for_status
    meta = dict(n_rows=np.zeros(3, dtype=np.int64), n_cols=np.zeros(3, dtype=np.int64))
    res = dict(status=np.array([0, 7, 0], dtype=np.int32), matching_size=np.full(3, -1, dtype=np.int32), meta=meta,
               layout="sparse", dims=(4, 4), sizes=None, offsets=np.array([0, 4, 2, 9]), loc=np.zeros((6, 2), dtype=np.int64),
               prices_ld=0)
    with pytest.raises(ValueError, match=r"^problem 1: offsets\[1\] \.\. offsets\[2\] = 4 \.\. 2 is not a slice of the 6 packed "
                                         r"entries \(0 <= start <= end <= nnz, fewer than 2\^31 - 1 entries\)$"):
        raise_for_status(res)
    res["status"] = np.array([0, 0, 7], dtype=np.int32)
    with pytest.raises(ValueError, match=r"^problem 2: offsets\[2\] \.\. offsets\[3\] = 2 \.\. 9 is not a slice of the 6"):
        raise_for_status(dict(res, outside_prices=None))
    ok = dict(res, outside_prices=None, offsets=np.array([0, 2, 4, 6]), sizes=np.array([[0, 2], [0, 2], [0, -5]]))
    with pytest.raises(ValueError, match=r"^problem 2: sizes\[2, 1\] = -5: at least 1"):
        raise_for_status(ok)
