"""Typed dense stacks without a GPU: misslap_options.mat_dtype sits where the header says and moves nothing, the three
entry points that read it validate it before they touch a device, every other entry point takes float64 only, and the
Python keyword checks the stack's dtype before any call into the library."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, hopcroft_solve_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_field_matches_the_header_and_moves_nothing():
    """Compile a tiny C program against the header (strict C99 and C11) and compare sizeof / offsetof with ctypes."""
    fields = ["struct_size", "max_iter", "rounds_per_sync", "cand_refresh_min", "mat_dtype", "reserved", "input_stream"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "misslap.h"', 'int main(void){',
            'printf("sizeof %zu\\n", sizeof(misslap_options));']
    prog += [f'printf("{f} %zu\\n", offsetof(misslap_options, {f}));' for f in fields]
    prog += ['printf("F64 %d\\nF32 %d\\nF16 %d\\nBF16 %d\\n", MISSLAP_DTYPE_F64, MISSLAP_DTYPE_F32, MISSLAP_DTYPE_F16, '
             'MISSLAP_DTYPE_BF16);', "return 0;}"]
    for std in ("c99", "c11"):
        with tempfile.TemporaryDirectory() as d:
            src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
            open(src, "w").write("\n".join(prog))
            subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I",
                                   os.path.join(ROOT, "include"), src, "-o", exe])
            out = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines())}
        assert out["sizeof"] == C.sizeof(_lib.Options) == 128
        for f in fields:
            assert out[f] == getattr(_lib.Options, f).offset, (std, f)
        # the first word of what was reserved[7]: right behind the version-1 struct's 88 bytes, nothing after it moved
        assert out["mat_dtype"] == 88 and out["input_stream"] == 120
        assert (out["F64"], out["F32"], out["F16"], out["BF16"]) == (0, 1, 2, 3)
        assert (_lib.DTYPE_F64, _lib.DTYPE_F32, _lib.DTYPE_F16, _lib.DTYPE_BF16) == (0, 1, 2, 3)
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    assert re.search(r"#define MISSLAP_ABI_VERSION 2\b", header)
    assert [n for n, _ in _lib.Options._fields_[:12]][-1] == "rounds_per_sync"  # (what an ABI-1 struct is built from)
    o = _lib.Options(mat_dtype=3)
    assert o.reserved[0] == 3 and len(o.reserved) == 7


def _opts(**kw):
    o = _lib.Options(struct_size=C.sizeof(_lib.Options), max_iter=10)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class _Calls:
    """The three entry points that read mat_dtype, on a 1 x 2 x 2 stack of two-byte-or-wider elements."""

    def __init__(self, lib):
        self.lib = lib
        self.m = np.ones((1, 2, 2))  # 32 bytes: enough for any element type
        self.sol = np.empty((1, 2), dtype=np.int32)
        self.i = [np.empty(1, dtype=np.int32) for _ in range(3)]

    def solve(self, o):
        return self.lib.misslap_solve_dense_batch(1, 2, 2, self.m.ctypes.data, None, None, None, 0, C.byref(o),
                                                  self.sol.ctypes.data, None, 0, None, None)

    def status(self, o):
        return self.lib.misslap_solve_dense_batch_status(1, 2, 2, self.m.ctypes.data, None, 0, None, 0, C.byref(o), None,
                                                         None, 0, self.sol.ctypes.data, None, 0, self.i[0].ctypes.data,
                                                         None, None, None)

    def matching(self, o):
        return self.lib.misslap_matching_dense_batch(1, 2, 2, self.m.ctypes.data, None, C.byref(o), self.i[0].ctypes.data,
                                                     self.i[1].ctypes.data, self.i[2].ctypes.data, None, 0, None, 0, 0, None)


@pytest.mark.parametrize("entry", ["solve", "status", "matching"])
def test_mat_dtype_is_validated_before_any_device(built_lib, entry):
    call = getattr(_Calls(built_lib), entry)
    for bad in (4, -1):
        assert call(_opts(mat_dtype=bad)) == _lib.ERR_INVALID
        assert b"mat_dtype" in built_lib.misslap_last_error()
    # a valid type with otherwise valid arguments passes the validation: only the device is missing here
    for dt in (0, 1, 2, 3):
        rc = call(_opts(mat_dtype=dt))
        assert rc in (0, _lib.ERR_NO_DEVICE), (dt, rc, built_lib.misslap_last_error())
    # the words behind it are still reserved
    o = _opts(mat_dtype=1)
    o.reserved[1] = 1
    assert call(o) == _lib.ERR_INVALID and b"reserved" in built_lib.misslap_last_error()
    # a shorter ABI-2 struct that ends before the field, and an ABI-1 struct, mean float64
    short = _opts()
    short.struct_size = _lib.Options.mat_dtype.offset + 4
    assert call(short) in (0, _lib.ERR_NO_DEVICE)

    class OptionsV1(C.Structure):
        _fields_ = _lib.Options._fields_[:12] + [("reserved", C.c_int32 * 8)]
    v1 = OptionsV1(struct_size=88, max_iter=10)
    buf = (C.c_char * 128)()
    C.memmove(buf, C.byref(v1), 88)
    assert call(C.cast(buf, C.POINTER(_lib.Options)).contents) in (0, _lib.ERR_NO_DEVICE)


def test_every_other_entry_point_takes_float64_only(built_lib):
    lib = built_lib
    o = _opts(mat_dtype=1, tail_threshold=-1)
    loc = np.array([[0, 0], [1, 1]], dtype=np.int32)
    val = np.array([1.0, 2.0])
    h = C.c_void_p()
    assert lib.misslap_create(C.byref(h), 2, loc.ctypes.data, val.ctypes.data, C.byref(o)) == _lib.ERR_INVALID
    msg = lib.misslap_last_error()
    assert b"float64 only" in msg and b"mat_dtype" in msg
    nnz = C.c_int64()
    assert lib.misslap_create_dense(C.byref(h), 2, 2, np.ones((2, 2)).ctypes.data, C.byref(o), C.byref(nnz)) == _lib.ERR_INVALID
    assert b"float64 only" in lib.misslap_last_error()

    o = _opts(mat_dtype=1)
    off = np.array([0, 2], dtype=np.int64)
    sol = np.empty((1, 2), dtype=np.int32)
    assert lib.misslap_solve_sparse_batch(1, loc.ctypes.data, val.ctypes.data, off.ctypes.data, None, None, None, 0, 0,
                                          C.byref(o), sol.ctypes.data, 2, None, 0, 0, None, None) == _lib.ERR_INVALID
    assert b"float64 only" in lib.misslap_last_error()
    status = np.empty(1, dtype=np.int32)
    assert lib.misslap_solve_sparse_batch_status(1, loc.ctypes.data, val.ctypes.data, off.ctypes.data, None, None, 0, None,
                                                 0, 0, C.byref(o), None, None, 0, 2, 2, sol.ctypes.data, None, 0,
                                                 status.ctypes.data, None, None, None) == _lib.ERR_INVALID
    assert b"float64 only" in lib.misslap_last_error()
    i = [np.empty(1, dtype=np.int32) for _ in range(3)]
    assert lib.misslap_matching_batch(1, loc.ctypes.data, off.ctypes.data, C.byref(o), i[0].ctypes.data, i[1].ctypes.data,
                                      i[2].ctypes.data, None, 0, None, 0, 0, None) == _lib.ERR_INVALID
    assert b"float64 only" in lib.misslap_last_error()
    # ... and with mat_dtype 0 the same calls pass this check
    o = _opts(tail_threshold=-1)
    rc = lib.misslap_create(C.byref(h), 2, loc.ctypes.data, val.ctypes.data, C.byref(o))
    assert rc in (0, _lib.ERR_NO_DEVICE)
    if rc == 0:
        lib.misslap_destroy(h)


class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


@pytest.mark.parametrize("mode", ["raise", "status"])
def test_keyword_is_checked_before_ffi(no_ffi, mode):
    ok = np.ones((2, 3, 4))
    kw = dict(errors=mode)
    for name, np_dtype in (("float32", np.float32), ("float16", np.float16), ("float64", np.float64)):
        for spelled in (name, np_dtype, np.dtype(np_dtype)):
            with pytest.raises(_NoFFI):  # a typed stack with its own name reaches the library
                auction_solve_batch(ok.astype(np_dtype), mat_dtype=spelled, **kw)
    with pytest.raises(ValueError, match="dtype"):  # the default keyword is float64, with the message it always had
        auction_solve_batch(ok.astype(np.float32), **kw)
    with pytest.raises(ValueError, match="Buffer dtype mismatch, expected 'double' but got 'float'"):
        auction_solve_batch(ok.astype(np.float32), **kw)
    with pytest.raises(ValueError, match="dtype.*float16.*float64"):  # nothing is converted: both types are named
        auction_solve_batch(ok, mat_dtype="float16", **kw)
    with pytest.raises(ValueError, match="dtype.*float32.*float16"):
        auction_solve_batch(ok.astype(np.float16), mat_dtype=np.float32, **kw)
    with pytest.raises(ValueError, match="bfloat16"):  # numpy has no bfloat16: such a stack is a device tensor
        auction_solve_batch(ok.astype(np.float32), mat_dtype="bfloat16", **kw)
    for bad in ("int32", np.int32, "double", None, 7):
        with pytest.raises(ValueError, match="mat_dtype"):
            auction_solve_batch(ok, mat_dtype=bad, **kw)
    with pytest.raises(_NoFFI):  # prices stay float64 whatever the stack's type
        auction_solve_batch(ok.astype(np.float32), mat_dtype="float32", prices=np.zeros((2, 4)), **kw)
    with pytest.raises(ValueError, match="dtype"):
        auction_solve_batch(ok.astype(np.float32), mat_dtype="float32", prices=np.zeros((2, 4), dtype=np.float32), **kw)


def test_torch_dtype_objects_name_the_type(no_ffi):
    torch = pytest.importorskip("torch")
    ok = np.ones((2, 3, 4), dtype=np.float32)
    with pytest.raises(_NoFFI):
        auction_solve_batch(ok, mat_dtype=torch.float32)
    with pytest.raises(ValueError, match="dtype.*float16.*float32"):
        auction_solve_batch(ok, mat_dtype=torch.half)
    with pytest.raises(ValueError, match="mat_dtype"):
        auction_solve_batch(ok, mat_dtype=torch.int32)


def test_matching_keyword_is_checked_before_ffi(no_ffi):
    ok = np.ones((2, 3, 4))
    with pytest.raises(_NoFFI):
        hopcroft_solve_batch(mats=ok.astype(np.float16), mat_dtype="float16")
    with pytest.raises(ValueError, match="dtype"):
        hopcroft_solve_batch(mats=ok.astype(np.float32))
    with pytest.raises(ValueError, match="dtype.*float32.*float64"):
        hopcroft_solve_batch(mats=ok, mat_dtype="float32")
    with pytest.raises(ValueError, match="mat_dtype"):
        hopcroft_solve_batch(mats=ok, mat_dtype="int32")
    with pytest.raises(TypeError, match="mat_dtype goes with mats"):
        hopcroft_solve_batch(loc=[np.array([[0, 0]])], mat_dtype="float32")


def test_the_options_carry_the_type(monkeypatch):
    """What reaches the library: the stack's own address and bytes, and mat_dtype in the options."""
    seen = {}

    class _Lib:
        def misslap_solve_dense_batch(self, B, N, M, mat, shapes, eps, p0, check, opts, *rest):
            o = C.cast(opts, C.POINTER(_lib.Options)).contents
            seen.update(mat=mat.value, dtype=o.mat_dtype, reserved=list(o.reserved)[1:])
            raise _NoFFI()

    monkeypatch.setattr(_lib, "load", lambda: _Lib())
    for code, np_dtype in ((0, np.float64), (1, np.float32), (2, np.float16)):
        m = np.ones((2, 3, 5), dtype=np_dtype)
        with pytest.raises(_NoFFI):
            auction_solve_batch(m, mat_dtype=np_dtype)
        assert seen == dict(mat=m.ctypes.data, dtype=code, reserved=[0] * 6)  # read in place: no converted copy
