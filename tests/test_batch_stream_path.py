"""The call path the six "verdict per problem, stream-ordered" batch entry points share (batch_stream_call,
csrc/abi_batch_stream.hpp), where the Python front ends never go: a meta array of the shortest stride, optional outputs
left out, the stream-ordered mode on a side stream against the library's own mode, and the workspace checks.

Every case runs for misslap_solve_dense_batch_status, misslap_solve_dense_batch_outside,
misslap_solve_sparse_batch_status, misslap_solve_sparse_batch_outside, misslap_solve_ell_batch and
misslap_solve_ell_batch_outside through ctypes, on three tiny problems (3 rows, 4 columns; problem 1 uses 2 rows) of
small distinct integers; the sparse calls take the ELL call's problems as loc / val.  What is expected comes from the
Python front end of the same entry point on the same input, which is tested against the oracle elsewhere -- and which
must give on device tensors, bit for bit, what it gives on the host arrays.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from sslap_amd import (_lib, auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch, batch_meta_to_host,
                       ell_to_packed)
from tests._batch_shapes import bits

B, N, M, K = 3, 3, 4, 3  # M: the dense stack's columns and the ELL / sparse calls' Mmax
GUARD = 0xA5
RECORD = C.sizeof(_lib.DenseBatchMeta)
PREFIX = _lib.DenseBatchMeta.its.offset  # the shortest stride the library takes: struct_size, n_rows, n_cols, eCE, nnz

MATS = ((np.arange(B * N * M) * 5) % (B * N * M) + 1).astype(np.float64).reshape(B, N, M)
SHAPES = np.array([[3, 4], [2, 3], [3, 4]], dtype=np.int32)
COLS = np.array([[[0, 1, 2], [1, 2, 3], [0, 2, 3]],
                 [[0, 1, -1], [1, 3, -1], [0, 1, 2]],
                 [[3, 0, -1], [0, 1, 2], [2, 3, 1]]], dtype=np.int32)
VALS = ((np.arange(B * N * K) * 7) % (B * N * K) + 1).astype(np.float64).reshape(B, N, K)
ROWS = np.array([3, 2, 3], dtype=np.int32)
OUTSIDE = np.array([[2., 9., 4.], [7., 3., 8.], [5., 6., 1.]])
_PACKED = ell_to_packed(COLS, VALS, ROWS)
LOC = np.ascontiguousarray(np.concatenate([l for l, _ in _PACKED]), dtype=np.int32)
VAL = np.ascontiguousarray(np.concatenate([v for _, v in _PACKED]), dtype=np.float64)
OFFSETS = np.concatenate([[0], np.cumsum([len(v) for _, v in _PACKED])]).astype(np.int64)
NNZ = int(OFFSETS[-1])

NAMES = ("dense_status", "dense_outside", "sparse_status", "sparse_outside", "ell", "ell_outside")
ENTRY = dict(dense_status="misslap_solve_dense_batch_status", dense_outside="misslap_solve_dense_batch_outside",
             sparse_status="misslap_solve_sparse_batch_status", sparse_outside="misslap_solve_sparse_batch_outside",
             ell="misslap_solve_ell_batch", ell_outside="misslap_solve_ell_batch_outside")
SIZING = dict(dense_status=("misslap_dense_batch_workspace_bytes", (B, N, M, 0, 1)),
              dense_outside=("misslap_dense_batch_outside_workspace_bytes", (B, N, M, 0)),
              sparse_status=("misslap_sparse_batch_workspace_bytes", (B, NNZ, 0, 1)),
              sparse_outside=("misslap_sparse_batch_outside_workspace_bytes", (B, N, M, 0)),
              ell=("misslap_ell_batch_workspace_bytes", (B, N, K, 0, 1)),
              ell_outside=("misslap_ell_batch_outside_workspace_bytes", (B, N, K, M, 0)))
# the arrays a call reads with the input (on the host, or as device tensors in the stream-ordered mode); the sparse
# calls' offsets are read on the host in both modes, and a second time on the device with a workspace
INPUTS = dict(dense_status=dict(mat=MATS, shapes=SHAPES), dense_outside=dict(mat=MATS, shapes=SHAPES, outside=OUTSIDE),
              sparse_status=dict(loc=LOC, val=VAL, offsets_dev=OFFSETS),
              sparse_outside=dict(loc=LOC, val=VAL, offsets_dev=OFFSETS, outside=OUTSIDE),
              ell=dict(cols=COLS, vals=VALS, rows=ROWS), ell_outside=dict(cols=COLS, vals=VALS, rows=ROWS, outside=OUTSIDE))


def front_end(name, a=None):
    """The status-mode result of the entry point's Python front end (fast, guard on where there is one) on the host
    input, or on `a`: INPUTS[name] as device tensors (the front end sends the sparse calls' offsets itself)."""
    a = INPUTS[name] if a is None else a
    kw = dict(fast=True, errors="status")
    if "outside" in a:
        kw["outside"] = a["outside"]
    if name.startswith("dense"):
        return auction_solve_batch(a["mat"], shapes=a["shapes"], **kw)
    if name.startswith("sparse"):
        return auction_solve_sparse_batch(a["loc"], a["val"], OFFSETS, dims=(N, M), **kw)
    return auction_solve_ell_batch(a["cols"], a["vals"], rows=a["rows"], n_cols=M, **kw)


def options(on_device):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 1000000
    o.input_on_device = 1 if on_device else 0
    return o


def ptr(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def solve(lib, name, a, opts, stream, work, nwork, out, on_device):
    """One call of the entry point: a the input arrays (INPUTS[name], or device copies), out the output arrays by the
    header's names (a missing key is a null pointer), info a DenseBatchInfo or missing."""
    a = {k: ptr(v) for k, v in a.items()}
    o = {k: ptr(out.get(k)) for k in ("sol", "prices_out", "outside_prices_out", "status", "matching_size", "meta")}
    info = C.byref(out["info"]) if out.get("info") is not None else None
    tail = (on_device, o["status"], o["matching_size"], o["meta"], info)
    way = (C.byref(opts), stream, ptr(work), nwork)
    if name == "dense_status":
        args = (B, N, M, a["mat"], a["shapes"], 1, None, 1) + way + (o["sol"], o["prices_out"]) + tail
    elif name == "dense_outside":
        args = (B, N, M, a["mat"], a["shapes"], 1, None) + way + (a["outside"], N, o["sol"], o["prices_out"],
                                                                     o["outside_prices_out"]) + tail
    elif name == "sparse_status":
        args = (B, a["loc"], a["val"], OFFSETS.ctypes.data, a["offsets_dev"], None, 1, None, 0, 1) + way + (
            N, M, o["sol"], o["prices_out"]) + tail
    elif name == "sparse_outside":
        args = (B, a["loc"], a["val"], OFFSETS.ctypes.data, a["offsets_dev"], None, 1, None, 0) + way + (
            N, M, a["outside"], N, o["sol"], o["prices_out"], o["outside_prices_out"]) + tail
    elif name == "ell":
        args = (B, N, K, a["cols"], 0, a["vals"], a["rows"], 1, None, 0, 1) + way + (M, o["sol"], o["prices_out"]) + tail
    else:
        args = (B, N, K, a["cols"], 0, a["vals"], a["rows"], 1, None, 0) + way + (
            M, a["outside"], N, o["sol"], o["prices_out"], o["outside_prices_out"]) + tail
    return getattr(lib, ENTRY[name])(*args)


def host_outputs(name, with_optional=True):
    out = dict(sol=np.full((B, N), -7, dtype=np.int32), status=np.full(B, -7, dtype=np.int32))
    if with_optional:
        out.update(matching_size=np.full(B, -7, dtype=np.int32), prices_out=np.full((B, M), -7.0), info=_lib.DenseBatchInfo())
        if name.endswith("outside"):
            out["outside_prices_out"] = np.full((B, N), -7.0)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    return front_end(name)


@functools.lru_cache(maxsize=None)
def short_stride_run(name):
    """The library's own mode with meta records of PREFIX bytes each, in a buffer of guard bytes."""
    lib = _lib.load()
    out = host_outputs(name)
    buf = np.full(B * PREFIX + 2 * RECORD, GUARD, dtype=np.uint8)
    buf[:4].view(np.int32)[0] = PREFIX
    out["meta"] = buf
    _lib.check(solve(lib, name, INPUTS[name], options(False), None, None, 0, out, 0))
    return out


def assert_outputs(name, got, want):
    assert np.array_equal(got["sol"], want["sol"]) and np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["matching_size"], want["matching_size"])
    assert np.array_equal(bits(got["prices_out"]), bits(want["prices"]))
    if name.endswith("outside"):
        assert np.array_equal(bits(got["outside_prices_out"]), bits(want["outside_prices"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_mode_with_the_shortest_meta_stride(gpu_lib, name):
    got, want = short_stride_run(name), expected(name)
    assert (want["status"] == 0).all()  # every problem is solved: the outputs below are results, not fills
    assert_outputs(name, got, want)
    buf = got["meta"]
    assert (buf[B * PREFIX:] == GUARD).all()  # nothing behind the accepted prefix of any record
    rec = buf[:B * PREFIX].reshape(B, PREFIX)
    assert (rec[:, :4].copy().view(np.int32)[:, 0] == PREFIX).all()  # struct_size: the caller's, in every record
    for k, field in enumerate(("n_rows", "n_cols", "eCE")):
        assert np.array_equal(rec[:, 4 + 4 * k:8 + 4 * k].copy().view(np.int32)[:, 0], want["meta"][field]), field
    assert np.array_equal(rec[:, 16:24].copy().view(np.int64)[:, 0], want["meta"]["nnz"])
    assert got["info"].threads == want["meta"]["gpu"]["threads"] and got["info"].lds_bytes == want["meta"]["gpu"]["lds_bytes"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_host_mode_without_the_optional_outputs(gpu_lib, name):
    out = host_outputs(name, with_optional=False)  # no matching_size, prices_out, outside_prices_out, meta, info
    _lib.check(solve(gpu_lib, name, INPUTS[name], options(False), None, None, 0, out, 0))
    first = short_stride_run(name)
    assert np.array_equal(out["sol"], first["sol"]) and np.array_equal(out["status"], first["status"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_stream_ordered_mode_is_the_host_mode_bit_for_bit(gpu_lib, name):
    import torch
    host = host_outputs(name)
    host["meta"] = np.zeros(B * RECORD, dtype=np.uint8)
    host["meta"][:4].view(np.int32)[0] = RECORD
    _lib.check(solve(gpu_lib, name, INPUTS[name], options(False), None, None, 0, host, 0))

    dev = torch.device("cuda", 0)
    a = {k: torch.from_numpy(v).to(dev) for k, v in INPUTS[name].items()}
    sizing, dims = SIZING[name]
    nbytes = int(getattr(gpu_lib, sizing)(*dims))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # exactly the bytes the sizing function names
    assert nbytes > 0 and work.data_ptr() % 256 == 0
    out = dict(sol=torch.full((B, N), -7, dtype=torch.int32, device=dev), status=torch.full((B,), -7, dtype=torch.int32, device=dev),
               matching_size=torch.full((B,), -7, dtype=torch.int32, device=dev),
               prices_out=torch.full((B, M), -7.0, dtype=torch.float64, device=dev),
               meta=torch.zeros(B * RECORD, dtype=torch.uint8, device=dev), info=_lib.DenseBatchInfo())
    if name.endswith("outside"):
        out["outside_prices_out"] = torch.full((B, N), -7.0, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))  # (the fills above)
    _lib.check(solve(gpu_lib, name, a, options(True), C.c_void_p(int(side.cuda_stream)), work, nbytes, out, 1))
    side.synchronize()
    for key in ("sol", "status", "matching_size", "meta"):
        assert np.array_equal(out[key].cpu().numpy(), host[key]), key
    for key in ("prices_out", "outside_prices_out")[:2 if name.endswith("outside") else 1]:
        assert np.array_equal(bits(out[key].cpu().numpy()), bits(host[key])), key
    assert (out["info"].threads, out["info"].lds_bytes) == (host["info"].threads, host["info"].lds_bytes)
    assert out["info"].threads == 256 and out["info"].wall_ms == 0  # nothing is waited for, nothing is timed


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_front_end_on_device_tensors_is_the_front_end_on_host_arrays(gpu_lib, name):
    import torch
    dev = torch.device("cuda", 0)
    want = expected(name)
    got = front_end(name, {k: torch.from_numpy(v).to(dev) for k, v in INPUTS[name].items() if k != "offsets_dev"})
    assert set(got) == set(want) | {"records", "info", "stream", "keep"}
    assert ("outside_prices" in want) == name.endswith("outside")
    got_meta = batch_meta_to_host(got)  # (waits for the call's stream)
    for key in ("sol", "status", "matching_size"):
        assert got[key].is_cuda and np.array_equal(got[key].cpu().numpy(), want[key]), key
    for key in ("prices", "outside_prices")[:2 if name.endswith("outside") else 1]:
        assert got[key].is_cuda and np.array_equal(bits(got[key].cpu().numpy()), bits(want[key])), key
    want_meta = batch_meta_to_host(want)
    assert want_meta is want["meta"] and set(got_meta) == set(want_meta)
    for key in set(want_meta) - {"timer", "gpu"}:  # length-B arrays, bit for bit
        assert got_meta[key].dtype == want_meta[key].dtype and got_meta[key].tobytes() == want_meta[key].tobytes(), key
    untimed = [k for k in want_meta["gpu"] if not k.endswith("_ms")]
    assert untimed and set(got_meta["gpu"]) == set(want_meta["gpu"])
    assert [got_meta["gpu"][k] for k in untimed] == [want_meta["gpu"][k] for k in untimed]


@pytest.mark.parametrize("name", NAMES)
def test_workspace_checks_name_the_sizing_function(built_lib, name):
    """Made before the device is touched: the input pointers are never followed."""
    sizing, dims = SIZING[name]
    need = int(getattr(built_lib, sizing)(*dims))
    assert need > 0 and need % 256 == 0
    out = host_outputs(name)
    out["meta"] = np.zeros(B * RECORD, dtype=np.uint8)
    err = built_lib.misslap_last_error
    for work, nwork in ((4096, need - 1), (4096 + 8, need), (4096 + 255, need + 4096)):
        assert solve(built_lib, name, INPUTS[name], options(True), None, work, nwork, out, 1) == _lib.ERR_INVALID
        text = err().decode()
        assert "workspace of %d bytes" % nwork in text and "%d bytes, 256-byte aligned (%s)" % (need, sizing) in text, text
    # the arrays come first: host input, host outputs or no meta array with a workspace
    for opts, on_device, meta in ((options(False), 1, out["meta"]), (options(True), 0, out["meta"]), (options(True), 1, None)):
        assert solve(built_lib, name, INPUTS[name], opts, None, 4096, need - 1, dict(out, meta=meta), on_device) == _lib.ERR_INVALID
        assert "with a workspace every array is on the device" in err().decode()
