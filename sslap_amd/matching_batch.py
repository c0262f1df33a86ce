"""Maximum matching of many small bipartite graphs in one call (misslap_matching_batch / misslap_matching_dense_batch,
include/misslap.h).

The batch form of `hopcroft_solve(loc=)` / `hopcroft_solve(mat=)`: graph b is matched by one workgroup of one launch,
and its result is exactly the reference's HopcroftKarpSolverCython.solve() on that graph -- the same size and the same
pairing arrays (csrc/kernels_matching_batch.hpp).  The reference has no counterpart; it matches one graph per call.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._batch import (_check_offsets, _check_shapes, _check_stack, _empty, _entries_flag, _is_device_tensor, _mat_dtype_name, _maxima,
                     _options, _ptr, _stack_strides)

MAX_DIM = _lib.MATCHING_BATCH_MAX_DIM


def _pack(locs):
    """A list of per-graph loc arrays -> (loc int32, offsets) on the host (cast to int32 as hopcroft_solve does)."""
    out = []
    for b, lb in enumerate(locs):
        if not isinstance(lb, np.ndarray):
            raise TypeError(f"graph {b}: loc must be a numpy array")
        if lb.ndim != 2 or lb.shape[1] != 2 or not np.issubdtype(lb.dtype, np.integer):
            raise ValueError(f"graph {b}: loc must be an integer array of shape (nnz, 2), got {lb.dtype} {lb.shape}")
        out.append(lb.astype(np.int32))
    if not out:
        raise ValueError("no graphs given")
    counts = np.array([x.shape[0] for x in out], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(out, axis=0).reshape(-1, 2), dtype=np.int32), offsets


def _check_loc(loc, offsets):
    """loc (numpy integer or device int32, (nnz, 2)) and host offsets; returns (loc, B, offsets int64, on_device)."""
    if isinstance(loc, np.ndarray):
        on_device = False
        if loc.ndim != 2 or loc.shape[1] != 2:
            raise ValueError(f"loc must have shape (nnz, 2), got {loc.shape}")
        if not np.issubdtype(loc.dtype, np.integer):
            raise ValueError(f"loc must be an integer array, got {loc.dtype}")
        loc = np.ascontiguousarray(loc, dtype=np.int32)
    elif _is_device_tensor(loc):
        import torch
        on_device = True
        if loc.dim() != 2 or loc.shape[1] != 2:
            raise ValueError(f"loc must have shape (nnz, 2), got {tuple(loc.shape)}")
        if loc.dtype != torch.int32:
            raise ValueError(f"loc must be int32, got {loc.dtype}")
        if not loc.is_contiguous():
            raise ValueError("a device tensor must be contiguous (it is read in place)")
    else:
        raise TypeError("loc must be a numpy array, a contiguous int32 tensor on the device or a list of numpy arrays")
    B, off = _check_offsets(offsets, int(loc.shape[0]),
                            "offsets is required with a packed loc (a list of per-graph loc arrays needs none)")
    return loc, B, off, on_device


def _check_mats(mats, shapes, mat_dtype):
    """mats (numpy or device, (B, N, M) of mat_dtype) and optional shapes; returns (B, N, M, shapes int32 or None,
    on_device, the MISSLAP_DTYPE_* code)."""
    B, N, M, on_device, dtype = _check_stack(mats, mat_dtype)
    if shapes is None:
        if N > MAX_DIM or M > MAX_DIM:
            raise ValueError(f"graph 0: {N} x {M} exceeds MISSLAP_MATCHING_BATCH_MAX_DIM ({MAX_DIM})")
        return B, N, M, None, on_device, dtype
    s = _check_shapes(shapes, B, N, M, "graph")
    big = (s[:, 0] > MAX_DIM) | (s[:, 1] > MAX_DIM)
    if big.any():
        b = int(np.flatnonzero(big)[0])
        raise ValueError(f"graph {b}: {int(s[b, 0])} x {int(s[b, 1])} exceeds MISSLAP_MATCHING_BATCH_MAX_DIM ({MAX_DIM})")
    return B, N, M, s, on_device, dtype


def hopcroft_solve_batch(loc=None, offsets=None, mats=None, shapes=None, mat_dtype="float64", entries="nonneg"):
    """Maximum matching of B small bipartite graphs in one call, one workgroup per graph.

    Exactly ONE of
    loc:  a packed integer (nnz, 2) array of edges (i, j), numpy or a contiguous int32 tensor on the device (read in
          place, ordered behind torch.cuda.current_stream()); graph b is the entries offsets[b]:offsets[b + 1] (a host
          integer array of length B + 1), rows ascending, n_b = max row + 1 and m_b = max column + 1 of the graph.  Or a
          list of per-graph loc numpy arrays, with offsets None.
    mats: a float64 (B, N, M) stack, numpy or a device tensor of any non-negative strides (a transposed view, a slice,
          an expanded matrix: read where it lies, misslap_matching_dense_batch_strided; the pairings are those of
          mats.contiguous()); graph b is mats[b, :n_b, :m_b] with
          (n_b, m_b) = shapes[b] (optional integer (B, 2); default N x M), edge (i, j) iff the entry is >= 0.
          mat_dtype ("float64", "float32", "float16", "bfloat16", or that numpy / torch dtype) names the stack's element
          type, which it must have exactly; the stack is read in place and the pairings are those of the widened stack.
          entries="finite" (default "nonneg", the rule above): edge (i, j) iff the entry is not a NaN, the rule of
          auction_solve_batch(entries="finite"); the pairings are those of hopcroft_solve(loc=loc_b) on the graph
          dense_to_packed(mats, shapes, "finite") gives.
    A graph has at most MISSLAP_MATCHING_BATCH_MAX_DIM rows and columns.

    Returns dict(size=int32 (B,), left_pairings=int32 (B, Nmax), right_pairings=int32 (B, Mmax), n_rows, n_cols);
    row b equals hopcroft_solve(loc=loc_b) / hopcroft_solve(mat=mats[b, :n_b, :m_b]) on [:n_b] / [:m_b], -1 beyond.
    Device input gives device tensors for the pairings.  All or nothing: a failing graph raises
    ValueError("graph <b>: ...") and nothing is matched.  The caller's arrays are never written.
    """
    if (loc is None) == (mats is None):
        raise ValueError("exactly one of loc and mats must be given")
    flag = _entries_flag(entries)
    if mats is not None:
        if offsets is not None:
            raise TypeError("offsets goes with loc, not with mats")
        B, N, M, shp, on_device, dtype = _check_mats(mats, shapes, mat_dtype)
        Nmax = int(shp[:, 0].max()) if shp is not None else N
        Mmax = int(shp[:, 1].max()) if shp is not None else M
        src = mats
    else:
        if shapes is not None:
            raise TypeError("shapes goes with mats, not with loc")
        if _mat_dtype_name(mat_dtype) != "float64":
            raise TypeError("mat_dtype goes with mats, not with loc")
        if flag:
            raise TypeError("entries goes with mats, not with loc")
        if isinstance(loc, (list, tuple)):
            if offsets is not None:
                raise TypeError("a list of per-graph loc arrays takes no offsets")
            loc, offsets = _pack(loc)
        loc, B, off, on_device = _check_loc(loc, offsets)
        max_row, max_col, _ = _maxima(loc, off, on_device, per_problem=False)
        Nmax = min(max(max_row + 1, 1), MAX_DIM)  # (a graph beyond the cap is rejected by the library, in its order)
        Mmax = min(max(max_col + 1, 1), MAX_DIM)
        src = loc
    opts = _options(on_device, src) if mats is None else _options(on_device, src, mat_dtype=dtype | flag)
    size = np.empty(B, dtype=np.int32)
    n_rows = np.empty(B, dtype=np.int32)
    n_cols = np.empty(B, dtype=np.int32)
    dev = src.device if on_device else None
    left, right = _empty((B, Nmax), np.int32, dev), _empty((B, Mmax), np.int32, dev)
    if not on_device:
        src = np.ascontiguousarray(src)
    info = _lib.MatchingBatchInfo()
    info.struct_size = C.sizeof(_lib.MatchingBatchInfo)
    outs = (size.ctypes.data, n_rows.ctypes.data, n_cols.ctypes.data, C.c_void_p(_ptr(left)), Nmax,
            C.c_void_p(_ptr(right)), Mmax, 1 if on_device else 0, C.byref(info))
    lib = _lib.load()
    if mats is not None:
        strides = _stack_strides(mats, on_device)
        ins = (C.c_void_p(_ptr(src)), _ptr(shp), C.byref(opts))
        if strides is None:
            _lib.check(lib.misslap_matching_dense_batch(B, N, M, *ins, *outs))
        else:
            _lib.check(lib.misslap_matching_dense_batch_strided(B, N, M, *strides, *ins, *outs))
    else:
        _lib.check(lib.misslap_matching_batch(B, C.c_void_p(_ptr(src)), off.ctypes.data, C.byref(opts), *outs))
    return dict(size=size, left_pairings=left, right_pairings=right, n_rows=n_rows, n_cols=n_cols,
                gpu=dict(threads=int(info.threads), lds_bytes=int(info.lds_bytes), check_ms=float(info.check_ms),
                         kernel_ms=float(info.kernel_ms), wall_ms=float(info.wall_ms)))
