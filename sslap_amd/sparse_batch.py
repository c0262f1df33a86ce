"""Many small sparse assignment problems in one call (misslap_solve_sparse_batch, include/misslap.h).

The batch form of `auction_solve(loc=, val=, size=)`: problem b of a packed (loc, val) is solved by one workgroup of one
launch, and its result is exactly what `from_sparse(loc_b, val_b, size=sizes[b], ...).solve()` returns
(csrc/kernels_batch_solve.hpp, csrc/kernels_sparse_batch.hpp).  The reference has no counterpart; it solves one
problem per AuctionSolver.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._batch import (_check_offsets, _decode_meta, _is_device_tensor, _maxima, _new_meta, _solve_options,
                     _starting_prices)
from .auction_solve import _cname

MAX_DIM = _lib.SPARSE_BATCH_MAX_DIM


def _pack(pairs):
    """A list of per-problem (loc_b, val_b) -> (loc, val, offsets) on the host (loc cast to int32 as from_sparse does)."""
    locs, vals = [], []
    for b, pair in enumerate(pairs):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise TypeError(f"problem {b}: expected a (loc, val) pair")
        lb, vb = pair
        if not isinstance(lb, np.ndarray) or not isinstance(vb, np.ndarray):
            raise TypeError(f"problem {b}: loc and val must be numpy arrays")
        if lb.ndim != 2 or lb.shape[1] != 2 or not np.issubdtype(lb.dtype, np.integer):
            raise ValueError(f"problem {b}: loc must be an integer array of shape (nnz, 2), got {lb.dtype} {lb.shape}")
        if vb.dtype != np.float64:
            raise ValueError(f"problem {b}: Buffer dtype mismatch, expected 'DTYPE_t' but got '{_cname(vb.dtype)}'")
        if vb.ndim != 1 or vb.shape[0] != lb.shape[0]:
            raise ValueError(f"problem {b}: val must have shape ({lb.shape[0]},), got {vb.shape}")
        locs.append(lb.astype(np.int32))  # :601
        vals.append(vb)
    if not locs:
        raise ValueError("no problems given")
    counts = np.array([x.shape[0] for x in locs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    loc = np.ascontiguousarray(np.concatenate(locs, axis=0).reshape(-1, 2), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate(vals), dtype=np.float64)
    return loc, val, offsets


def _check_input(loc, val, offsets):
    """dtype / shape / device of loc and val, offsets against them; returns (B, nnz, offsets int64, on_device)."""
    if isinstance(loc, np.ndarray) and isinstance(val, np.ndarray):
        on_device = False
        if loc.ndim != 2 or loc.shape[1] != 2:
            raise ValueError(f"loc must have shape (nnz, 2), got {loc.shape}")
        if loc.dtype != np.int32:
            raise ValueError(f"loc must be int32, got {loc.dtype}")
        if val.ndim != 1:
            raise ValueError(f"val must have 1 dimension, got {val.ndim}")
        if val.dtype != np.float64:
            raise ValueError(f"Buffer dtype mismatch, expected 'DTYPE_t' but got '{_cname(val.dtype)}'")
    elif _is_device_tensor(loc) and _is_device_tensor(val):
        import torch
        on_device = True
        if loc.dim() != 2 or loc.shape[1] != 2:
            raise ValueError(f"loc must have shape (nnz, 2), got {tuple(loc.shape)}")
        if loc.dtype != torch.int32:
            raise ValueError(f"loc must be int32, got {loc.dtype}")
        if val.dim() != 1:
            raise ValueError(f"val must have 1 dimension, got {val.dim()}")
        if val.dtype != torch.float64:
            raise ValueError(f"val must be float64, got {val.dtype}")
        if not loc.is_contiguous() or not val.is_contiguous():
            raise ValueError("device tensors must be contiguous (they are read in place)")
        if loc.device != val.device:
            raise ValueError(f"loc is on {loc.device}, val on {val.device}")
    else:
        raise TypeError("loc and val must both be numpy arrays or both tensors on the device")
    nnz = int(loc.shape[0])
    if int(val.shape[0]) != nnz:
        raise ValueError(f"loc holds {nnz} entries, val {int(val.shape[0])}")
    B, off = _check_offsets(offsets, nnz, "offsets is required with packed loc / val (a list of (loc, val) pairs needs "
                                          "none)")
    return B, nnz, off, on_device


def _check_sizes(sizes, B):
    if sizes is None:
        return None
    s = np.asarray(sizes)
    if s.shape != (B, 2) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"sizes must be an integer array of shape ({B}, 2), got {s.dtype} {s.shape}")
    return np.ascontiguousarray(s, dtype=np.int64)


def auction_solve_sparse_batch(loc, val=None, offsets=None, problem="min", eps_start=0., max_iter=1000000, fast=False,
                               sizes=None, cardinality_check=True, prices=None):
    """Solve B independent sparse problems in one call, one workgroup per problem.

    loc: int32 (nnz, 2) and val: float64 (nnz,), both numpy arrays or both contiguous tensors on the device (read in place,
    ordered behind torch.cuda.current_stream()); problem b is the entries offsets[b]:offsets[b + 1] (a host integer array
    of length B + 1), its row and column indices its own and 0-based, rows ascending as from_sparse requires.  Or `loc` is
    a list of per-problem (loc_b, val_b) pairs and val / offsets are None.  sizes: optional int (B, 2), row b what
    from_sparse's `size=` is for problem b.  prices: optional float64 (B, P), P >= every problem's n_cols, starting prices
    (of the maximised problem) as AuctionSolver.resolve takes them.  A problem has at most MISSLAP_SPARSE_BATCH_MAX_DIM
    rows and columns.

    Returns dict(sol=int32 (B, Nmax) with -1 beyond n_b, prices=float64 (B, Mmax) with 0 beyond n_cols_b, meta=dict of
    length-B arrays); Nmax / Mmax are the largest n_b / n_cols.  Device input gives device tensors for sol and prices.
    All or nothing: a failing problem raises ValueError("problem <b>: <what from_sparse raises for it>") and nothing is
    solved.  The one check made before the call is `fast` with N_b = 0 (ZeroDivisionError, as from_sparse raises it).
    The caller's arrays are never written, problem='min' included.
    """
    if isinstance(loc, (list, tuple)):
        if val is not None or offsets is not None:
            raise TypeError("a list of (loc, val) pairs takes no val / offsets; packed loc and val are numpy arrays or "
                            "device tensors")
        loc, val, offsets = _pack(loc)
    B, nnz, off, on_device = _check_input(loc, val, offsets)
    szs = _check_sizes(sizes, B)
    e = float(eps_start)
    if e != e:
        raise ValueError("eps_start is NaN")
    max_row, max_col, rows = _maxima(loc, off, on_device, per_problem=fast and szs is None)
    Nmax = min(max(max_row + 1, 1), MAX_DIM)  # (a problem beyond the cap is rejected by the library, in its order)
    Mmax = min(max(max_col + 1, 1), MAX_DIM)
    p, p_ptr, p_ld = _starting_prices(prices, B, Mmax, False, on_device, loc, "loc / val")
    if _is_device_tensor(prices) and prices.device != loc.device:
        raise ValueError(f"prices are on {prices.device}, loc on {loc.device}")
    keep = [p]  # buffers that must live through the call
    eps_b = None
    if fast:  # auction_.pyx:614-615: eps_start = 1 / N of each problem (from_sparse's N: size[1], or the max row)
        N = szs[:, 1] if szs is not None else rows
        nonempty = np.diff(off) > 0  # (an empty problem is reported by the library: "no entries")
        zero = nonempty & (N == 0)
        if zero.any():
            raise ZeroDivisionError(f"problem {int(np.flatnonzero(zero)[0])}: division by zero")
        Nf = np.where(nonempty, N, 1).astype(np.float64)
        eps_b = np.ascontiguousarray((1.0 / Nf).astype(np.float32))
    opts = _solve_options(on_device, loc, problem, e, max_iter)
    if on_device:
        import torch
        sol = torch.empty((B, Nmax), dtype=torch.int32, device=loc.device)
        pout = torch.empty((B, Mmax), dtype=torch.float64, device=loc.device)
        sol_ptr, pout_ptr, loc_ptr, val_ptr = sol.data_ptr(), pout.data_ptr(), loc.data_ptr(), val.data_ptr()
    else:
        lc, vc = np.ascontiguousarray(loc), np.ascontiguousarray(val)
        keep += [lc, vc]
        sol = np.empty((B, Nmax), dtype=np.int32)
        pout = np.empty((B, Mmax), dtype=np.float64)
        sol_ptr, pout_ptr, loc_ptr, val_ptr = sol.ctypes.data, pout.ctypes.data, lc.ctypes.data, vc.ctypes.data
    metas, info = _new_meta(B)
    _lib.check(_lib.load().misslap_solve_sparse_batch(
        B, C.c_void_p(loc_ptr), C.c_void_p(val_ptr), off.ctypes.data, None if szs is None else szs.ctypes.data,
        None if eps_b is None else eps_b.ctypes.data, None if p_ptr is None else C.c_void_p(p_ptr), p_ld,
        1 if cardinality_check else 0, C.byref(opts), C.c_void_p(sol_ptr), Nmax, C.c_void_p(pout_ptr), Mmax,
        1 if on_device else 0, metas, C.byref(info)))
    return dict(sol=sol, prices=pout, meta=_decode_meta(metas, info))
