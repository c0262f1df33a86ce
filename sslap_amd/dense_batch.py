"""Many small dense assignment problems in one call (misslap_solve_dense_batch, include/misslap.h).

No counterpart in the reference, whose own benchmark solves small dense matrices one at a time
(benchmarking.py:146).  Problem b of a (B, N, M) stack is solved by one workgroup of one launch, and its result is
exactly what `auction_solve(mat=mats[b, :n_b, :m_b], ...)` returns (csrc/kernels_dense_batch.hpp).
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .auction_solve import _ENV_DEVICE, _cname

MAX_DIM = _lib.DENSE_BATCH_MAX_DIM


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _check_stack(mats):
    """dtype / rank / cap of `mats` (numpy array or device tensor); returns (B, N, M, on_device)."""
    if isinstance(mats, np.ndarray):
        on_device = False
        if mats.ndim != 3:
            raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.ndim}")
        if mats.dtype != np.float64:
            raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(mats.dtype)}'")
    elif _is_device_tensor(mats):
        import torch
        on_device = True
        if mats.dim() != 3:
            raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.dim()}")
        if mats.dtype != torch.float64:
            raise ValueError(f"mats must be float64, got {mats.dtype}")
        if not mats.is_contiguous():
            raise ValueError("a device tensor must be contiguous (it is read in place)")
    else:
        raise TypeError("mats must be a numpy array or a contiguous tensor on the device")
    B, N, M = (int(d) for d in mats.shape)
    if B < 1 or N < 1 or M < 1:
        raise ValueError(f"empty stack of shape {(B, N, M)}")
    if N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"problems of {N} x {M}: auction_solve_batch takes at most {MAX_DIM} x {MAX_DIM} "
                         f"(MISSLAP_DENSE_BATCH_MAX_DIM); solve larger problems with from_matrix / solve_batch")
    return B, N, M, on_device


def _check_shapes(shapes, B, N, M):
    if shapes is None:
        return None
    s = np.asarray(shapes)
    if s.shape != (B, 2) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"shapes must be an integer array of shape ({B}, 2), got {s.dtype} {s.shape}")
    bad = (s[:, 0] < 1) | (s[:, 0] > N) | (s[:, 1] < 1) | (s[:, 1] > M)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"problem {b}: shape ({int(s[b, 0])}, {int(s[b, 1])}) outside 1 .. {N} x 1 .. {M}")
    return np.ascontiguousarray(s, dtype=np.int32)


def auction_solve_batch(mats, problem="min", eps_start=0., max_iter=1000000, fast=False, cardinality_check=True,
                        shapes=None, prices=None):
    """Solve B independent dense problems in one call, one workgroup per problem.

    mats: float64 (B, N, M), a numpy array or a contiguous tensor on the device (read in place, ordered behind
    torch.cuda.current_stream()); entries v >= 0 are edges, anything else (-1, NaN) is not.  shapes: optional int
    (B, 2); problem b is then mats[b, :n_b, :m_b].  prices: optional float64 (B, M) starting prices (of the maximised
    problem) as AuctionSolver.resolve takes them.  N, M <= MISSLAP_DENSE_BATCH_MAX_DIM.

    Returns dict(sol=int32 (B, N) with -1 beyond n_b, prices=float64 (B, M) with 0 beyond m_b, meta=dict of length-B
    arrays).  Device input gives device tensors for sol and prices.  All or nothing: a failing problem raises
    ValueError("problem <b>: <what from_matrix raises for that slice>") and nothing is solved.  The caller's arrays are
    never written.
    """
    B, N, M, on_device = _check_stack(mats)
    shp = _check_shapes(shapes, B, N, M)
    ns = shp[:, 0] if shp is not None else np.full(B, N, dtype=np.int32)
    e = float(eps_start)
    if e != e:
        raise ValueError("eps_start is NaN")
    keep = []  # buffers that must live through the call
    p_ptr = None
    if prices is not None:
        if isinstance(prices, np.ndarray):
            if prices.dtype != np.float64:
                raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(prices.dtype)}'")
            if tuple(prices.shape) != (B, M):
                raise ValueError(f"prices must have shape ({B}, {M}), got {tuple(prices.shape)}")
            if on_device:
                import torch
                p = torch.from_numpy(np.ascontiguousarray(prices)).to(mats.device)
                p_ptr = p.data_ptr()
            else:
                p = np.ascontiguousarray(prices)
                p_ptr = p.ctypes.data
        elif _is_device_tensor(prices):
            import torch
            if not on_device:
                raise TypeError("prices on the device need mats on the device")
            if prices.dtype != torch.float64:
                raise ValueError(f"prices must be float64, got {prices.dtype}")
            if tuple(prices.shape) != (B, M):
                raise ValueError(f"prices must have shape ({B}, {M}), got {tuple(prices.shape)}")
            p = prices.contiguous()
            p_ptr = p.data_ptr()
        else:
            raise TypeError("prices must be a numpy array or a tensor on the device")
        keep.append(p)
    eps_b = None
    if fast:  # auction_.pyx:568-569: eps_start = 1 / N of each problem, as a C float
        eps_b = (1.0 / ns.astype(np.float64)).astype(np.float32)
    stream = None
    if on_device:
        import torch
        stream = torch.cuda.current_stream(mats.device).cuda_stream
    # (no tuning knob applies to this path: only the fields the entry point reads are set)
    opts = _lib.Options()
    opts.struct_size = C.sizeof(_lib.Options)
    opts.device = int(os.environ.get(_ENV_DEVICE, 0))
    if on_device and mats.device.index is not None:
        opts.device = mats.device.index
    opts.maximize = 1 if problem != "min" else 0  # (every string other than 'min' is 'max', auction_.pyx:236)
    opts.eps_start = float(np.float32(e))
    opts.max_iter = int(max_iter)
    opts.input_on_device = 1 if on_device else 0
    opts.input_stream = None if stream is None else C.c_void_p(int(stream))
    if on_device:
        import torch
        sol = torch.empty((B, N), dtype=torch.int32, device=mats.device)
        pout = torch.empty((B, M), dtype=torch.float64, device=mats.device)
        sol_ptr, pout_ptr, mat_ptr = sol.data_ptr(), pout.data_ptr(), mats.data_ptr()
    else:
        mc = np.ascontiguousarray(mats)
        keep.append(mc)
        sol = np.empty((B, N), dtype=np.int32)
        pout = np.empty((B, M), dtype=np.float64)
        sol_ptr, pout_ptr, mat_ptr = sol.ctypes.data, pout.ctypes.data, mc.ctypes.data
    metas = (_lib.DenseBatchMeta * B)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)
    info = _lib.DenseBatchInfo()
    _lib.check(_lib.load().misslap_solve_dense_batch(
        B, N, M, C.c_void_p(mat_ptr), None if shp is None else shp.ctypes.data,
        None if eps_b is None else eps_b.ctypes.data, None if p_ptr is None else C.c_void_p(p_ptr),
        1 if cardinality_check else 0, C.byref(opts), C.c_void_p(sol_ptr), C.c_void_p(pout_ptr),
        1 if on_device else 0, metas, C.byref(info)))
    raw = np.ctypeslib.as_array(metas)  # structured view, one record per problem
    obj_f32 = raw["obj_f32"].astype(np.float32)
    start_f32, final_f32 = raw["start_eps"].astype(np.float32), raw["final_eps"].astype(np.float32)
    meta = dict(
        its=raw["its"].astype(np.int64), nreductions=raw["nreductions"].astype(np.int64), eCE=raw["eCE"].astype(np.int64),
        soln_found=raw["soln_found"].astype(np.int64), n_assigned=raw["n_assigned"].astype(np.int64),
        # rounded as the reference rounds them (auction_.pyx:264, :302-303: Python's round of the float)
        obj=np.array([round(float(x), 3) for x in obj_f32]), obj_f64=raw["obj_f64"].astype(np.float64),
        start_eps=np.array([round(float(x), 3) for x in start_f32]),
        final_eps=np.array([round(float(x), 3) for x in final_f32]),
        start_eps_f32=start_f32, final_eps_f32=final_f32, n_rows=raw["n_rows"].astype(np.int64),
        n_cols=raw["n_cols"].astype(np.int64), nnz=raw["nnz"].astype(np.int64), bids_made=raw["bids_made"].astype(np.int64),
    )
    meta["timer"] = {"solve": f"{info.wall_ms:.2f}ms"}
    meta["gpu"] = dict(threads=int(info.threads), lds_bytes=int(info.lds_bytes), check_ms=float(info.check_ms),
                       matching_ms=float(info.matching_ms), kernel_ms=float(info.solve_ms), wall_ms=float(info.wall_ms))
    return dict(sol=sol, prices=pout, meta=meta)
