"""Many small dense assignment problems in one call (misslap_solve_dense_batch, include/misslap.h).

No counterpart in the reference, whose own benchmark solves small dense matrices one at a time
(benchmarking.py:146).  Problem b of a (B, N, M) stack is solved by one workgroup of one launch, and its result is
exactly what `auction_solve(mat=mats[b, :n_b, :m_b], ...)` returns (csrc/kernels_batch_solve.hpp,
csrc/kernels_dense_batch.hpp).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._batch import _check_shapes, _check_stack, _decode_meta, _new_meta, _solve_options, _starting_prices

MAX_DIM = _lib.DENSE_BATCH_MAX_DIM


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
    if N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"problems of {N} x {M}: auction_solve_batch takes at most {MAX_DIM} x {MAX_DIM} "
                         f"(MISSLAP_DENSE_BATCH_MAX_DIM); solve larger problems with from_matrix / solve_batch")
    shp = _check_shapes(shapes, B, N, M, "problem")
    ns = shp[:, 0] if shp is not None else np.full(B, N, dtype=np.int32)
    e = float(eps_start)
    if e != e:
        raise ValueError("eps_start is NaN")
    p, p_ptr, _ = _starting_prices(prices, B, M, True, on_device, mats, "mats")
    keep = [p]  # buffers that must live through the call
    eps_b = None
    if fast:  # auction_.pyx:568-569: eps_start = 1 / N of each problem, as a C float
        eps_b = (1.0 / ns.astype(np.float64)).astype(np.float32)
    opts = _solve_options(on_device, mats, problem, e, max_iter)
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
    metas, info = _new_meta(B)
    _lib.check(_lib.load().misslap_solve_dense_batch(
        B, N, M, C.c_void_p(mat_ptr), None if shp is None else shp.ctypes.data,
        None if eps_b is None else eps_b.ctypes.data, None if p_ptr is None else C.c_void_p(p_ptr),
        1 if cardinality_check else 0, C.byref(opts), C.c_void_p(sol_ptr), C.c_void_p(pout_ptr),
        1 if on_device else 0, metas, C.byref(info)))
    return dict(sol=sol, prices=pout, meta=_decode_meta(metas, info))
