"""Many small dense assignment problems between two point sets (misslap_solve_points_batch, include/misslap.h).

The costs are squared distances, c[b, i, j] = |x[b, i] - y[b, j]|^2, and the (B, N, M) stack is never stored: the
kernels form every cost they need from the coordinates (csrc/kernels_points_batch.hpp).  `points_to_dense` is the
definition: the result of problem b is bit for bit the dense batch's (`auction_solve_batch`) on the float64 stack it
returns.  Problems of up to 2048 x 2048 are taken, twice the dense batch's cap.

With `finish="reverse"` every solved problem gets the reverse-auction clean-up behind its forward solve, which makes a
warm start (`prices=` with `outside=`) optimal (misslap_points_batch_reverse_finish); `points_reverse_finish` is its
definition in numpy.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .auction_solve import _ENV_DEVICE
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_device_shapes, _check_outside, _check_shapes, _empty, _eps, _host,
                     _is_device_tensor, _ptr, _send, _solve_options, _starting_prices, batch_meta_to_host,
                     raise_for_status)
from .dense_batch import dense_reverse_finish

MAX_DIM = _lib.POINTS_BATCH_MAX_DIM
MAX_COORDS = _lib.POINTS_BATCH_MAX_COORDS

_STATUS_TEXT = {
    _lib.BATCH_STATUS_BAD_SHAPE: "shape ({n}, {m}) outside 1 .. {N} x 1 .. {M}",
    _lib.BATCH_STATUS_BAD_OUTSIDE: "the outside value of row {row} is {value!r}: it must be >= 0 (a negative value or a NaN "
                                   "would be an absent entry)",
    _lib.BATCH_STATUS_INFINITE_VALUE: "a cost |x_i - y_j|^2 is not finite (a NaN or an infinite coordinate, or an "
                                      "overflow){also}",
    _lib.BATCH_STATUS_INFEASIBLE: "Matrix is infeasible (Maximum matching possible only involves {card} out of {n} rows.)",
    _lib.BATCH_STATUS_PRICE_NOT_FINITE: "prices hold a NaN or an infinity",
    _lib.BATCH_STATUS_PRICE_NEGATIVE: "prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
}


def points_to_dense(x, y, shapes=None):
    """x (B, N, D) and y (B, M, D), float32 or float64, numpy arrays or tensors -> the float64 (B, N, M) cost stack of
    squared distances: the definition of auction_solve_points_batch.

        xw, yw = x, y widened to float64 (exact)
        d_k    = xw[b, i, k] - yw[b, j, k]                 k = 0 .. D - 1
        s_0    = d_0 * d_0
        s_k    = s_(k-1) + d_k * d_k
        c[b, i, j] = s_(D-1)

    Every one of the 3 D - 1 operations is a separately rounded IEEE float64 operation, in exactly this order: no fused
    multiply-add, no reassociation, no float32 arithmetic.  A cost is never negative and never -0.0 (a square of a
    float64 is neither); it is a NaN or +inf where a coordinate is a NaN or infinite or where the chain overflows.
    shapes: optional integer (B, 2); the elements beyond (n_b, m_b) of problem b are +inf.
    Problem b of auction_solve_points_batch(x, y, shapes=shapes, ...) with status 0 is bit for bit problem b of
    auction_solve_batch(points_to_dense(x, y, shapes), shapes=shapes, ..., errors="status", cardinality_check=False),
    or, with outside, of auction_solve_batch(points_to_dense(x, y, shapes), shapes=shapes, outside=outside, ...,
    errors="status")."""
    x = np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    y = np.asarray(y.cpu().numpy() if hasattr(y, "cpu") else y)
    if x.ndim != 3 or y.ndim != 3:
        raise ValueError(f"x and y must have 3 dimensions (B, N, D) and (B, M, D), got {x.ndim} and {y.ndim}")
    if x.dtype != y.dtype or x.dtype not in (np.float32, np.float64):
        raise ValueError(f"x and y must both be float32 or both float64, got {x.dtype.name} and {y.dtype.name}")
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2] or x.shape[2] < 1:
        raise ValueError(f"x {x.shape} and y {y.shape} must share B and D >= 1")
    B, N, D = x.shape
    M = y.shape[1]
    xw, yw = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = xw[:, :, None, 0] - yw[:, None, :, 0]
        c = d * d
        for k in range(1, D):
            d = xw[:, :, None, k] - yw[:, None, :, k]
            q = d * d
            c = c + q
    c = np.ascontiguousarray(c)
    if shapes is not None:
        shp = np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes)
        for b in range(B):
            n, m = (max(int(v), 0) for v in shp[b])
            c[b, n:, :] = np.inf
            c[b, :, m:] = np.inf
    return c


def points_reverse_finish(x, y, sol, prices, final_eps, problem="min", shapes=None, outside=None, outside_prices=None,
                          max_iter=1000000, run=None, trace=None):
    """The reverse-auction finish of auction_solve_points_batch(finish="reverse"), stated in numpy: its definition.

    It is dense_reverse_finish (whose docstring states the loop, the stall rule and the return keys) applied to
    points_to_dense(x, y, shapes): every finite squared distance is an entry under the "nonneg" rule, so a problem has
    no holes.  x (B, N, D) and y (B, M, D) as points_to_dense takes them; sol, prices, final_eps, problem, shapes,
    outside, outside_prices, max_iter, run and trace as dense_reverse_finish takes them.  numpy has no size cap.
    Returns dict(sol, prices, [outside_prices], obj_f64, obj_f32, eCE, reverse=dict(its, left), ran)."""
    return dense_reverse_finish(points_to_dense(x, y, shapes), sol, prices, final_eps, problem=problem, shapes=shapes,
                                outside=outside, outside_prices=outside_prices, entries="nonneg", max_iter=max_iter,
                                run=run, trace=trace)


def _check_points(x, y):
    """dtype / rank / device of x and y; returns (B, N, M, D, on_device, the MISSLAP_DTYPE_* of the coordinates)."""
    if isinstance(x, np.ndarray) and isinstance(y, np.ndarray):
        on_device = False
        names = (x.dtype.name, y.dtype.name)
        ndims = (x.ndim, y.ndim)
    elif _is_device_tensor(x) and _is_device_tensor(y):
        on_device = True
        names = (str(x.dtype).split(".")[-1], str(y.dtype).split(".")[-1])
        ndims = (x.dim(), y.dim())
    elif (isinstance(x, np.ndarray) or _is_device_tensor(x)) and (isinstance(y, np.ndarray) or _is_device_tensor(y)):
        raise TypeError("x and y must both be numpy arrays or both tensors on the device")
    else:
        raise TypeError("x and y must be numpy arrays or tensors on the device")
    if names[0] != names[1]:
        raise ValueError(f"x and y must have one dtype, got {names[0]} and {names[1]}")
    if names[0] not in ("float64", "float32"):
        raise ValueError(f"x and y must be float64 or float32, got {names[0]}")
    if ndims != (3, 3):
        raise ValueError(f"x and y must have 3 dimensions (B, N, D) and (B, M, D), got {ndims[0]} and {ndims[1]}")
    (B, N, D), (By, M, Dy) = (tuple(int(v) for v in a.shape) for a in (x, y))
    if B != By or D != Dy:
        raise ValueError(f"x has shape {(B, N, D)}, y {(By, M, Dy)}: B and D must agree")
    if B < 1 or N < 1 or M < 1 or D < 1:
        raise ValueError(f"empty point sets of shapes {(B, N, D)} and {(B, M, D)}")
    if D > MAX_COORDS:
        raise ValueError(f"points of {D} coordinates: auction_solve_points_batch takes at most {MAX_COORDS} "
                         f"(MISSLAP_POINTS_BATCH_MAX_COORDS)")
    if N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"problems of {N} x {M}: auction_solve_points_batch takes at most {MAX_DIM} x {MAX_DIM} "
                         f"(MISSLAP_POINTS_BATCH_MAX_DIM)")
    if on_device:
        if x.device != y.device:
            raise ValueError(f"x is on {x.device}, y on {y.device}")
        for name, a in (("x", x), ("y", y)):
            if min(int(s) for s in a.stride()) < 0:
                raise ValueError(f"{name} has strides {tuple(a.stride())}: a stride must be >= 0")
    return B, N, M, D, on_device, _lib.DTYPE_F32 if names[0] == "float32" else _lib.DTYPE_F64


_NO_FINISH = type("_NoFinish", (), {"__repr__": lambda self: "<no finish>"})()  # finish= was left out


def _strides(a, rows, D):
    """The element strides of a point set as the library reads it: a tensor's own, a numpy array's compact ones."""
    if isinstance(a, np.ndarray):
        return rows * D, D, 1
    return tuple(int(s) for s in a.stride())


def auction_solve_points_batch(x, y, problem="min", eps_start=0., max_iter=1000000, fast=None, shapes=None, prices=None,
                               outside=None, errors="raise", finish=_NO_FINISH):
    """Solve B independent dense problems whose costs are the squared distances between two point sets, one workgroup
    per problem; the cost stack is never stored.

    x: (B, N, D) and y: (B, M, D) of one dtype, float32 or float64, with 1 <= D <= MISSLAP_POINTS_BATCH_MAX_COORDS (8)
    and N, M <= MISSLAP_POINTS_BATCH_MAX_DIM (2048): numpy arrays, or tensors on one device.  A device tensor of any
    non-negative element strides is read where it lies -- state[..., :2] of a (B, N, 7) track state,
    pts.transpose(1, 2) of a (B, D, M) buffer, one.expand(B, M, D) -- and nothing is copied, cast or written; a numpy array
    goes through np.ascontiguousarray and the library's upload.  Problem b is the n_b x m_b problem (shapes, else N x M)
    with the costs of points_to_dense, whose docstring is the definition: a problem with status 0 is, bit for bit in sol,
    prices, outside_prices and every field of meta, problem b of
    auction_solve_batch(points_to_dense(x, y, shapes), shapes=shapes, ..., errors="status", cardinality_check=False), or
    with outside of auction_solve_batch(points_to_dense(x, y, shapes), shapes=shapes, outside=outside, ...,
    errors="status").  meta n_cols is m_b (m_b + n_b with outside), nnz is n_b * m_b (+ n_b with outside).

    shapes, prices, eps_start, max_iter, problem, fast and outside have the meaning, types, device / host forms and
    defaults they have in auction_solve_batch; fast=None is False without outside and with it True unless eps_start > 0.
    outside (a float, float64 (B,) or float64 (B, N)) is a squared-distance limit under the dense call's rule: -0.0 is
    valid, +inf gives MISSLAP_BATCH_STATUS_INFINITE_VALUE and a negative value or a NaN MISSLAP_BATCH_STATUS_BAD_OUTSIDE.
    A row never keeps a column dearer than its outside value at the optimum, so outside is also the radius gate.

    Both errors= modes run the same call and return the status-mode dict of auction_solve_batch with layout="points"
    (sol (B, N), prices (B, M), status (B,), matching_size (B,), meta, with outside also outside_prices (B, N));
    "raise" (default) then applies raise_for_status.  With device input the call is ordered on
    torch.cuda.current_stream(x.device): two launches (check, solve with verdict), allocations through torch only, no
    wait and no read-back.  The verdicts of a problem, in their order: BAD_SHAPE (a device shape outside 1 .. N x 1 .. M;
    nothing of the problem is read), with outside BAD_OUTSIDE, INFINITE_VALUE (some cost c[b, i, j] with i < n_b, j < m_b
    is not finite: a NaN or infinite coordinate inside the shape, or float64 coordinates whose squared distance overflows;
    with outside also an outside value of +inf), without outside INFEASIBLE (n_b > m_b; every pair is an edge, so no
    matcher runs), PRICE_NOT_FINITE, PRICE_NEGATIVE.  matching_size is min(n_b, m_b) for a good shape without outside,
    else -1.  A condemned problem has sol -1, prices 0 and a meta of n_rows, n_cols, nnz and zeros.

    finish: left out (the default), the call is the one described so far, in every respect.  The keyword takes the one
    value "reverse"; finish=None is a TypeError, as it was before the keyword existed (the call's whole-call checks pin
    that it has no finish=None), and any other value a ValueError.  finish="reverse" is for warm starts: every
    outside problem is rectangular (n_b rows, m_b + n_b objects), and a forward auction that starts from prices other
    than zero ends with status 0 and eCE = 1 but, in general, far from the optimum.  With finish="reverse" every problem
    with status 0 whose rows all hold an object gets the reverse-auction clean-up of auction_solve_batch(finish="reverse")
    behind its forward solve (misslap_points_batch_reverse_finish: one more launch on the same stream, nothing is waited
    for), with that call's meaning, result key and rules: the result is bit for bit points_reverse_finish (the definition)
    applied to the outputs of the same call without finish -- sol, prices, outside_prices and obj_f64, obj_f32 and eCE
    of meta; every other meta field, status and matching_size stay -- and gains reverse=dict(its, left), both -1 where the
    finish did not run (status != 0, or max_iter, which is also the finish's own budget, cut the forward solve) and left
    > 0 where the budget or a stalled iteration ended it.  Afterwards the assignment is optimal within n_b * final_eps.
    Both errors= modes run the status call, then the finish ("raise": then raise_for_status).  numpy point sets are
    uploaded once and the result comes back as numpy arrays.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    if finish is None:
        raise TypeError("auction_solve_points_batch() takes no finish=None: leave finish out for the call without a "
                        "finish, or pass finish='reverse'")
    if finish is not _NO_FINISH:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be left out or 'reverse', got {finish!r}")
        return _solve_with_finish(x, y, problem, eps_start, max_iter, fast, shapes, prices, outside, errors)
    B, N, M, D, on_device, dtype = _check_points(x, y)
    dev = x.device if on_device else None
    if dev is not None and _is_device_tensor(shapes):
        shp = _check_device_shapes(shapes, B, dev)
    elif _is_device_tensor(shapes):
        raise TypeError("shapes on the device need x / y on the device")
    else:
        shp = _check_shapes(shapes, B, N, M, "problem")
    e = _eps(eps_start)
    if _is_device_tensor(prices) and on_device and prices.device != dev:
        raise ValueError(f"prices are on {prices.device}, x on {dev}")
    p = _starting_prices(prices, B, M, True, on_device and not isinstance(prices, np.ndarray), x, "x / y")[0]
    out_v, out_ld = (None, 0) if outside is None else _check_outside(outside, B, N, dev, "x / y", "x", True)
    if fast is None:  # (resolved here: the library gets a plain flag)
        fast = outside is not None and not e > 0
    opts = _solve_options(on_device, x, problem, e, max_iter, dtype)
    xc, yc = (a if on_device else np.ascontiguousarray(a) for a in (x, y))
    lib = _lib.load()
    d_shp, d_p, d_out = _send(shp, dev), _send(p, dev), _send(out_v, dev)
    call = _StatusCall(lib, opts, B, N, M, None if outside is None else N, dev, "misslap_points_batch_workspace_bytes",
                       (B, N, M, 0 if p is None else 1, 0 if outside is None else 1))
    outs = call.outs if outside is not None else (*call.outs[:2], None, *call.outs[2:])
    _lib.check(lib.misslap_solve_points_batch(
        B, N, M, D, _ptr(xc), *_strides(xc, N, D), _ptr(yc), *_strides(yc, M, D), _ptr(d_shp), 1 if fast else 0, _ptr(d_p),
        *call.way, _ptr(d_out), out_ld, *outs))
    own = {} if outside is None else dict(outside=d_out)
    res = call.result((x, y, d_shp, d_p, d_out), shapes=d_shp, stack=(N, M), layout="points", **own)
    return raise_for_status(res) if errors == "raise" else res


def _reverse_finish_launch(x, y, res, problem, max_iter):
    """misslap_points_batch_reverse_finish on the device result `res` of a status-mode call on the device point sets x
    and y, on the call's stream: res's outputs are rewritten in place and res gains `reverse`."""
    import torch
    B, N, M, D, _, dtype = _check_points(x, y)
    dev = x.device
    opts = _solve_options(True, x, problem, 0.0, max_iter, dtype)
    with torch.cuda.device(dev):
        its, left = _empty(B, np.int64, dev), _empty(B, np.int32, dev)
    d_out = res.get("outside") if "outside_prices" in res else None
    _lib.check(_lib.load().misslap_points_batch_reverse_finish(
        B, N, M, D, _ptr(x), *_strides(x, N, D), _ptr(y), *_strides(y, M, D), _ptr(res["shapes"]), _ptr(d_out),
        0 if d_out is None or d_out.dim() == 1 else N, C.byref(opts), C.c_void_p(int(res["stream"].cuda_stream)),
        _ptr(res["status"]), _ptr(res["sol"]), _ptr(res["prices"]), _ptr(res.get("outside_prices")), _ptr(res["records"]),
        _ptr(its), _ptr(left)))
    res["reverse"] = dict(its=its, left=left)
    return its, left


def _solve_with_finish(x, y, problem, eps_start, max_iter, fast, shapes, prices, outside, errors):
    """auction_solve_points_batch(finish="reverse"): the status-mode call on device point sets, then the reverse finish
    on its outputs -- one more launch on the call's stream, nothing is waited for.  numpy point sets are uploaded once
    and their result brought back as numpy arrays."""
    on_device = _check_points(x, y)[4]
    xd, yd = x, y
    if not on_device:
        import torch
        dev = torch.device("cuda", int(os.environ.get(_ENV_DEVICE, 0)))
        xd, yd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, y))
    res = auction_solve_points_batch(xd, yd, problem, eps_start, max_iter, fast, shapes, prices, outside, "status")
    its, left = _reverse_finish_launch(xd, yd, res, problem, max_iter)
    if not on_device:
        meta = batch_meta_to_host(res)  # (waits for the call's stream once)
        res = {k: v for k, v in res.items() if k not in ("records", "info", "stream", "keep")}
        res = {k: _host(v) if _is_device_tensor(v) else v for k, v in res.items()}
        res.update(meta=meta, reverse=dict(its=_host(its), left=_host(left)))
    return raise_for_status(res) if errors == "raise" else res


def _status_error(res, b, code, n, m, card):
    """The exception of problem b of a points result (n: the record's n_rows; card: its matching_size)."""
    N, M = res["stack"]
    m = 0  # (only a bad shape names its columns)
    if code == _lib.BATCH_STATUS_BAD_SHAPE:
        n, m = (int(v) for v in _host(res["shapes"])[b])
    row, value = 0, 0.0
    if code == _lib.BATCH_STATUS_BAD_OUTSIDE:  # the first row < n_b whose outside value is no entry
        o = _host(res["outside"])[b]
        o = np.broadcast_to(o, (n,)) if o.ndim == 0 else o[:n]
        with np.errstate(invalid="ignore"):
            row = int(np.flatnonzero(~(o >= 0))[0])
        value = float(o[row])
    also = " or an outside value is +inf" if "outside_prices" in res else ""
    text = _STATUS_TEXT[code].format(n=n, m=m, N=N, M=M, card=card, row=row, value=value, also=also)
    return ValueError(f"problem {b}: {text}")


_STATUS_ERRORS["points"] = _status_error
