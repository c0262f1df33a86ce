"""Many small dense assignment problems between two point sets (misslap_solve_points_batch, include/misslap.h).

The costs are squared distances, c[b, i, j] = |x[b, i] - y[b, j]|^2, and the (B, N, M) stack is never stored: the
kernels form every cost they need from the coordinates (csrc/kernels_points_batch.hpp).  `points_to_dense` is the
definition: the result of problem b is bit for bit the dense batch's (`auction_solve_batch`) on the float64 stack it
returns.  Problems of up to 2048 x 2048 are taken, twice the dense batch's cap.

With `finish="reverse"` every solved problem gets the reverse-auction clean-up behind its forward solve, which makes a
warm start (`prices=` with `outside=`) optimal (misslap_points_batch_reverse_finish); `points_reverse_finish` is its
definition in numpy.

`points_candidates` turns the two point sets into padded candidate lists -- per row the (at most) K nearest columns
under a per-row limit, in the (B, N, K) layout `auction_solve_ell_batch` reads in place -- without storing the stack
(misslap_points_batch_candidates); `points_to_ell` is its definition in numpy.  With `candidates=K` the points call
runs that builder and the ELL solve back to back on the caller's stream.

`whiten=W` on the two definitions, the builder and the solve gives every row a lower-triangular matrix and the
Mahalanobis cost c[b, i, j] = |W[b, i] (x[b, i] - y[b, j])|^2 (misslap_solve_points_batch_whitened,
misslap_points_batch_candidates_whitened; csrc/kernels_points_whiten.hpp); `points_to_dense(..., whiten=W)` states it.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .auction_solve import _ENV_DEVICE
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_device_shapes, _check_outside, _check_shapes, _empty, _eps, _host,
                     _is_device_tensor, _options, _ptr, _send, _solve_options, _starting_prices, batch_meta_to_host,
                     raise_for_status)
from .dense_batch import dense_reverse_finish
from .ell_batch import auction_solve_ell_batch

MAX_DIM = _lib.POINTS_BATCH_MAX_DIM
MAX_COORDS = _lib.POINTS_BATCH_MAX_COORDS
MAX_CANDIDATES = _lib.POINTS_CANDIDATES_MAX_K
MAX_WHITEN_COORDS = _lib.POINTS_BATCH_MAX_WHITEN_COORDS

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


def _np(a):
    return np.asarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def _lower_triangles(whiten, x, shp):
    """whiten (B, N, D, D) of x's dtype -> float64 (B, N, D, D) holding W[b, i, k, l] for l <= k and i < shp[b, 0] (all
    rows without shp) and 0.0 everywhere else: exactly the elements the definition reads, and no other."""
    w = _np(whiten)
    B, N, D = x.shape
    if w.ndim != 4:
        raise ValueError(f"whiten must have 4 dimensions (B, N, D, D), got {w.ndim}")
    if w.dtype != x.dtype:
        raise ValueError(f"whiten must have the dtype of x and y, {x.dtype.name}, got {w.dtype.name}")
    if w.shape != (B, N, D, D):
        raise ValueError(f"whiten must have shape {(B, N, D, D)}, got {w.shape}")
    if D > MAX_WHITEN_COORDS:
        raise ValueError(f"points of {D} coordinates with whiten: at most {MAX_WHITEN_COORDS} "
                         f"(MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS)")
    rows = np.full(B, N) if shp is None else np.clip(np.asarray(shp)[:, 0].astype(np.int64), 0, N)
    keep = (np.arange(N)[None, :] < rows[:, None])[:, :, None, None] & np.tril(np.ones((D, D), dtype=bool))[None, None]
    out = np.zeros((B, N, D, D), dtype=np.float64)
    np.copyto(out, w, where=keep, casting="same_kind")
    return out


def _points_xy(x, y):
    """x and y of the two definitions as numpy arrays, checked."""
    x, y = _np(x), _np(y)
    if x.ndim != 3 or y.ndim != 3:
        raise ValueError(f"x and y must have 3 dimensions (B, N, D) and (B, M, D), got {x.ndim} and {y.ndim}")
    if x.dtype != y.dtype or x.dtype not in (np.float32, np.float64):
        raise ValueError(f"x and y must both be float32 or both float64, got {x.dtype.name} and {y.dtype.name}")
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2] or x.shape[2] < 1:
        raise ValueError(f"x {x.shape} and y {y.shape} must share B and D >= 1")
    return x, y


def _points_costs(x, y, whiten, shp):
    """The float64 (B, N, M) costs of points_to_dense before the shapes are applied (shp: only which rows of whiten are
    read).  x and y: from _points_xy."""
    D = x.shape[2]
    xw, yw = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if whiten is None:
            d = xw[:, :, None, 0] - yw[:, None, :, 0]
            c = d * d
            for k in range(1, D):
                d = xw[:, :, None, k] - yw[:, None, :, k]
                q = d * d
                c = c + q
        else:
            ww = _lower_triangles(whiten, x, shp)
            d = [xw[:, :, None, l] - yw[:, None, :, l] for l in range(D)]
            c = None
            for k in range(D):
                z = ww[:, :, None, k, 0] * d[0]
                for l in range(1, k + 1):
                    q = ww[:, :, None, k, l] * d[l]
                    z = z + q
                q = z * z
                c = q if k == 0 else c + q
    return np.ascontiguousarray(c)


def points_to_dense(x, y, shapes=None, whiten=None):
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
    errors="status").

    whiten: None (the default: everything above), or W of shape (B, N, D, D) and the dtype of x and y, a numpy array or
    a tensor, with D <= MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS (4): W[b, i] is a lower-triangular matrix for row i and
    the cost is the Mahalanobis form c[b, i, j] = |W[b, i] (x[b, i] - y[b, j])|^2.  With everything widened to float64:

        d_l    = xw[b, i, l] - yw[b, j, l]                  l = 0 .. D - 1
        z_k    = W[k][0] * d_0;  z_k = z_k + W[k][l] * d_l   for l = 1 .. k, in this order;  k = 0 .. D - 1
        s_0    = z_0 * z_0;      s_k = s_(k-1) + z_k * z_k
        c[b, i, j] = s_(D-1)

    D^2 + 3 D - 1 separately rounded float64 operations, nothing fused or reassociated.  Only W[b, i, k, l] with l <= k
    and i < n_b is ever read: the upper triangle and the rows beyond the shape may hold anything, NaN included.  A cost
    is a sum of squares, never negative and never -0.0, and it is not finite iff an intermediate of the chain is not
    finite: a NaN or infinite coordinate or matrix element that is read, an overflow, or -- unlike the plain chain, and
    from finite inputs -- two products that overflow to +inf and -inf, whose sum is a NaN.  With S = L L^T the innovation
    covariance of a track and W = L^-1, c is the Mahalanobis distance d^T S^-1 d."""
    x, y = _points_xy(x, y)
    shp = None if shapes is None else np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes)
    c = _points_costs(x, y, whiten, shp)
    B = c.shape[0]
    if shapes is not None:
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


def _check_k(k):
    """k of points_to_ell / points_candidates / candidates=: an integer in 1 .. MISSLAP_POINTS_CANDIDATES_MAX_K."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"the number of candidates per row must be an integer, got {k!r}")
    if not 1 <= int(k) <= MAX_CANDIDATES:
        raise ValueError(f"the number of candidates per row must be in 1 .. {MAX_CANDIDATES} "
                         f"(MISSLAP_POINTS_CANDIDATES_MAX_K), got {int(k)}")
    return int(k)


def points_to_ell(x, y, k, shapes=None, limit=None, whiten=None):
    """x (B, N, D) and y (B, M, D) as points_to_dense takes them, k in 1 .. 64 -> dict(cols int32 (B, N, k), vals float64
    (B, N, k), counts int32 (B, N), rows int32 (B,)): per row the (at most) k nearest columns under the row's limit, as
    padded candidate lists in the layout auction_solve_ell_batch reads.  The definition of points_candidates and of
    auction_solve_points_batch(candidates=k): the GPU's four arrays are these bit for bit.

    limit: None, a float, float64 (B,) (one value per problem) or float64 (B, N) (one per row).
    With c = points_to_dense(x, y, shapes) -- the chain of 3 D - 1 separately rounded float64 operations -- and
    (n_b, m_b) = shapes[b] (without shapes: (N, M)):

    Shapes      rows[b] = n_b for a shape inside 1 .. N x 1 .. M.  For any other shape rows[b] = 0, which
                auction_solve_ell_batch reports as BAD_SHAPE, and every slot of the problem is a hole.
    Candidates  for row i < n_b, column j < m_b is a candidate iff c[b, i, j] is not finite, or
                c[b, i, j] <= limit[b, i].  The comparison is IEEE: a limit of -0.0 admits a cost of +0.0, a NaN limit
                admits no finite cost, a limit of +inf every one; limit=None admits everything.  counts[b, i] is the
                number of candidates, before any truncation, and 0 for rows >= n_b.
    Non-finite  a cost that is not finite (a NaN or an infinite coordinate, or an overflow) is always a candidate, sorts
                ahead of every finite one and is stored as +inf (no NaN payload has to agree, and the ELL call then
                condemns exactly the problems the points call condemns, with INFINITE_VALUE).
    Truncation  where counts[b, i] > k the k smallest candidates by (cost, column) are kept, the non-finite ones first,
                by column.
    Order       the kept candidates are stored in ascending column order in slots 0 .., and every later slot holds
                cols = -1, vals = 0.0.  In column order an untruncated row is exactly the row gate.nonzero() would give
                the sparse batch.
    whiten      None, or W (B, N, D, D) as points_to_dense takes it: c is then points_to_dense(x, y, shapes, whiten=W),
                the limit is in the units of that cost, and everything above holds as it stands."""
    k = _check_k(k)
    x, y = _points_xy(x, y)
    shp = None
    if shapes is not None:
        shp = np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes).astype(np.int64)
        if shp.shape != (x.shape[0], 2):
            raise ValueError(f"shapes must have shape ({x.shape[0]}, 2), got {shp.shape}")
    # (the shape is applied below: beyond it nothing is a candidate, +inf or not)
    return _ell_from_costs(_points_costs(x, y, whiten, shp), k, shp, limit)


def _ell_from_costs(c, k, shp, limit):
    """The lists of points_to_ell from the float64 (B, N, M) costs c before the shapes are applied (shp: int64 (B, 2)
    or None); boxes_to_ell is the same function of its own costs."""
    B, N, M = c.shape
    if shp is None:
        shp = np.tile(np.array([N, M], dtype=np.int64), (B, 1))
    if limit is None:
        lim = None
    else:
        lim = np.asarray(limit.cpu() if hasattr(limit, "cpu") else limit, dtype=np.float64)
        if lim.shape not in ((), (B,), (B, N)):
            raise ValueError(f"limit must be a float or have shape ({B},) or ({B}, {N}), got {lim.shape}")
        lim = np.broadcast_to(lim if lim.ndim != 1 else lim[:, None], (B, N))
    cols = np.full((B, N, k), -1, dtype=np.int32)
    vals = np.zeros((B, N, k), dtype=np.float64)
    counts = np.zeros((B, N), dtype=np.int32)
    rows = np.zeros(B, dtype=np.int32)
    far = np.iinfo(np.int64).max
    for b in range(B):
        n, m = int(shp[b, 0]), int(shp[b, 1])
        if not (1 <= n <= N and 1 <= m <= M):
            continue
        rows[b] = n
        cost = c[b, :n, :m]
        finite = np.isfinite(cost)
        if lim is None:
            cand = np.ones((n, m), dtype=bool)
        else:
            with np.errstate(invalid="ignore"):
                cand = ~finite | (cost <= lim[b, :n, None])
        counts[b, :n] = cand.sum(axis=1)
        # the order (non-finite first, then cost, then column): a stable sort of the row on -inf / the cost, with what is
        # no candidate at +inf (no candidate's sort value is +inf)
        value = np.where(cand, np.where(finite, cost, -np.inf), np.inf)
        order = np.argsort(value, axis=1, kind="stable")[:, :k]
        kept = np.arange(order.shape[1])[None, :] < np.minimum(counts[b, :n], k)[:, None]
        kept_cols = np.sort(np.where(kept, order, far), axis=1)  # ascending columns, what was not kept behind them
        w = kept_cols.shape[1]
        here = kept_cols < far
        at = np.where(here, kept_cols, 0)
        stored = np.where(finite, cost, np.inf)
        cols[b, :n, :w] = np.where(here, at, -1)
        vals[b, :n, :w] = np.where(here, np.take_along_axis(stored, at, axis=1), 0.0)
    return dict(cols=cols, vals=vals, counts=counts, rows=rows)


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


def _check_whiten(whiten, x, B, N, D, on_device):
    """whiten of the GPU calls against the checked x: a numpy array with numpy point sets, a tensor on x's device with
    device point sets; shape (B, N, D, D), x's dtype, D within the whitened cap, strides >= 0."""
    if on_device:
        if not _is_device_tensor(whiten):
            raise TypeError("whiten must be a tensor on the device of x / y (x and y are device tensors)")
        name, ndim = str(whiten.dtype).split(".")[-1], whiten.dim()
        xname = str(x.dtype).split(".")[-1]
    else:
        if not isinstance(whiten, np.ndarray):
            raise TypeError("whiten must be a numpy array (x and y are numpy arrays)")
        name, ndim, xname = whiten.dtype.name, whiten.ndim, x.dtype.name
    if ndim != 4:
        raise ValueError(f"whiten must have 4 dimensions (B, N, D, D), got {ndim}")
    if name != xname:
        raise ValueError(f"whiten must have the dtype of x and y, {xname}, got {name}")
    if D > MAX_WHITEN_COORDS:
        raise ValueError(f"points of {D} coordinates with whiten: at most {MAX_WHITEN_COORDS} "
                         f"(MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS)")
    shape = tuple(int(v) for v in whiten.shape)
    if shape != (B, N, D, D):
        raise ValueError(f"whiten must have shape {(B, N, D, D)}, got {shape}")
    if on_device:
        if whiten.device != x.device:
            raise ValueError(f"whiten is on {whiten.device}, x on {x.device}")
        if min(int(s) for s in whiten.stride()) < 0:
            raise ValueError(f"whiten has strides {tuple(whiten.stride())}: a stride must be >= 0")


def _whiten_strides(w, N, D):
    """The element strides of the matrices as the library reads them: a tensor's own, a numpy array's compact ones."""
    if isinstance(w, np.ndarray):
        return N * D * D, D * D, D, 1
    return tuple(int(s) for s in w.stride())


_NO_FINISH = type("_NoFinish", (), {"__repr__": lambda self: "<no finish>"})()  # finish= was left out


def _strides(a, rows, D):
    """The element strides of a point set as the library reads it: a tensor's own, a numpy array's compact ones."""
    if isinstance(a, np.ndarray):
        return rows * D, D, 1
    return tuple(int(s) for s in a.stride())


def auction_solve_points_batch(x, y, problem="min", eps_start=0., max_iter=1000000, fast=None, shapes=None, prices=None,
                               outside=None, errors="raise", finish=_NO_FINISH, candidates=None, whiten=None):
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

    candidates: left out (None, the default), the call is the one described so far, in every respect.  candidates=K
    (1 .. MISSLAP_POINTS_CANDIDATES_MAX_K = 64) takes the list route: points_candidates(x, y, K, shapes, limit=outside)
    builds per row the (at most) K nearest columns under the row's outside value -- outside is the radius gate; without
    outside there is no limit -- and auction_solve_ell_batch(cols, vals, rows=rows, n_cols=M, outside=outside,
    prices=prices, problem="min", eps_start=..., max_iter=..., fast=..., finish=..., errors="status") solves the lists,
    back to back on the same stream; with device input nothing is waited for.  The result is the ELL call's dict
    (layout="ell"; outside, prices, fast and finish have that call's rules -- a scalar outside must be finite, prices are
    (B, P), finish left out is its finish=None) and gains candidates=dict(cols, vals, counts, rows), the builder's output,
    and truncated, int32 (B,): the rows of problem b with counts > K.  Problem b is bit for bit -- status, sol, prices,
    outside_prices, meta, reverse -- problem b of that ELL call on points_to_ell(x, y, K, shapes, limit=outside), the
    definition.  With outside and truncated[b] == 0 its optimum is the optimum of the full points problem: a pair dearer
    than the row's outside value is never in an optimal assignment.  Where truncated[b] > 0 some in-gate pairs were
    dropped and the optimum of the lists may be worse: raise K.  A NaN or infinite coordinate gives INFINITE_VALUE for its
    problem, a bad device shape BAD_SHAPE.  problem="max" with candidates is a ValueError: the lists are the NEAREST
    columns.  errors="raise" applies raise_for_status behind the solve (the ELL call's texts).  numpy point sets are
    uploaded once and the result comes back as numpy arrays.

    whiten: left out (None, the default), the call is the one described so far, in every respect.  whiten=W gives every
    row its own metric: W has shape (B, N, D, D) and the dtype of x and y, with D <= MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS
    (4), W[b, i] is a lower-triangular matrix and the cost is c[b, i, j] = |W[b, i] (x[b, i] - y[b, j])|^2, the chain of
    points_to_dense(x, y, shapes, whiten=W), which replaces points_to_dense(x, y, shapes) in every statement above
    (misslap_solve_points_batch_whitened).  For a Kalman tracker with innovation covariances S: L = cholesky(S),
    W = solve_triangular(L, eye(D), upper=False) gives the Mahalanobis distance d^T S^-1 d, and outside is its chi-square
    gate.  W is a numpy array with numpy point sets and a tensor on the same device with device point sets; a device view
    of any non-negative strides is read where it lies and never written -- cov[1:B + 1, 1:N + 1, :D, :D] of a larger
    buffer, W.expand(B, N, D, D) of one matrix per problem (B, 1, D, D) or of one for the call (1, 1, D, D).  Only the
    lower triangle of the rows i < n_b is read; the rest may hold anything.  INFINITE_VALUE then also covers a NaN or an
    infinite matrix element that is read, and finite inputs whose products overflow to +inf and -inf (their sum is a NaN).
    candidates=K with whiten runs the whitened builder (points_candidates(..., whiten=W)) and the ELL call unchanged, so
    prices= and finish="reverse" are available on that route.  finish="reverse" with whiten and without candidates is a
    ValueError: the points finish kernel takes no matrix.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    if finish is None:
        raise TypeError("auction_solve_points_batch() takes no finish=None: leave finish out for the call without a "
                        "finish, or pass finish='reverse'")
    if finish is not _NO_FINISH:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be left out or 'reverse', got {finish!r}")
    if candidates is not None:
        return _solve_from_candidates(x, y, candidates, problem, eps_start, max_iter, fast, shapes, prices, outside, errors,
                                      None if finish is _NO_FINISH else finish, whiten)
    if finish is not _NO_FINISH and whiten is not None:
        raise ValueError("finish='reverse' with whiten needs candidates=K: the points finish takes no matrix, the list "
                         "route (candidates=K, whiten=W, finish='reverse') runs the ELL finish on the whitened lists")
    if finish is not _NO_FINISH:
        return _solve_with_finish(x, y, problem, eps_start, max_iter, fast, shapes, prices, outside, errors)
    B, N, M, D, on_device, dtype = _check_points(x, y)
    if whiten is not None:
        _check_whiten(whiten, x, B, N, D, on_device)
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
    if whiten is None:
        _lib.check(lib.misslap_solve_points_batch(
            B, N, M, D, _ptr(xc), *_strides(xc, N, D), _ptr(yc), *_strides(yc, M, D), _ptr(d_shp), 1 if fast else 0,
            _ptr(d_p), *call.way, _ptr(d_out), out_ld, *outs))
    else:
        wc = whiten if on_device else np.ascontiguousarray(whiten)
        _lib.check(lib.misslap_solve_points_batch_whitened(
            B, N, M, D, _ptr(xc), *_strides(xc, N, D), _ptr(yc), *_strides(yc, M, D), _ptr(wc), *_whiten_strides(wc, N, D),
            _ptr(d_shp), 1 if fast else 0, _ptr(d_p), *call.way, _ptr(d_out), out_ld, *outs))
    own = {} if outside is None else dict(outside=d_out)
    if whiten is not None:
        own["whitened"] = True
    res = call.result((x, y, whiten, d_shp, d_p, d_out), shapes=d_shp, stack=(N, M), layout="points", **own)
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


def _check_limit(limit, B, N, dev):
    """The limit of points_candidates: None, a float (any: its sign and finiteness are the kernel's business), or
    float64 (B,) / (B, N) on the host or (with device input, dev) contiguous on the input's device, under the rules of
    _check_outside.  Returns (array or tensor or None, limit_ld)."""
    if limit is None:
        return None, 0
    if _is_device_tensor(limit) or isinstance(limit, np.ndarray):
        try:
            return _check_outside(limit, B, N, dev, "x / y", "x")
        except (TypeError, ValueError) as e:
            raise type(e)(str(e).replace("outside", "limit")) from None
    if isinstance(limit, (bool, str, bytes)) or not isinstance(limit, (int, float, np.integer, np.floating)):
        raise TypeError("limit must be a float, a float64 numpy array or a float64 tensor on the device")
    if dev is not None:
        import torch
        return torch.full((B,), float(limit), dtype=torch.float64, device=dev), 0
    return np.full(B, float(limit), dtype=np.float64), 0


def _candidates_launch(x, y, k, d_shp, d_lim, lim_ld, w=None):
    """misslap_points_batch_candidates (w, a checked device tensor: misslap_points_batch_candidates_whitened) on device
    point sets, on the current stream of their device: d_shp / d_lim are device tensors or None.  Returns dict(cols, vals, counts, rows) of device tensors; nothing is waited for."""
    import torch
    B, N, M, D, _, dtype = _check_points(x, y)
    dev = x.device
    opts = _options(True, x, mat_dtype=dtype)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        out = dict(cols=_empty((B, N, k), np.int32, dev), vals=_empty((B, N, k), np.float64, dev),
                   counts=_empty((B, N), np.int32, dev), rows=_empty(B, np.int32, dev))
    tail = (k, _ptr(d_shp), _ptr(d_lim), lim_ld, C.byref(opts), C.c_void_p(int(stream.cuda_stream)),
            *(_ptr(v) for v in out.values()))
    if w is None:
        _lib.check(lib.misslap_points_batch_candidates(
            B, N, M, D, _ptr(x), *_strides(x, N, D), _ptr(y), *_strides(y, M, D), *tail))
    else:
        _lib.check(lib.misslap_points_batch_candidates_whitened(
            B, N, M, D, _ptr(x), *_strides(x, N, D), _ptr(y), *_strides(y, M, D), _ptr(w), *_whiten_strides(w, N, D),
            *tail))
    return out


def _candidates_input(x, y, shapes, whiten=None):
    """The whole-call checks of the two list calls on x, y, shapes and whiten.  Returns (B, N, M, on_device, shapes as
    the launch takes them: the device tensor, a checked int32 host array or None)."""
    B, N, M, D, on_device, _ = _check_points(x, y)
    if whiten is not None:
        _check_whiten(whiten, x, B, N, D, on_device)
    if _is_device_tensor(shapes):
        if not on_device:
            raise TypeError("shapes on the device need x / y on the device")
        shp = _check_device_shapes(shapes, B, x.device)
    else:
        shp = _check_shapes(shapes, B, N, M, "problem")
    return B, N, M, on_device, shp


def _upload_points(x, y, whiten=None):
    """numpy x, y (and whiten) -> (x, y, whiten or None) on the device"""
    import torch
    dev = torch.device("cuda", int(os.environ.get(_ENV_DEVICE, 0)))
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, y, whiten))


def points_candidates(x, y, k, shapes=None, limit=None, whiten=None):
    """Per row the (at most) k nearest points of y under the row's limit, as padded candidate lists: a batched, gated
    nearest-neighbour search on the squared distances of auction_solve_points_batch, and the lists
    auction_solve_ell_batch reads in place.  The (B, N, M) stack is never stored (misslap_points_batch_candidates: one
    launch, a wavefront per row).

    x (B, N, D), y (B, M, D) and shapes as auction_solve_points_batch takes them (device tensors of any non-negative
    strides are read where they lie); k in 1 .. MISSLAP_POINTS_CANDIDATES_MAX_K (64); limit: None, a float, or float64
    (B,) / (B, N) -- a numpy array or, with device input, a contiguous tensor on the same device.  Its sign and
    finiteness are judged per row: -0.0 admits a cost of +0.0, a negative value or a NaN no finite cost, +inf every one.
    Returns dict(cols int32 (B, N, k), vals float64 (B, N, k), counts int32 (B, N), rows int32 (B,)), bit for bit
    points_to_ell(x, y, k, shapes, limit), whose docstring is the definition: candidates in ascending column order,
    holes (cols -1, vals 0.0) behind them, counts before truncation, rows[b] = 0 for a bad device shape, a cost that is
    not finite stored as +inf.  Device tensors give device tensors, ordered on torch.cuda.current_stream(x.device), and
    nothing is waited for; numpy point sets are uploaded once and the result comes back as numpy arrays.
    whiten: None, or W (B, N, D, D) as auction_solve_points_batch takes it (a numpy array or a device view, matching
    x / y; D <= 4): the costs are those of points_to_dense(x, y, shapes, whiten=W), the limit is in their units, and the
    result is bit for bit points_to_ell(x, y, k, shapes, limit, whiten=W) (misslap_points_batch_candidates_whitened)."""
    k = _check_k(k)
    B, N, _, on_device, shp = _candidates_input(x, y, shapes, whiten)
    lim, lim_ld = _check_limit(limit, B, N, x.device if on_device else None)
    xd, yd, wd = (x, y, whiten) if on_device else _upload_points(x, y, whiten)
    out = _candidates_launch(xd, yd, k, _send(shp, xd.device), _send(lim, xd.device), lim_ld, wd)
    return out if on_device else {key: _host(v) for key, v in out.items()}


def _solve_from_candidates(x, y, candidates, problem, eps_start, max_iter, fast, shapes, prices, outside, errors, finish,
                           whiten=None):
    """auction_solve_points_batch(candidates=K): the builder with the outside values as its limit, then the ELL call on
    its lists, both on the current stream of the point sets' device; nothing is waited for with device input."""
    if problem != "min":
        raise ValueError(f"candidates needs problem='min', got {problem!r}: the lists hold the NEAREST columns")
    k = _check_k(candidates)
    B, N, M, on_device, shp = _candidates_input(x, y, shapes, whiten)
    _eps(eps_start)
    if not on_device and (_is_device_tensor(prices) or _is_device_tensor(outside)):
        raise TypeError(f"{'prices' if _is_device_tensor(prices) else 'outside'} on the device need x / y on the device")
    if outside is not None and not on_device:
        _check_outside(outside, B, N, None, "x / y", "x")  # (dtype, shape and a finite scalar, ahead of the upload)
    xd, yd, wd = (x, y, whiten) if on_device else _upload_points(x, y, whiten)
    dev = xd.device
    out_v, out_ld = (None, 0) if outside is None else _check_outside(outside, B, N, dev, "x / y", "x")
    d_out = _send(out_v, dev)
    cand = _candidates_launch(xd, yd, k, _send(shp, dev), d_out, out_ld, wd)
    res = auction_solve_ell_batch(cand["cols"], cand["vals"], rows=cand["rows"], n_cols=M, problem="min",
                                  eps_start=eps_start, max_iter=max_iter, fast=fast, prices=prices, errors="status",
                                  outside=d_out, finish=finish)
    import torch
    res["candidates"] = cand
    res["truncated"] = (cand["counts"] > k).sum(dim=1, dtype=torch.int32)
    if not on_device:
        meta = batch_meta_to_host(res)  # (waits for the call's stream once)
        res = {key: v for key, v in res.items() if key not in ("records", "info", "stream", "keep")}
        res = {key: {q: _host(t) for q, t in v.items()} if key in ("candidates", "reverse") else v for key, v in res.items()}
        res = {key: _host(v) if _is_device_tensor(v) else v for key, v in res.items()}
        res["meta"] = meta
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
    if res.get("whitened") and code == _lib.BATCH_STATUS_INFINITE_VALUE:
        return ValueError(f"problem {b}: a cost |W_i (x_i - y_j)|^2 is not finite (a NaN or an infinite coordinate or "
                          f"element of the whitening matrix's lower triangle, or an overflow in the chain){also}")
    text = _STATUS_TEXT[code].format(n=n, m=m, N=N, M=M, card=card, row=row, value=value, also=also)
    return ValueError(f"problem {b}: {text}")


_STATUS_ERRORS["points"] = _status_error
