"""Many small dense assignment problems between two box sets (misslap_solve_boxes_batch, include/misslap.h).

The costs are 1 - IoU or 1 - GIoU of boxes (x1, y1, x2, y2), and the (B, N, M) stack is never stored: the kernels form
every cost they need from the coordinates (csrc/kernels_boxes_batch.hpp).  `boxes_to_dense` is the definition: the
result of a problem with status 0 is bit for bit the dense batch's (`auction_solve_batch`) on the float64 stack it
returns.  Problems of up to 2048 x 2048 are taken, twice the dense batch's cap.  It is the points call
(`auction_solve_points_batch`) with a third cost family: the keywords, the status mode, the stream ordering and the
list route (`candidates=K`: `boxes_candidates`, then `auction_solve_ell_batch`) are that call's; `boxes_to_ell` is the
definition of the lists.

These costs lie in [0, 2].  fast=True -- the default with `outside` -- means eps = 1 / n and a guarantee of
n * eps = 1 in total, which is coarse on this scale: a tracker should pass eps_start= (any 0 < eps_start <= 1 / n is
still a single phase, optimal within n * eps_start).  Rounds grow as C / eps.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_device_shapes, _check_outside, _check_shapes, _empty, _eps, _host,
                     _is_device_tensor, _options, _ptr, _send, _solve_options, _starting_prices, batch_meta_to_host,
                     raise_for_status)
from .ell_batch import auction_solve_ell_batch
from .points_batch import (_NO_FINISH, _check_k, _check_limit, _ell_from_costs, _np, _strides, _upload_points)

MAX_DIM = _lib.POINTS_BATCH_MAX_DIM
MAX_CANDIDATES = _lib.POINTS_CANDIDATES_MAX_K
_METRICS = {"iou": _lib.BOXES_METRIC_IOU, "giou": _lib.BOXES_METRIC_GIOU}

_STATUS_TEXT = {
    _lib.BATCH_STATUS_BAD_SHAPE: "shape ({n}, {m}) outside 1 .. {N} x 1 .. {M}",
    _lib.BATCH_STATUS_BAD_OUTSIDE: "the outside value of row {row} is {value!r}: it must be >= 0 (a negative value or a NaN "
                                   "would be an absent entry)",
    _lib.BATCH_STATUS_INFINITE_VALUE: "a box cost is not finite (a NaN or an infinite coordinate, or a width, an area, a sum "
                                      "of areas or a hull that overflows){also}",
    _lib.BATCH_STATUS_BAD_BOX: "a box has x2 < x1 or y2 < y1 (boxes are (x1, y1, x2, y2); zero width or height is legal)",
    _lib.BATCH_STATUS_INFEASIBLE: "Matrix is infeasible (Maximum matching possible only involves {card} out of {n} rows.)",
    _lib.BATCH_STATUS_PRICE_NOT_FINITE: "prices hold a NaN or an infinity",
    _lib.BATCH_STATUS_PRICE_NEGATIVE: "prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
}


def _check_metric(metric):
    if not isinstance(metric, str) or metric not in _METRICS:
        raise ValueError(f"metric must be 'iou' or 'giou', got {metric!r}")
    return _METRICS[metric]


def _boxes_ab(a, b):
    """a and b of the two definitions as numpy arrays, checked."""
    a, b = _np(a), _np(b)
    if a.ndim != 3 or b.ndim != 3:
        raise ValueError(f"a and b must have 3 dimensions (B, N, 4) and (B, M, 4), got {a.ndim} and {b.ndim}")
    if a.dtype != b.dtype or a.dtype not in (np.float32, np.float64):
        raise ValueError(f"a and b must both be float32 or both float64, got {a.dtype.name} and {b.dtype.name}")
    if a.shape[0] != b.shape[0] or a.shape[2] != 4 or b.shape[2] != 4:
        raise ValueError(f"a {a.shape} and b {b.shape} must be (B, N, 4) and (B, M, 4) with one B")
    return a, b


def _boxes_chain(a, b, giou):
    """The chain of boxes_to_dense on a (B, N, 4) and b (B, M, 4) from _boxes_ab.  Returns (c, bad, inv_a, inv_b): the
    float64 (B, N, M) result of the chain as it stands; bool (B, N, M), the pairs with a NaN or infinite coordinate or an
    infinite intermediate; bool (B, N) and (B, M), the boxes with x2 < x1 or y2 < y1."""
    aw, bw = a.astype(np.float64), b.astype(np.float64)
    inf = np.inf

    def lo(p, q):
        return np.where(p < q, p, q)

    def hi(p, q):
        return np.where(p > q, p, q)

    with np.errstate(all="ignore"):
        ax1, ay1, ax2, ay2 = (aw[:, :, None, k] for k in range(4))
        bx1, by1, bx2, by2 = (bw[:, None, :, k] for k in range(4))
        wa, ha = ax2 - ax1, ay2 - ay1
        wb, hb = bx2 - bx1, by2 - by1
        area_a, area_b = wa * ha, wb * hb
        bad = ~np.isfinite(aw).all(axis=2)[:, :, None] | ~np.isfinite(bw).all(axis=2)[:, None, :]
        for v in (wa, ha, area_a, wb, hb, area_b):
            bad = bad | (np.abs(v) == inf)
        iw = lo(ax2, bx2) - hi(ax1, bx1)
        ih = lo(ay2, by2) - hi(ay1, by1)
        bad = bad | (np.abs(iw) == inf) | (np.abs(ih) == inf)
        iw = np.where(iw > 0, iw, 0.0)
        ih = np.where(ih > 0, ih, 0.0)
        inter = iw * ih
        s = area_a + area_b
        bad = bad | (np.abs(inter) == inf) | (np.abs(s) == inf)
        u = s - inter
        q = inter / u
        iou = np.where(u > 0, q, 0.0)
        if not giou:
            c = 1.0 - iou
        else:
            cw = hi(ax2, bx2) - lo(ax1, bx1)
            ch = hi(ay2, by2) - lo(ay1, by1)
            hull = cw * ch
            bad = bad | (np.abs(cw) == inf) | (np.abs(ch) == inf) | (np.abs(hull) == inf)
            e = hull - u
            e = np.where(e > 0, e, 0.0)
            t = e / hull
            r = np.where(hull > 0, t, 0.0)
            g = iou - r
            c = 1.0 - g
        inv_a = (aw[:, :, 2] < aw[:, :, 0]) | (aw[:, :, 3] < aw[:, :, 1])
        inv_b = (bw[:, :, 2] < bw[:, :, 0]) | (bw[:, :, 3] < bw[:, :, 1])
    return np.array(np.broadcast_to(c, bad.shape), order="C"), bad, inv_a, inv_b


def _boxes_costs(a, b, metric):
    """The float64 (B, N, M) costs of boxes_to_dense before the shapes are applied."""
    c, bad, inv_a, inv_b = _boxes_chain(a, b, _check_metric(metric) == _lib.BOXES_METRIC_GIOU)
    c[bad | inv_a[:, :, None] | inv_b[:, None, :]] = np.inf
    return c


def boxes_to_dense(a, b, shapes=None, metric="iou"):
    """a (B, N, 4) and b (B, M, 4), boxes (x1, y1, x2, y2) of float32 or float64 (both the same), numpy arrays or tensors
    -> the float64 (B, N, M) cost stack of 1 - IoU (metric="iou") or 1 - GIoU ("giou"): the definition of
    auction_solve_boxes_batch.  With the coordinates widened to float64 (exact):

        per box   w = x2 - x1,  h = y2 - y1,  area = w * h
        per pair  iw = min(ax2, bx2) - max(ax1, bx1);  iw = iw > 0 ? iw : 0      (ih likewise, from the y's)
                  inter = iw * ih
                  s = area_a + area_b;  u = s - inter
                  iou = u > 0 ? inter / u : 0
        "iou"     c = 1 - iou
        "giou"    cw = max(ax2, bx2) - min(ax1, bx1)   (ch likewise);   hull = cw * ch
                  e = hull - u;  e = e > 0 ? e : 0
                  r = hull > 0 ? e / hull : 0
                  c = 1 - (iou - r)

    Every operation is a separately rounded IEEE float64 operation, in exactly this order: nothing is fused or
    reassociated, the division is correctly rounded, min, max and the selects are exact (min(p, q) is p < q ? p : q).
    The clamp of e is needed: hull - u comes out negative by rounding for boxes that (almost) fill their hull.
    For boxes with x2 >= x1 and y2 >= y1 rounding is monotone, so iw is at most either width, inter at most either
    area, s >= 2 inter and u >= inter: iou and r lie in [0, 1], a cost in [0, 1] ("iou") or [0, 2] ("giou"), and no cost
    is negative or -0.0.  Identical boxes cost +0.0, disjoint ones 1.0 under "iou", two zero-area boxes at one point
    (u = 0) 1.0.

    What is no cost.  A pair (i, j) is stored as +inf where a coordinate of either box is a NaN or infinite, where an
    intermediate of the chain is infinite -- a width, a height, an area, iw or ih before the clamp, inter, s, cw, ch or
    hull: float64 boxes can overflow there, float32 boxes cannot -- (the selects would otherwise swallow it: a NaN
    compares false), or where either box is a bad box, x2 < x1 or y2 < y1.  Zero width or height is legal.
    auction_solve_boxes_batch condemns a problem that holds such a pair inside its shape: INFINITE_VALUE for the first
    two, BAD_BOX behind it for the third.
    shapes: optional integer (B, 2); the elements beyond (n_b, m_b) of problem b are +inf.
    Problem b of auction_solve_boxes_batch(a, b, metric, shapes=shapes, ...) with status 0 is bit for bit problem b of
    auction_solve_batch(boxes_to_dense(a, b, shapes, metric), shapes=shapes, ..., errors="status",
    cardinality_check=False), or, with outside, of auction_solve_batch(boxes_to_dense(a, b, shapes, metric),
    shapes=shapes, outside=outside, ..., errors="status")."""
    a, b = _boxes_ab(a, b)
    c = _boxes_costs(a, b, metric)
    if shapes is not None:
        shp = np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes)
        for p in range(c.shape[0]):
            n, m = (max(int(v), 0) for v in shp[p])
            c[p, n:, :] = np.inf
            c[p, :, m:] = np.inf
    return c


def boxes_to_ell(a, b, k, shapes=None, limit=None, metric="iou"):
    """a (B, N, 4) and b (B, M, 4) as boxes_to_dense takes them, k in 1 .. 64 -> dict(cols int32 (B, N, k), vals float64
    (B, N, k), counts int32 (B, N), rows int32 (B,)): per row the (at most) k cheapest columns under the row's limit, as
    padded candidate lists in the layout auction_solve_ell_batch reads.  The definition of boxes_candidates and of
    auction_solve_boxes_batch(candidates=k): the GPU's four arrays are these bit for bit.

    It is points_to_ell on the costs c = boxes_to_dense(a, b, shapes, metric), and its docstring states the shapes, the
    candidates (c <= limit under the IEEE comparison, or c not finite), the counts, the truncation (the k smallest by
    (cost, column), the non-finite ones first), the order (ascending columns) and the holes.  limit is a cost:
    1 - t admits the pairs with IoU >= t.  A pair that boxes_to_dense stores as +inf -- a NaN or infinite coordinate, an
    infinite intermediate, a bad box -- is always a candidate, sorts first and is stored as +inf, so the ELL call
    condemns its problem with INFINITE_VALUE: BAD_BOX surfaces as status 3 on the list route."""
    k = _check_k(k)
    a, b = _boxes_ab(a, b)
    shp = None
    if shapes is not None:
        shp = np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes).astype(np.int64)
        if shp.shape != (a.shape[0], 2):
            raise ValueError(f"shapes must have shape ({a.shape[0]}, 2), got {shp.shape}")
    return _ell_from_costs(_boxes_costs(a, b, metric), k, shp, limit)


def _check_boxes(a, b):
    """dtype / rank / device of a and b; returns (B, N, M, on_device, the MISSLAP_DTYPE_* of the coordinates)."""
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        on_device = False
        names = (a.dtype.name, b.dtype.name)
        ndims = (a.ndim, b.ndim)
    elif _is_device_tensor(a) and _is_device_tensor(b):
        on_device = True
        names = (str(a.dtype).split(".")[-1], str(b.dtype).split(".")[-1])
        ndims = (a.dim(), b.dim())
    elif (isinstance(a, np.ndarray) or _is_device_tensor(a)) and (isinstance(b, np.ndarray) or _is_device_tensor(b)):
        raise TypeError("a and b must both be numpy arrays or both tensors on the device")
    else:
        raise TypeError("a and b must be numpy arrays or tensors on the device")
    if names[0] != names[1]:
        raise ValueError(f"a and b must have one dtype, got {names[0]} and {names[1]}")
    if names[0] not in ("float64", "float32"):
        raise ValueError(f"a and b must be float64 or float32, got {names[0]}")
    if ndims != (3, 3):
        raise ValueError(f"a and b must have 3 dimensions (B, N, 4) and (B, M, 4), got {ndims[0]} and {ndims[1]}")
    (B, N, D), (Bb, M, Db) = (tuple(int(v) for v in t.shape) for t in (a, b))
    if D != 4 or Db != 4:
        raise ValueError(f"a has shape {(B, N, D)}, b {(Bb, M, Db)}: a box is 4 coordinates (x1, y1, x2, y2)")
    if B != Bb:
        raise ValueError(f"a has shape {(B, N, D)}, b {(Bb, M, Db)}: B must agree")
    if B < 1 or N < 1 or M < 1:
        raise ValueError(f"empty box sets of shapes {(B, N, 4)} and {(B, M, 4)}")
    if N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"problems of {N} x {M}: auction_solve_boxes_batch takes at most {MAX_DIM} x {MAX_DIM} "
                         f"(MISSLAP_POINTS_BATCH_MAX_DIM)")
    if on_device:
        if a.device != b.device:
            raise ValueError(f"a is on {a.device}, b on {b.device}")
        for name, t in (("a", a), ("b", b)):
            if min(int(s) for s in t.stride()) < 0:
                raise ValueError(f"{name} has strides {tuple(t.stride())}: a stride must be >= 0")
    return B, N, M, on_device, _lib.DTYPE_F32 if names[0] == "float32" else _lib.DTYPE_F64


def auction_solve_boxes_batch(a, b, metric="iou", problem="min", eps_start=0., max_iter=1000000, fast=None, shapes=None,
                              prices=None, outside=None, errors="raise", candidates=None, finish=_NO_FINISH):
    """Solve B independent dense problems whose costs are 1 - IoU or 1 - GIoU between two box sets, one workgroup per
    problem; the cost stack is never stored.

    a: (B, N, 4) and b: (B, M, 4) of one dtype, float32 or float64, boxes (x1, y1, x2, y2) with x2 >= x1 and y2 >= y1,
    N, M <= MISSLAP_POINTS_BATCH_MAX_DIM (2048): numpy arrays, or tensors on one device.  A device tensor of any
    non-negative element strides is read where it lies -- state[..., :4] of a (B, N, 7) track state, a transposed
    (B, 4, M) buffer, one.expand(B, M, 4) -- and nothing is copied, cast or written; a numpy array goes through
    np.ascontiguousarray and the library's upload.  metric: "iou" or "giou".  Problem b is the n_b x m_b problem (shapes,
    else N x M) with the costs of boxes_to_dense, whose docstring is the definition: a problem with status 0 is, bit for
    bit in sol, prices, outside_prices and every field of meta, problem b of
    auction_solve_batch(boxes_to_dense(a, b, shapes, metric), shapes=shapes, ..., errors="status",
    cardinality_check=False), or with outside of auction_solve_batch(boxes_to_dense(a, b, shapes, metric), shapes=shapes,
    outside=outside, ..., errors="status").  meta n_cols is m_b (m_b + n_b with outside), nnz n_b * m_b (+ n_b).

    shapes, prices, eps_start, max_iter, problem, fast, outside and errors have the meaning, types, device / host forms
    and defaults they have in auction_solve_points_batch; fast=None is False without outside and with it True unless
    eps_start > 0.  outside (a float, float64 (B,) or float64 (B, N)) is a cost: 1 - iou_min gates at IoU >= iou_min, a
    row never keeps a column dearer than its outside value at the optimum.

    The costs lie in [0, 2].  fast=True -- the default with outside -- means eps = 1 / n_b and a guarantee of
    n_b * eps = 1 in total, which is coarse on this scale: it can leave a row outside that the optimum matches.  A
    tracker should pass eps_start= (any 0 < eps_start <= 1 / n_b is still a single phase, optimal within
    n_b * eps_start).  Rounds grow as C / eps.

    Both errors= modes run the same call and return the status-mode dict of auction_solve_batch with layout="boxes"
    (sol (B, N), prices (B, M), status (B,), matching_size (B,), meta, with outside also outside_prices (B, N)); "raise"
    (default) then applies raise_for_status.  With device input the call is ordered on
    torch.cuda.current_stream(a.device): two launches (check, solve with verdict), allocations through torch only, no
    wait and no read-back.  The verdicts of a problem, in their order: BAD_SHAPE, with outside BAD_OUTSIDE,
    INFINITE_VALUE (a NaN or infinite coordinate inside the shape, an infinite intermediate of the chain -- float64
    widths, areas, sums and hulls can overflow --, with outside also an outside value of +inf), BAD_BOX (code 16: a box
    inside the shape with x2 < x1 or y2 < y1), without outside INFEASIBLE (n_b > m_b; no matcher runs),
    PRICE_NOT_FINITE, PRICE_NEGATIVE.  A condemned problem has sol -1, prices 0 and a meta of n_rows, n_cols, nnz and
    zeros.

    candidates: left out (None), the call is the one described so far.  candidates=K (1 .. 64) takes the list route:
    boxes_candidates(a, b, K, shapes, limit=outside, metric=metric) builds per row the (at most) K cheapest columns under
    the row's outside value, and auction_solve_ell_batch(cols, vals, rows=rows, n_cols=M, outside=outside, prices=prices,
    problem="min", eps_start=..., max_iter=..., fast=..., finish=..., errors="status") solves the lists, back to back on
    the same stream; with device input nothing is waited for.  The result is the ELL call's dict (layout="ell") and gains
    candidates=dict(cols, vals, counts, rows) and truncated, int32 (B,): the rows of problem b with counts > K.
    Problem b is bit for bit problem b of that ELL call on boxes_to_ell(a, b, K, shapes, limit=outside, metric=metric).
    With outside and truncated[b] == 0 its optimum is the optimum of the full problem.  The builder has no status: a bad
    box, like a NaN coordinate, gives INFINITE_VALUE (3) on this route, not BAD_BOX.  prices= and finish="reverse" are
    available on this route (the ELL call's).  problem="max" with candidates is a ValueError.

    finish: left out, the call has no finish.  finish="reverse" needs candidates=K, else it is a ValueError: there is no
    boxes finish kernel, the list route runs the ELL finish.  finish=None is a TypeError, any other value a ValueError.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    code = _check_metric(metric)
    if finish is None:
        raise TypeError("auction_solve_boxes_batch() takes no finish=None: leave finish out for the call without a "
                        "finish, or pass finish='reverse' with candidates=K")
    if finish is not _NO_FINISH:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be left out or 'reverse', got {finish!r}")
    if candidates is not None:
        return _solve_from_candidates(a, b, code, candidates, problem, eps_start, max_iter, fast, shapes, prices, outside,
                                      errors, None if finish is _NO_FINISH else finish)
    if finish is not _NO_FINISH:
        raise ValueError("finish='reverse' needs candidates=K: there is no boxes finish kernel, the list route "
                         "(candidates=K, finish='reverse') runs the ELL finish on the box lists")
    B, N, M, on_device, dtype = _check_boxes(a, b)
    dev = a.device if on_device else None
    if dev is not None and _is_device_tensor(shapes):
        shp = _check_device_shapes(shapes, B, dev)
    elif _is_device_tensor(shapes):
        raise TypeError("shapes on the device need a / b on the device")
    else:
        shp = _check_shapes(shapes, B, N, M, "problem")
    e = _eps(eps_start)
    if _is_device_tensor(prices) and on_device and prices.device != dev:
        raise ValueError(f"prices are on {prices.device}, a on {dev}")
    p = _starting_prices(prices, B, M, True, on_device and not isinstance(prices, np.ndarray), a, "a / b")[0]
    out_v, out_ld = (None, 0) if outside is None else _check_outside(outside, B, N, dev, "a / b", "a", True)
    if fast is None:  # (resolved here: the library gets a plain flag)
        fast = outside is not None and not e > 0
    opts = _solve_options(on_device, a, problem, e, max_iter, dtype)
    ac, bc = (t if on_device else np.ascontiguousarray(t) for t in (a, b))
    lib = _lib.load()
    d_shp, d_p, d_out = _send(shp, dev), _send(p, dev), _send(out_v, dev)
    call = _StatusCall(lib, opts, B, N, M, None if outside is None else N, dev, "misslap_points_batch_workspace_bytes",
                       (B, N, M, 0 if p is None else 1, 0 if outside is None else 1))
    outs = call.outs if outside is not None else (*call.outs[:2], None, *call.outs[2:])
    _lib.check(lib.misslap_solve_boxes_batch(
        B, N, M, _ptr(ac), *_strides(ac, N, 4), _ptr(bc), *_strides(bc, M, 4), code, _ptr(d_shp), 1 if fast else 0,
        _ptr(d_p), *call.way, _ptr(d_out), out_ld, *outs))
    own = {} if outside is None else dict(outside=d_out)
    res = call.result((a, b, d_shp, d_p, d_out), shapes=d_shp, stack=(N, M), layout="boxes", metric=metric, **own)
    return raise_for_status(res) if errors == "raise" else res


def _candidates_launch(a, b, code, k, d_shp, d_lim, lim_ld):
    """misslap_boxes_batch_candidates on device box sets, on the current stream of their device: d_shp / d_lim are
    device tensors or None.  Returns dict(cols, vals, counts, rows) of device tensors; nothing is waited for."""
    import torch
    B, N, M, _, dtype = _check_boxes(a, b)
    dev = a.device
    opts = _options(True, a, mat_dtype=dtype)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        out = dict(cols=_empty((B, N, k), np.int32, dev), vals=_empty((B, N, k), np.float64, dev),
                   counts=_empty((B, N), np.int32, dev), rows=_empty(B, np.int32, dev))
    _lib.check(lib.misslap_boxes_batch_candidates(
        B, N, M, _ptr(a), *_strides(a, N, 4), _ptr(b), *_strides(b, M, 4), code, k, _ptr(d_shp), _ptr(d_lim), lim_ld,
        C.byref(opts), C.c_void_p(int(stream.cuda_stream)), *(_ptr(v) for v in out.values())))
    return out


def _candidates_input(a, b, shapes):
    """The whole-call checks of the two list calls on a, b and shapes.  Returns (B, N, M, on_device, shapes as the
    launch takes them: the device tensor, a checked int32 host array or None)."""
    B, N, M, on_device, _ = _check_boxes(a, b)
    if _is_device_tensor(shapes):
        if not on_device:
            raise TypeError("shapes on the device need a / b on the device")
        shp = _check_device_shapes(shapes, B, a.device)
    else:
        shp = _check_shapes(shapes, B, N, M, "problem")
    return B, N, M, on_device, shp


def _text(e):
    return str(e).replace("x / y", "a / b").replace(", x on", ", a on")


def boxes_candidates(a, b, k, shapes=None, limit=None, metric="iou"):
    """Per row the (at most) k cheapest boxes of b under the row's limit, as padded candidate lists: a batched,
    IoU-gated neighbour search on the costs of auction_solve_boxes_batch, and the lists auction_solve_ell_batch reads in
    place.  The (B, N, M) stack is never stored (misslap_boxes_batch_candidates: one launch, a wavefront per row).

    a (B, N, 4), b (B, M, 4), shapes and metric as auction_solve_boxes_batch takes them (device tensors of any
    non-negative strides are read where they lie); k in 1 .. MISSLAP_POINTS_CANDIDATES_MAX_K (64); limit: None, a float,
    or float64 (B,) / (B, N) -- a numpy array or, with device input, a contiguous tensor on the same device.  It is a
    cost: 1 - t admits the pairs with IoU >= t.  Returns dict(cols int32 (B, N, k), vals float64 (B, N, k), counts int32
    (B, N), rows int32 (B,)), bit for bit boxes_to_ell(a, b, k, shapes, limit, metric), whose docstring is the
    definition.  Device tensors give device tensors, ordered on torch.cuda.current_stream(a.device), and nothing is
    waited for; numpy box sets are uploaded once and the result comes back as numpy arrays."""
    k = _check_k(k)
    code = _check_metric(metric)
    B, N, _, on_device, shp = _candidates_input(a, b, shapes)
    try:
        lim, lim_ld = _check_limit(limit, B, N, a.device if on_device else None)
    except (TypeError, ValueError) as e:
        raise type(e)(_text(e)) from None
    ad, bd, _ = (a, b, None) if on_device else _upload_points(a, b)
    out = _candidates_launch(ad, bd, code, k, _send(shp, ad.device), _send(lim, ad.device), lim_ld)
    return out if on_device else {key: _host(v) for key, v in out.items()}


def _solve_from_candidates(a, b, code, candidates, problem, eps_start, max_iter, fast, shapes, prices, outside, errors,
                           finish):
    """auction_solve_boxes_batch(candidates=K): the builder with the outside values as its limit, then the ELL call on
    its lists, both on the current stream of the box sets' device; nothing is waited for with device input."""
    if problem != "min":
        raise ValueError(f"candidates needs problem='min', got {problem!r}: the lists hold the CHEAPEST columns")
    k = _check_k(candidates)
    B, N, M, on_device, shp = _candidates_input(a, b, shapes)
    _eps(eps_start)
    if not on_device and (_is_device_tensor(prices) or _is_device_tensor(outside)):
        raise TypeError(f"{'prices' if _is_device_tensor(prices) else 'outside'} on the device need a / b on the device")
    try:
        if outside is not None and not on_device:
            _check_outside(outside, B, N, None, "a / b", "a")  # (dtype, shape and a finite scalar, ahead of the upload)
        ad, bd, _ = (a, b, None) if on_device else _upload_points(a, b)
        dev = ad.device
        out_v, out_ld = (None, 0) if outside is None else _check_outside(outside, B, N, dev, "a / b", "a")
    except (TypeError, ValueError) as e:
        raise type(e)(_text(e)) from None
    d_out = _send(out_v, dev)
    cand = _candidates_launch(ad, bd, code, k, _send(shp, dev), d_out, out_ld)
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
    """The exception of problem b of a boxes result (n: the record's n_rows; card: its matching_size)."""
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


_STATUS_ERRORS["boxes"] = _status_error
