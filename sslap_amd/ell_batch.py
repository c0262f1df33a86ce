"""Many small sparse assignment problems given as padded candidate lists (misslap_solve_ell_batch, include/misslap.h).

The layout a top-k, a gating step or a nearest-neighbour search leaves on the device: `cols` (B, N, K) and `vals`
(B, N, K).  Problem b is rows 0 .. n_b - 1 of cols[b] / vals[b]; slot (i, k) is an entry iff cols[b, i, k] >= 0, a
negative column is a hole in any position and the value stored in a hole is never interpreted.  `ell_to_packed` is the
definition: the result of problem b is bit for bit `auction_solve(loc=loc_b, val=val_b, size=(m_b, n_b), ...)` on its
output (csrc/kernels_batch_solve.hpp, csrc/kernels_ell_batch.hpp).  The reference has no counterpart.

With `outside` every row also holds an outside option, so a row may stay unmatched (a partial assignment): problem b is
the packed problem plus one entry (i, m_b + i) per row, stored last in its row, and its result is the reference's on
that n_b x (m_b + n_b) problem (misslap_solve_ell_batch_outside).
"""
import numpy as np

from . import _lib
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_outside, _contiguous, _eps, _finished_to_host, _is_device_tensor,
                     _list_finish_launch, _ptr, _send, _solve_options, _starting_prices, raise_for_status)

MAX_DIM = _lib.SPARSE_BATCH_MAX_DIM
_INT_MAX = 2**31 - 1
_MAX_SLOTS = _INT_MAX - 128  # N * K: the guard indexes the slots of a problem with an int

# what each status code of misslap_solve_ell_batch says, in the words of the dense and the sparse batch where a code is
# theirs
_STATUS_TEXT = {
    _lib.BATCH_STATUS_BAD_SHAPE: "rows = {r} outside 1 .. {N}",
    _lib.BATCH_STATUS_EMPTY_ROW: "every row 0..N-1 must have at least one entry (auction_.pyx:33-48 contract)",
    _lib.BATCH_STATUS_INFINITE_VALUE: "val holds a NaN or an infinity{also}",
    _lib.BATCH_STATUS_PRICES_TOO_NARROW: "prices hold {P} columns, the problem has {m}",
    _lib.BATCH_STATUS_INFEASIBLE: "Matrix is infeasible (Maximum matching possible only involves {card} out of {n} rows.)",
    _lib.BATCH_STATUS_PRICE_NOT_FINITE: "prices hold a NaN or an infinity",
    _lib.BATCH_STATUS_PRICE_NEGATIVE: "prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
}


def ell_to_packed(cols, vals, rows=None, outside=None):
    """numpy (B, N, K) cols / vals -> [(loc_b int32 (nnz_b, 2), val_b float64 (nnz_b,))]: the entries of rows
    0 .. rows[b] - 1 of problem b in row order, within a row in slot order, the holes (cols < 0) dropped.  The
    definition of auction_solve_ell_batch: problem b is auction_solve(loc=loc_b, val=val_b, size=(m_b, n_b)) with
    n_b = rows[b] and m_b = loc_b[:, 1].max() + 1.
    outside (a float, float64 (B,) or float64 (B, N)): every row i < n_b gets one more entry (i, m_b + i), stored last in
    its row behind every slot, whose value is the row's outside value; m_b = max real column + 1, 0 for a problem without
    any entry.  Problem b is then auction_solve(loc=loc_b, val=val_b, size=(m_b + n_b, n_b))."""
    cols, vals = np.asarray(cols), np.asarray(vals)
    if cols.ndim != 3 or vals.shape != cols.shape:
        raise ValueError(f"cols and vals must have one shape (B, N, K), got {cols.shape} and {vals.shape}")
    B, N, _ = cols.shape
    ns = np.full(B, N) if rows is None else np.asarray(rows)
    if outside is not None:
        o = np.asarray(outside, dtype=np.float64)
        if o.shape not in ((), (B,), (B, N)):
            raise ValueError(f"outside must be a float or have shape ({B},) or ({B}, {N}), got {o.shape}")
        o = np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, N))
    out = []
    for b in range(B):
        n = max(int(ns[b]), 0)
        c, v = cols[b, :n], vals[b, :n]
        if outside is not None:  # one more slot behind the K of every row
            m = int(c.max()) + 1 if n and (c >= 0).any() else 0
            c = np.concatenate([c.astype(np.int64), (m + np.arange(n, dtype=np.int64))[:, None]], axis=1)
            v = np.concatenate([v.astype(np.float64), o[b, :n, None]], axis=1)
        i, k = np.nonzero(c >= 0)  # (row-major: row order, then slot order)
        loc = np.ascontiguousarray(np.stack([i, c[i, k]], axis=1), dtype=np.int32)
        out.append((loc, np.ascontiguousarray(v[i, k], dtype=np.float64)))
    return out


def _check_input(cols, vals):
    """dtype / shape / device of cols and vals; returns (B, N, K, on_device, cols_int64, the MISSLAP_DTYPE_* of vals)."""
    if isinstance(cols, np.ndarray) and isinstance(vals, np.ndarray):
        on_device = False
        names = (cols.dtype.name, vals.dtype.name)
        ndims = (cols.ndim, vals.ndim)
    elif _is_device_tensor(cols) and _is_device_tensor(vals):
        on_device = True
        names = (str(cols.dtype).split(".")[-1], str(vals.dtype).split(".")[-1])
        ndims = (cols.dim(), vals.dim())
    else:
        raise TypeError("cols and vals must both be numpy arrays or both tensors on the device")
    if names[0] not in ("int32", "int64"):
        raise ValueError(f"cols must be int32 or int64, got {names[0]}")
    if names[1] not in ("float64", "float32"):
        raise ValueError(f"vals must be float64 or float32, got {names[1]}")
    if ndims[0] != 3:
        raise ValueError(f"cols must have 3 dimensions (B, N, K), got {ndims[0]}")
    if tuple(vals.shape) != tuple(cols.shape):
        raise ValueError(f"cols has shape {tuple(cols.shape)}, vals {tuple(vals.shape)}")
    if on_device:
        if cols.device != vals.device:
            raise ValueError(f"cols is on {cols.device}, vals on {vals.device}")
        if not cols.is_contiguous() or not vals.is_contiguous():
            raise ValueError("device tensors must be contiguous (they are read in place)")
    B, N, K = (int(d) for d in cols.shape)
    if B < 1 or N < 1 or K < 1:
        raise ValueError(f"empty stack of shape {(B, N, K)}")
    if N > MAX_DIM:
        raise ValueError(f"problems of {N} rows: auction_solve_ell_batch takes at most {MAX_DIM} "
                         f"(MISSLAP_SPARSE_BATCH_MAX_DIM)")
    if N * K > _MAX_SLOTS:
        raise ValueError(f"N * K = {N * K} slots per problem: at most {_MAX_SLOTS}")
    return B, N, K, on_device, names[0] == "int64", _lib.DTYPE_F32 if names[1] == "float32" else _lib.DTYPE_F64


def _check_rows(rows, B, on_device, dev):
    """Optional int32 (B,) row counts, on the host or (with device input) on the device.  Their values are the
    library's to judge: a count outside 1 .. N is the problem's status."""
    if rows is None:
        return None
    if _is_device_tensor(rows):
        import torch
        if not on_device:
            raise TypeError("rows on the device need cols / vals on the device")
        if rows.dtype != torch.int32 or tuple(rows.shape) != (B,) or rows.device != dev or not rows.is_contiguous():
            raise ValueError(f"a device rows tensor must be contiguous int32 of shape ({B},) on {dev}, got {rows.dtype} "
                             f"{tuple(rows.shape)} on {rows.device}")
        return rows
    r = np.asarray(rows)
    if r.shape != (B,) or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"rows must be an integer array of shape ({B},), got {r.dtype} {r.shape}")
    return np.ascontiguousarray(np.clip(r, -1, _INT_MAX), dtype=np.int32)  # (whatever is out of range stays so)


def _check_n_cols(n_cols):
    try:
        ok = int(n_cols) == n_cols and 1 <= int(n_cols) <= MAX_DIM
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"n_cols must be an integer in 1 .. {MAX_DIM} (MISSLAP_SPARSE_BATCH_MAX_DIM), got {n_cols!r}")
    return int(n_cols)


def auction_solve_ell_batch(cols, vals, rows=None, n_cols=None, problem="min", eps_start=0., max_iter=1000000, fast=None,
                            cardinality_check=True, prices=None, errors="raise", outside=None, finish=None):
    """Solve B independent sparse problems given as padded candidate lists, one workgroup per problem.

    cols: int32 or int64 (B, N, K) and vals: float64 or float32 of the same shape, both numpy arrays or both contiguous
    tensors on one device (read in place, never written, problem='min' included).  Problem b is rows 0 .. rows[b] - 1
    (rows: optional int32 (B,), on the host or the device; default N); slot (i, k) is an entry iff cols[b, i, k] >= 0,
    any negative column is a hole and its value is never interpreted.  The result of problem b is bit for bit
    auction_solve(loc=loc_b, val=val_b, size=(m_b, n_b)) on ell_to_packed's (loc_b, val_b); float32 values are widened to
    float64 as they are read, which is exact.  N <= MISSLAP_SPARSE_BATCH_MAX_DIM, N * K <= 2^31 - 129.
    n_cols: Mmax in 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM, the caller's bound on every column (a column at or above it is
    MISSLAP_BATCH_STATUS_TOO_LARGE for its problem).  Without it the maximum of cols is taken: with device input that is
    the call's one read-back; with it a call on device input waits for nothing.
    prices: optional float64 (B, P) starting prices, on the host or the device; a problem with more than P columns gets
    MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW.

    errors="status" returns dict(sol=int32 (B, N) with -1 beyond n_b, prices=float64 (B, n_cols) with 0 beyond m_b,
    status=int32 (B,) MISSLAP_BATCH_STATUS_* codes, matching_size=int32 (B,), meta, layout="ell", ...): the dict of the
    other status modes, for device input device tensors ordered on torch.cuda.current_stream(cols.device).  The checks,
    in their order: rows[b] outside 1 .. N (BAD_SHAPE), an empty row, a NaN / infinity in an entry, a column >= n_cols,
    prices narrower than the problem, the matching guard (cardinality_check), a bad starting price.  A problem with a
    status other than 0 has sol -1, prices 0 and a meta of n_rows, n_cols, nnz and zeros.  batch_meta_to_host and
    raise_for_status take the result.
    errors="raise" (default) runs the same call and raises ValueError("problem <b>: ...") for the first problem whose
    status is not 0; else it returns the same dict.

    outside: partial assignments (misslap_solve_ell_batch_outside).  A finite float, float64 (B,) or float64 (B, N) -- a
    numpy array or, with device input, a contiguous tensor on the same device: the outside value of every row, in the
    units of vals (problem="min": the cost of leaving row i unmatched; "max": the value of doing so).  Problem b is then
    the packed problem plus one entry (i, m_b + i) per row, stored last in its row, and its result is bit for bit
    auction_solve(loc=loc_b, val=val_b, size=(m_b + n_b, n_b)) on ell_to_packed(cols, vals, rows, outside=outside); with
    prices the solve starts from [p0[:m_b], zeros(n_b)].  sol[b, i] is the real column, or -1 where row i took its outside
    option (and beyond n_b, on a condemned problem, or where max_iter cut the solve).  prices stays (B, n_cols), the real
    columns; the new key outside_prices is float64 (B, N), the price of row i's outside object and 0 beyond n_b (a row
    without any real entry bids +inf as a one-entry row of the reference does, so its outside price is +inf).  meta is the
    augmented problem's record (n_cols = m_b + n_b, nnz = entries + n_b; n_assigned counts rows on their outside option).
    The checks, in their order: BAD_SHAPE, INFINITE_VALUE (an entry or the outside value of a row < n_b is a NaN or an
    infinity), TOO_LARGE (a real column >= n_cols), PRICES_TOO_NARROW, PRICE_NOT_FINITE, PRICE_NEGATIVE.  EMPTY_ROW and
    INFEASIBLE cannot occur: rows without entries, graphs without a complete matching, n_b > m_b and problems of holes
    only are solved; the guard is not launched whatever cardinality_check says and matching_size is -1.  The values of
    rows >= n_b are never read.

    fast=None (default) is False without outside (the call is what it always was) and with outside True, unless
    eps_start > 0 was given (then False); an explicit fast= or eps_start= is passed through as it is.  Why: the augmented
    problem is rectangular (n rows, m + n columns).  A single phase (fast=True, or 0 < eps_start <= 1 / n) from zero prices
    is optimal within n * eps.  The reference's eps-scaling (fast=False, eps_start=0) keeps prices between phases and has no
    reverse phase: it gives the reference's answer on the augmented problem, which is NOT the optimum in general.  The
    same holds for every rectangular problem (n < m) of the batch solves.

    finish: None (default) is the call described so far, in every respect.  finish="reverse" is for rectangular problems
    (n_b < m_b, and every outside problem) that do NOT start from zero prices -- a tracker or a matcher that passes the
    last frame's prices= -- or that run the reference's eps-scaling: the forward auction then ends with eps-CS but, in
    general, far from the optimum, because objects that were bid up and abandoned keep prices above those of the objects
    in use; status 0 and eCE = 1 do not show it.  Every solved problem (status 0, every row assigned) then gets the
    reverse-auction clean-up behind its forward solve (misslap_ell_batch_reverse_finish: one more launch on the same
    stream, one workgroup per problem, waiting for nothing; it first builds a column index of each problem in a
    workspace that the result keeps alive).  Afterwards the assignment still satisfies eps-CS at the solve's final eps
    and no unassigned object is priced above lambda, the smallest price of an assigned object: optimal within
    n_b * final_eps from any starting prices and with any fast / eps_start (for problems without duplicates of an (i, j);
    with duplicates the largest value among them is the entry).  The result is exactly sparse_reverse_finish (its
    docstring is the definition) on ell_to_packed(cols, vals, rows) and the outputs of the same call with finish=None:
    sol, prices and outside_prices are rewritten, meta obj / obj_f64 and eCE recomputed, every other meta field stays the
    forward solve's, and the result gains reverse=dict(its=int64 (B,), left=int32 (B,)): the iterations made and the
    unassigned objects still priced above lambda (0 unless max_iter, which is also the finish's own budget, cut it, or a
    stalled iteration ended it: where eps is lost to rounding, outside max(|a|, |p|) * 2**-52 < final_eps, the finish
    ends with left > 0 while status stays 0 and eCE may be 1, so read left -- dense_reverse_finish has the rule); both
    -1 where the finish did not run -- status != 0, or max_iter cut the forward solve -- and nothing of such a problem
    is touched.  It combines with every other keyword; device input with n_cols= waits for nothing.  Numpy input is
    uploaded once, takes the device route and comes back as numpy arrays (meta as batch_meta_to_host gives it).  Cold
    solves should keep fast=True from zero prices: that needs no finish.  Any other value raises ValueError.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    if finish is not None:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be None or 'reverse', got {finish!r}")
        return _solve_with_finish(cols, vals, rows, n_cols, problem, eps_start, max_iter, fast, cardinality_check, prices,
                                  errors, outside)
    B, N, K, on_device, wide, dtype = _check_input(cols, vals)
    dev = cols.device if on_device else None
    rws = _check_rows(rows, B, on_device, dev)
    e = _eps(eps_start)
    if prices is not None:  # dtype and shape: float64 (B, P), any P >= 1; a device tensor only with device input
        _starting_prices(prices, B, 1, False, on_device and not isinstance(prices, np.ndarray), cols, "cols / vals")
        if _is_device_tensor(prices) and prices.device != dev:
            raise ValueError(f"prices are on {prices.device}, cols on {dev}")
    if n_cols is not None:
        Mmax = _check_n_cols(n_cols)
    else:  # (with device input the call's one read-back, ordered behind the current stream like every read of cols)
        Mmax = min(max(int(cols.max()) + 1, 1), MAX_DIM)
    check = 1 if cardinality_check else 0
    out_v, out_ld = (None, 0) if outside is None else _check_outside(outside, B, N, dev)
    if fast is None:  # (resolved here: the library gets a plain flag)
        fast = outside is not None and not e > 0
    opts = _solve_options(on_device, cols, problem, e, max_iter, dtype)
    lib = _lib.load()
    cc, vc = _contiguous(cols), _contiguous(vals)  # (device tensors are: they are read in place)
    d_rows, d_out, d_p = _send(rws, dev), _send(out_v, dev), _send(_contiguous(prices), dev)
    p_ld, has_p = (0, 0) if prices is None else (int(prices.shape[1]), 1)
    head = (B, N, K, _ptr(cc), 1 if wide else 0, _ptr(vc), _ptr(d_rows), 1 if fast else 0, _ptr(d_p), p_ld)
    if outside is None:
        call = _StatusCall(lib, opts, B, N, Mmax, None, dev, "misslap_ell_batch_workspace_bytes", (B, N, K, has_p, check))
        _lib.check(lib.misslap_solve_ell_batch(*head, check, *call.way, Mmax, *call.outs))
    else:
        call = _StatusCall(lib, opts, B, N, Mmax, N, dev, "misslap_ell_batch_outside_workspace_bytes",
                           (B, N, K, Mmax, has_p))
        _lib.check(lib.misslap_solve_ell_batch_outside(*head, *call.way, Mmax, _ptr(d_out), out_ld, *call.outs))
    res = call.result((cols, vals, d_rows, d_p, d_out), rows=d_rows, layout="ell", stack=(N, K), n_cols=Mmax, prices_ld=p_ld)
    return raise_for_status(res) if errors == "raise" else res


def _reverse_finish_launch(res, problem, max_iter):
    """misslap_ell_batch_reverse_finish on the device result `res` of a call on device input, on the call's stream, with
    max_iter as the finish's budget: res's outputs are rewritten in place and res gains `reverse`."""
    _, cols, vals, _, _, d_out = res["keep"][:6]
    import torch
    B, (N, K) = int(cols.shape[0]), res["stack"]
    dtype = _lib.DTYPE_F32 if vals.dtype == torch.float32 else _lib.DTYPE_F64
    head = (B, N, K, _ptr(cols), 1 if cols.dtype == torch.int64 else 0, _ptr(vals))
    return _list_finish_launch(res, "misslap_ell_batch_reverse_finish", head, B * N * K, cols, problem, max_iter, dtype, N,
                               res["n_cols"], d_out if "outside_prices" in res else None)


def _solve_with_finish(cols, vals, rows, n_cols, problem, eps_start, max_iter, fast, cardinality_check, prices, errors,
                       outside):
    """auction_solve_ell_batch(finish="reverse"): the call on device input, then the reverse finish on its outputs -- one
    more launch on the call's stream (misslap_ell_batch_reverse_finish), nothing is waited for.  Numpy arrays are
    uploaded once and their result brought back as numpy arrays."""
    on_device = _check_input(cols, vals)[3]
    if not on_device:
        import os

        import torch

        from .auction_solve import _ENV_DEVICE
        dev = torch.device("cuda", int(os.environ.get(_ENV_DEVICE, 0)))
        cols = torch.from_numpy(np.ascontiguousarray(cols)).to(dev)
        vals = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
    res = auction_solve_ell_batch(cols, vals, rows, n_cols, problem, eps_start, max_iter, fast, cardinality_check, prices,
                                  "status", outside)
    _reverse_finish_launch(res, problem, max_iter)
    if not on_device:
        res = _finished_to_host(res)
    return raise_for_status(res) if errors == "raise" else res


def _status_error(res, b, code, n, m, card):
    """The exception of problem b of an ELL result (n, m: the record's n_rows and n_cols; card: its matching_size)."""
    N, Mmax = res["stack"][0], res["n_cols"]
    if "outside_prices" in res and m < _INT_MAX:  # (the record counts the n outside objects too)
        m -= n
    if code == _lib.BATCH_STATUS_TOO_LARGE:
        if m >= _INT_MAX:
            text = "column index too large (max + 1 must fit an int32)"
        else:
            text = f"{n} x {m} does not fit n_cols = {Mmax}"
    else:
        r = N
        if code == _lib.BATCH_STATUS_BAD_SHAPE:
            rows = res["rows"]
            r = int(rows[b] if isinstance(rows, np.ndarray) else rows[b].item())
        also = " (in an entry or in the outside value of a row)" if "outside_prices" in res else ""
        text = _STATUS_TEXT[code].format(r=r, N=N, n=n, m=m, card=card, P=res["prices_ld"], also=also)
    return ValueError(f"problem {b}: {text}")


_STATUS_ERRORS["ell"] = _status_error
