"""Many small sparse assignment problems in one call (misslap_solve_sparse_batch, include/misslap.h).

The batch form of `auction_solve(loc=, val=, size=)`: problem b of a packed (loc, val) is solved by one workgroup of one
launch, and its result is exactly what `from_sparse(loc_b, val_b, size=sizes[b], ...).solve()` returns
(csrc/kernels_batch_solve.hpp, csrc/kernels_sparse_batch.hpp).  The reference has no counterpart; it solves one
problem per AuctionSolver.

With `outside` every row also holds an outside option, so a row may stay unmatched (a partial assignment) and a row may
have no entry at all: problem b is its packed entries plus one entry (i, m_b + i) per row i < n_b, stored last in its
row, and its result is the reference's on that n_b x (m_b + n_b) problem (misslap_solve_sparse_batch_outside).
`sparse_to_augmented` is the definition; it is the one `ell_to_packed(outside=)` gives for the ELL layout.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_device_offsets, _check_offsets, _contiguous, _decode_meta,
                     _empty, _eps, _finished_to_host, _host, _is_device_tensor, _list_finish_launch, _maxima, _new_meta, _ptr,
                     _scalar_outside, _send, _solve_options, _starting_prices, raise_for_status)
from .auction_solve import _cname

MAX_DIM = _lib.SPARSE_BATCH_MAX_DIM
_INT_MAX = 2**31 - 1
_DEVICE_OFFSETS_NEED_DIMS = ("offsets on the device need dims=(Nmax, Mmax): sizing the outputs from loc would read it "
                             "back, and no wait may hide in this call")
_DEVICE_OFFSETS_DEFAULT_MODE = ("offsets on the device are taken with errors='status' or with outside= (and dims=): the "
                                "default mode reads offsets on the host")

# what each status code of misslap_solve_sparse_batch_status says in the words of the default mode without its host
# guard (abi_sparse_batch.hpp, abi_batch_common.hpp: reject_bad_prices)
_STATUS_TEXT = {
    _lib.BATCH_STATUS_NO_ENTRIES: "no entries",
    _lib.BATCH_STATUS_DIVISION_BY_ZERO: "division by zero",
    _lib.BATCH_STATUS_TOO_FEW_VALUES: "Matrix is infeasible - Fewer than {N} valid values provided for {N} rows.",
    _lib.BATCH_STATUS_INFEASIBLE: "Matrix is infeasible (Maximum matching possible only involves {card} out of {n} rows.)",
    _lib.BATCH_STATUS_ROWS_UNSORTED: "loc rows must be sorted in ascending order (auction_.pyx:33-48 contract)",
    _lib.BATCH_STATUS_ROW_GAP: "every row 0..N-1 must have at least one entry (auction_.pyx:33-48 contract)",
    _lib.BATCH_STATUS_INFINITE_VALUE: "val holds a NaN or an infinity",
    _lib.BATCH_STATUS_PRICES_TOO_NARROW: "prices hold {P} columns, the problem has {m}",
    _lib.BATCH_STATUS_PRICE_NOT_FINITE: "prices hold a NaN or an infinity",
    _lib.BATCH_STATUS_PRICE_NEGATIVE: "prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
}


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
    """dtype / shape / device of loc and val, offsets against them; returns (B, nnz, offsets, on_device, view).  offsets:
    int64 on the host, or the caller's device tensor.  view: None for what the contiguous entry points read -- numpy
    arrays, or contiguous int32 / float64 tensors with host offsets -- else what the view entry points need to know:
    dict(int64=, strides=(stride_e, stride_c), dtype=MISSLAP_DTYPE_*)."""
    view = None
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
        if loc.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"loc must be int32 or int64, got {loc.dtype}")
        if val.dim() != 1:
            raise ValueError(f"val must have 1 dimension, got {val.dim()}")
        if val.dtype not in (torch.float64, torch.float32):
            raise ValueError(f"val must be float64 or float32, got {val.dtype}")
        if not val.is_contiguous():
            raise ValueError("a device val tensor must be contiguous (it is read in place; loc may have any strides)")
        if loc.device != val.device:
            raise ValueError(f"loc is on {loc.device}, val on {val.device}")
        if loc.dtype != torch.int32 or val.dtype != torch.float64 or not loc.is_contiguous() or _is_device_tensor(offsets):
            view = dict(int64=loc.dtype == torch.int64, strides=tuple(int(x) for x in loc.stride()),
                        dtype=_lib.DTYPE_F32 if val.dtype == torch.float32 else _lib.DTYPE_F64)
    else:
        raise TypeError("loc and val must both be numpy arrays or both tensors on the device")
    nnz = int(loc.shape[0])
    if int(val.shape[0]) != nnz:
        raise ValueError(f"loc holds {nnz} entries, val {int(val.shape[0])}")
    if on_device and _is_device_tensor(offsets):
        B, off = _check_device_offsets(offsets, loc.device)
    else:
        B, off = _check_offsets(offsets, nnz, "offsets is required with packed loc / val (a list of (loc, val) pairs "
                                              "needs none)")
    return B, nnz, off, on_device, view


def sparse_to_augmented(loc, val, offsets, sizes=None, outside=0.):
    """numpy packed loc (nnz, 2) / val (nnz,) / offsets (B + 1,) -> [(loc_b int32, val_b float64, m_b, n_b)]: the
    definition of auction_solve_sparse_batch(outside=).  n_b = sizes[b, 1] where sizes is given, else the last stored
    row + 1; m_b = the largest real column + 1, 0 for a problem without an entry (sizes[b, 0] is not read).  The problem's
    own entries are kept in stored order, duplicates of an (i, j) included, and every row i < n_b -- a row without any
    other entry included -- gets one more entry (i, m_b + i), stored last in its row, whose value is the row's outside
    value.  outside: a float, float64 (B,) or float64 (B, P) with P >= every n_b.  Problem b is then
    auction_solve(loc=loc_b, val=val_b, size=(m_b + n_b, n_b), cardinality_check=False).  Rows must ascend."""
    loc, val, off = np.asarray(loc), np.asarray(val, dtype=np.float64), np.asarray(offsets, dtype=np.int64)
    if loc.ndim != 2 or loc.shape[1] != 2 or val.shape != (loc.shape[0],):
        raise ValueError(f"loc must have shape (nnz, 2) and val (nnz,), got {loc.shape} and {val.shape}")
    if off.ndim != 1 or off.shape[0] < 2 or off[0] != 0 or off[-1] != loc.shape[0] or (np.diff(off) < 0).any():
        raise ValueError("offsets must have length B + 1, start at 0, end at nnz and not decrease")
    B = off.shape[0] - 1
    szs = None if sizes is None else np.asarray(sizes)
    if szs is not None and szs.shape != (B, 2):
        raise ValueError(f"sizes must have shape ({B}, 2), got {szs.shape}")
    o = np.asarray(outside, dtype=np.float64)
    if o.ndim > 2 or (o.ndim >= 1 and o.shape[0] != B):
        raise ValueError(f"outside must be a float or have shape ({B},) or ({B}, P), got {o.shape}")
    out = []
    for b in range(B):
        lb, vb = loc[off[b]:off[b + 1]].astype(np.int64), val[off[b]:off[b + 1]]
        n = int(szs[b, 1]) if szs is not None else (int(lb[-1, 0]) + 1 if len(lb) else 0)
        m = int(lb[:, 1].max()) + 1 if len(lb) else 0
        if len(lb) and ((np.diff(lb[:, 0]) < 0).any() or lb[0, 0] < 0 or lb[-1, 0] >= n):
            raise ValueError(f"problem {b}: rows must ascend within 0 .. n_b - 1 = {n - 1}")
        if o.ndim == 2 and o.shape[1] < n:
            raise ValueError(f"outside holds {o.shape[1]} rows per problem, problem {b} has {n}")
        ob = np.broadcast_to(o if o.ndim == 0 else o[b] if o.ndim == 1 else o[b, :n], (n,))
        # behind the last stored entry of row i: a stable sort by row, the outside entries after the stored ones
        rows = np.concatenate([lb[:, 0], np.arange(n, dtype=np.int64)])
        order = np.argsort(rows, kind="stable")
        cols = np.concatenate([lb[:, 1], m + np.arange(n, dtype=np.int64)])[order]
        vals = np.concatenate([vb, ob])[order]
        out.append((np.ascontiguousarray(np.stack([rows[order], cols], axis=1), dtype=np.int32),
                    np.ascontiguousarray(vals, dtype=np.float64), m, n))
    return out


def _np(x):
    """A tensor as a numpy array on the host; everything else (an array, a list, a float) as it is."""
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def sparse_reverse_finish(loc, val, offsets, sol, prices, final_eps, shapes, problem="min", outside=None,
                          outside_prices=None, max_iter=1000000, run=None, trace=None):
    """The reverse-auction finish of auction_solve_sparse_batch / auction_solve_ell_batch(finish="reverse"), stated in
    numpy: its definition.

    Takes the outputs of a forward solve -- sol int (B, Nmax), prices float64 (B, Mmax), with `outside` also
    outside_prices float64 (B, Nmax), and final_eps (B,): meta["final_eps_f32"] -- on the packed problems loc (nnz, 2) /
    val (nnz,) / offsets (B + 1,) under the same problem and outside, or on a list of per-problem (loc_b, val_b) pairs
    with val and offsets None (an ELL stack goes through ell_to_packed(cols, vals, rows), without its outside keyword).
    shapes: int (B, 2), row b = (n_b, m_b): the rows and the REAL columns of problem b, from the solve's records: n_rows,
    and n_cols (minus n_rows with outside).

    The iteration is dense_reverse_finish's, not restated here: problem b becomes its dense image (a, valid) over the m_b
    real objects and, with outside, the n_b outside objects (object m_b + i has the one entry of row i), and the loop
    that serves the dense batch runs on it -- the same cursor / chained-object choice, strict ">", the smallest row
    winning a tie for beta, omega counting a second row at beta, the stall rule and the budget.  So the image decides and
    the stored order of a row does not.  Duplicates of an (i, j) are legal in the list families: the image holds the
    largest maximised value among them.  The finish's promise (eps-CS at the solve's final eps, no unassigned object
    priced above lambda, optimal within n_b * eps) is stated for problems without duplicates; with them this function is
    still the definition and the GPU matches it.

    Behind the loop eCE and the objective are recomputed as the list solve makes them: for row i on object j the choice
    is the LAST stored entry of column j in the row and every stored entry is tested against it (target_eps =
    float32(1 / n_b), tolerance 1e-7); the objective adds EVERY stored entry of the chosen column, in row order and
    within a row in stored order.

    Returns dict(sol, prices, [outside_prices], obj_f64, obj_f32, eCE, reverse=dict(its=int64 (B,), left=int32 (B,)), ran)
    with dense_reverse_finish's conventions: copies of the inputs rewritten where the finish ran (a row on its outside
    option is -1 in sol); its = left = -1 and obj_f64 = NaN where it did not run -- run[b] false (what the call uses:
    status == 0 and n_assigned == n_rows; by default every problem whose rows all hold an object), or a sol that is not
    a solve's output (a row without an object, an object that is not an entry of its row, two rows on one object) --
    and nothing of such a problem changes.  trace: an optional list that receives, per iteration, (b, j, i* or -1, the
    object i* left or -1, whether j was the object freed by the iteration before)."""
    from .dense_batch import _reverse_finish_one
    if isinstance(loc, (list, tuple)):
        if val is not None or offsets is not None:
            raise TypeError("a list of (loc, val) pairs takes no val / offsets")
        loc, val, offsets = _pack(loc)
    loc, val = np.asarray(_np(loc)), np.asarray(_np(val), dtype=np.float64)
    off = np.asarray(_np(offsets), dtype=np.int64)
    if loc.ndim != 2 or loc.shape[1] != 2 or val.shape != (loc.shape[0],):
        raise ValueError(f"loc must have shape (nnz, 2) and val (nnz,), got {loc.shape} and {val.shape}")
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("offsets must have length B + 1")
    B = off.shape[0] - 1
    shp = np.asarray(_np(shapes))
    if shp.shape != (B, 2):
        raise ValueError(f"shapes must have shape ({B}, 2), got {shp.shape}")
    sol = np.array(_np(sol), dtype=np.int32)
    prices = np.array(_np(prices), dtype=np.float64)
    if sol.ndim != 2 or sol.shape[0] != B or prices.ndim != 2 or prices.shape[0] != B:
        raise ValueError(f"sol and prices must have shape ({B}, Nmax) and ({B}, Mmax), got {sol.shape} and {prices.shape}")
    Nmax, Mmax = sol.shape[1], prices.shape[1]
    eps_b = np.asarray(_np(final_eps)).astype(np.float64).reshape(B)
    maximize = problem != "min"
    o = None
    if outside is not None:
        o = np.asarray(_np(outside), dtype=np.float64)
        if o.ndim > 2 or (o.ndim >= 1 and o.shape[0] != B) or (o.ndim == 2 and o.shape[1] < Nmax):
            raise ValueError(f"outside must be a float or have shape ({B},) or ({B}, P) with P >= {Nmax}, got {o.shape}")
        o = np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, max(Nmax, o.shape[1] if o.ndim == 2 else 0)))
        if outside_prices is None:
            raise ValueError("with outside, the solve's outside_prices are needed")
        outside_prices = np.array(_np(outside_prices), dtype=np.float64).reshape(B, Nmax)
    out = dict(sol=sol, prices=prices)
    if o is not None:
        out["outside_prices"] = outside_prices
    its, left = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int32)
    obj64, ece, ran = np.full(B, np.nan), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    run = None if run is None else np.asarray(_np(run)).astype(bool).reshape(B)
    for b in range(B):
        n, m = (int(x) for x in shp[b])
        if not (1 <= n <= Nmax and (0 if o is not None else 1) <= m <= Mmax) or (run is not None and not run[b]):
            continue
        ii, jj = loc[off[b]:off[b + 1], 0].astype(np.int64), loc[off[b]:off[b + 1], 1].astype(np.int64)
        x = val[off[b]:off[b + 1]] if maximize else val[off[b]:off[b + 1]] * -1.0  # the maximised values, in stored order
        if ((ii < 0) | (ii >= n) | (jj < 0) | (jj >= m)).any():
            continue
        mo = m + n if o is not None else m
        # the dense image: per (i, j) the largest maximised value among its stored copies
        a, valid = np.full((n, mo), -np.inf), np.zeros((n, mo), dtype=bool)
        np.maximum.at(a, (ii, jj), x)
        valid[ii, jj] = True
        a[~valid] = 0.0
        p = prices[b, :m].copy()
        rows = np.arange(n)
        if o is not None:
            ox = o[b, :n] if maximize else o[b, :n] * -1.0
            a[rows, m + rows], valid[rows, m + rows] = ox, True
            p = np.concatenate([p, outside_prices[b, :n]])
        p2o = sol[b, :n].astype(np.int64)
        if o is not None:
            p2o = np.where(p2o == -1, m + rows, p2o)
        if ((p2o < 0) | (p2o >= mo)).any() or not valid[rows, p2o].all() or np.unique(p2o).size != n:
            continue
        with np.errstate(invalid="ignore"):
            steps = None if trace is None else []
            its[b], left[b] = _reverse_finish_one(a, valid, p, p2o, eps_b[b], int(max_iter), steps)
            if trace is not None:
                trace.extend((b,) + t for t in steps)
            ran[b] = True
            sol[b, :n] = np.where(p2o < m, p2o, -1)
            prices[b, :m] = p[:m]
            if o is not None:
                outside_prices[b, :n] = p[m:]
            # eCE_satisfied at target_eps (auction_.pyx:443-485) and get_obj (:489-523) over the stored entries
            teps = float(np.float32(1.0 / np.float64(n)))
            hit = jj == p2o[ii]
            choice = a[rows, p2o].copy()  # (a row on its outside object: that one entry)
            for k in np.flatnonzero(hit):  # :462-467: the last stored match stays
                choice[ii[k]] = x[k]
            lhs = choice - p[p2o] + 1e-7
            bad = (lhs[ii] < (x - p[jj]) - teps).any()
            if o is not None:
                bad = bad or (lhs < (ox - p[m + rows]) - teps).any()
            ece[b] = 0 if bad else 1
            on_out = rows[p2o >= m]
            who = np.concatenate([ii[hit], on_out])
            what = np.concatenate([x[hit], a[on_out, p2o[on_out]]])
            obj = 0.0
            for k in np.argsort(who, kind="stable"):  # row order, within a row stored order
                v = float(what[k])
                obj = obj + v if maximize else obj - v
        obj64[b] = obj
    with np.errstate(over="ignore"):  # (an objective beyond float32 is +-inf there, as the kernel's cast gives it)
        obj32 = obj64.astype(np.float32)
    out.update(obj_f64=obj64, obj_f32=obj32, eCE=ece, reverse=dict(its=its, left=left), ran=ran)
    return out


def _check_sizes(sizes, B, dev=None):
    """sizes as the call reads them: int64 (B, 2) on the host, or with device input (dev) possibly the caller's
    contiguous int64 (B, 2) tensor on that device, whose values are the library's to judge."""
    if sizes is None:
        return None
    if _is_device_tensor(sizes):
        import torch
        if dev is None:
            raise TypeError("sizes on the device need loc / val on the device")
        if sizes.dtype != torch.int64 or tuple(sizes.shape) != (B, 2) or sizes.device != dev or not sizes.is_contiguous():
            raise ValueError(f"device sizes must be a contiguous int64 tensor of shape ({B}, 2) on {dev}, got {sizes.dtype} "
                             f"{tuple(sizes.shape)} on {sizes.device}")
        return sizes
    s = np.asarray(sizes)
    if s.shape != (B, 2) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"sizes must be an integer array of shape ({B}, 2), got {s.dtype} {s.shape}")
    return np.ascontiguousarray(s, dtype=np.int64)


def auction_solve_sparse_batch(loc, val=None, offsets=None, problem="min", eps_start=0., max_iter=1000000, fast=None,
                               sizes=None, cardinality_check=True, prices=None, errors="raise", dims=None, outside=None,
                               finish=None):
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

    errors="status": a verdict per problem instead.  The call only raises for what is wrong with the whole call (dtypes,
    the shapes of loc / val / offsets / sizes / prices, a NaN eps_start, dims); the result also holds status (int32 (B,),
    the MISSLAP_BATCH_STATUS_* codes of include/misslap.h) and matching_size (int32 (B,), the device guard's cardinality,
    -1 where it did not run).  Every problem with status 0 is solved, with exactly the default mode's results; the others
    have sol -1, prices 0 and a meta of n_rows, n_cols, nnz and zeros.  status[b] is the first check problem b fails in
    the default mode's order without its host guard: no entries, `fast` with N = 0, fewer entries than N, the matching
    guard (cardinality_check, on every graph that is clean -- rows ascending from 0 without a gap, no negative index --
    and within the cap), a negative index, rows not ascending, a row gap, a NaN / infinity in val, beyond dims or the cap,
    prices with fewer columns than the problem (prices may have any P >= 1 here), a bad starting price.  The one
    difference from the default mode: for a graph that is not clean or beyond the cap, the default mode with
    cardinality_check lets its host guard speak first ("loc entry ... outside", "rows must be sorted", an
    infeasibility); this mode does no host work and reports the structural code, with matching_size -1.  The guard
    always runs on the device here.  raise_for_status(res) raises what the default mode with cardinality_check=False
    raises for those codes (ZeroDivisionError for `fast` with N = 0).
    dims=(Nmax, Mmax), each 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM: the caller's bound on every problem's rows and columns;
    sol is (B, Nmax), prices (B, Mmax), and a problem beyond them gets MISSLAP_BATCH_STATUS_TOO_LARGE and is not solved.
    With loc / val on the device the call is stream-ordered: its kernels go onto torch.cuda.current_stream(loc.device),
    and sol, prices, status, matching_size and the meta fields are device tensors ordered on that stream
    (batch_meta_to_host(res) gives the default mode's meta dict).  With dims it waits for nothing and copies nothing
    back; without dims the maxima of loc are read back once before the call, the mode's only wait.  offsets stays a host
    array; sizes and prices may be host arrays (sent from pinned memory without a wait), prices also a device tensor.

    outside: partial assignments (misslap_solve_sparse_batch_outside).  A finite float, float64 (B,) or float64 (B, P)
    with P >= Nmax -- a numpy array or, with device input, a tensor on loc's device ((B,) contiguous; (B, P) with unit
    stride along a row, so a slice of a wider buffer is taken in place): the outside value of every row, in the units of
    val (problem="min": the cost of leaving row i unmatched; "max": the value of doing so).  It may be negative.  Problem
    b is then its packed entries plus one entry (i, m_b + i) per row i < n_b, stored last in its row, with n_b =
    sizes[b, 1] (without sizes the last stored row + 1) and m_b = the largest real column + 1 (sizes[b, 0] is not read);
    its result is bit for bit auction_solve(loc=loc_b, val=val_b, size=(m_b + n_b, n_b), cardinality_check=False) on
    sparse_to_augmented(loc, val, offsets, sizes, outside); with prices the solve starts from [p0[:m_b], zeros(n_b)].
    A ROW WITHOUT ANY ENTRY IS LEGAL -- leading, in the middle, or trailing when sizes names it -- and so is a problem
    without entries whose rows sizes names; graphs without a complete matching and n_b > m_b are solved.  The result is
    the status-mode dict: sol[b, i] is the real column, or -1 where row i took its outside option (and beyond n_b, on a
    condemned problem, or where max_iter cut the solve); prices stays (B, Mmax), the real columns; the new key
    outside_prices is float64 (B, Nmax), the price of row i's outside object and 0 beyond n_b (+inf for a row without
    any real entry: a one-entry row of the reference bids +inf).  meta is the augmented problem's record (n_rows = n_b,
    n_cols = m_b + n_b, nnz = nnz_b + n_b).  matching_size is -1: no guard is launched and cardinality_check is not
    consulted.  The checks, in their order: NO_ENTRIES (no entries and no sizes), NEGATIVE_INDEX, ROWS_UNSORTED,
    BAD_SHAPE (sizes[b, 1] < max(1, last row + 1)), INFINITE_VALUE (a NaN or an infinity in val or in the outside value of
    a row < min(n_b, Nmax)), TOO_LARGE (n_b > Nmax or m_b > Mmax), PRICES_TOO_NARROW, PRICE_NOT_FINITE, PRICE_NEGATIVE.
    A condemned problem has sol -1, prices 0, outside_prices 0.  Both values of errors run the same stream-ordered call;
    "raise" (the default) then raises ValueError("problem <b>: ...") for the first status that is not 0, and dims= is taken
    with either.  Without dims, Nmax = max(largest row + 1, largest sizes[:, 1]) and Mmax = max(largest column + 1, 1), each
    capped at MISSLAP_SPARSE_BATCH_MAX_DIM: the mode's single read-back with device input.  With device loc / val /
    outside and dims the call enqueues two launches on the current stream, waits for nothing and reads nothing back; a
    host outside travels from pinned memory as sizes and prices do.

    fast=None (default) is False without outside (the call is what it always was) and with outside True, unless
    eps_start > 0 was given (then False); an explicit fast= or eps_start= is passed through.  fast=True means
    eps = 1 / n_b.  Why: the augmented problem is rectangular, where the reference's eps-scaling is not optimal in general
    and a single phase from zero prices is (README "Rectangular problems").

    Views (device tensors only; misslap_solve_sparse_batch_status_view / _outside_view): what a device pipeline has is read
    where it lies.  loc may be int32 or int64 of shape (nnz, 2) with ANY non-negative strides -- idx[:, 1:] of a
    (nnz, 3) nonzero(), coo.indices()[1:].t() -- val float64 or float32 (1-d, contiguous; a float32 value is widened as it
    is read, which is exact, and everything downstream and every output stays float64), offsets a host array as before
    or a contiguous int64 (B + 1,) tensor on loc's device, sizes a host array or a contiguous int64 (B, 2) tensor there.
    A contiguous int32 / float64 loc / val with host offsets takes the calls it always took; everything else takes the
    view entry points, whose result is bit for bit that of the call on loc.to(int32).contiguous(), val.double(),
    offsets.cpu().  Device offsets are never read on the host, so they need dims= (ValueError without: no wait may
    hide in the call) and are taken with errors="status" and with outside= (the default mode reads offsets on the host:
    TypeError); they are judged per problem on the device: a slice that is not 0 <= offsets[b] <= offsets[b + 1] <= nnz
    (or holds 2^31 - 1 entries or more) gets status 7 (MISSLAP_BATCH_STATUS_BAD_SHAPE) ahead of every other check,
    nothing of it is read, its outputs are the condemned ones with an all-zero record, and no other problem notices.
    offsets[0] != 0 or offsets[B] != nnz is no error: entries in no slice are never read.  An int64 index outside the
    int32 range saturates before any check: a column >= 2^31 is TOO_LARGE (so is a last row that large with outside=;
    without, it is first of all a ROW_GAP, as INT32_MAX is in an int32 loc), a value <= -2^31 NEGATIVE_INDEX; nothing is
    truncated into a valid index.  errors="raise" on a view runs the status call and then raise_for_status, which
    returns the status-mode dict; raise_for_status copies device offsets / sizes back itself, after its synchronise.
    Host numpy arrays keep every rule they had (int32 loc, float64 val, offsets from 0 to nnz).  The recipe:

        idx = gate.nonzero()                                  # (nnz, 3) int64: b, i, j, sorted
        off = torch.searchsorted(idx[:, 0].contiguous(), torch.arange(B + 1, device=idx.device))   # int64 (B + 1,)
        res = auction_solve_sparse_batch(idx[:, 1:], cost[gate], off, dims=(N, M), outside=cost_limit, errors="status")

    No wait, no copy of an entry: the only launches besides the library's are nonzero, the mask gather and searchsorted.

    finish: None (default) is the call described so far, in every respect.  finish="reverse" is for rectangular problems
    (n_b < m_b, and every outside problem) that do NOT start from zero prices -- a tracker or a matcher that passes the
    last frame's prices= -- or that run the reference's eps-scaling: the forward auction then ends with eps-CS but, in
    general, far from the optimum, because objects that were bid up and abandoned keep prices above those of the objects
    in use; status 0 and eCE = 1 do not show it.  Every solved problem (status 0, every row assigned) then gets the
    reverse-auction clean-up behind its forward solve (misslap_sparse_batch_reverse_finish: one more launch on the same
    stream, one workgroup per problem, waiting for nothing; it first builds a column index of each problem in a
    workspace that the result keeps alive): lambda = the smallest price of an assigned object, and every unassigned
    object priced above lambda takes the row that values it most or drops to lambda.  Afterwards the assignment still
    satisfies eps-CS at the solve's final eps and no unassigned object is priced above lambda: optimal within
    n_b * final_eps from any starting prices and with any fast / eps_start (for problems without duplicates of an (i, j);
    with duplicates the largest value among them is the entry).  The result is exactly sparse_reverse_finish (its
    docstring is the definition) applied to the outputs of the same call with finish=None: sol, prices and outside_prices
    are rewritten, meta obj / obj_f64 and eCE recomputed, every other meta field stays the forward solve's, and the result
    gains reverse=dict(its=int64 (B,), left=int32 (B,)): the iterations made and the unassigned objects still priced
    above lambda (0 unless max_iter, which is also the finish's own budget, cut it, or a stalled iteration ended it:
    where eps is lost to rounding, outside max(|a|, |p|) * 2**-52 < final_eps, the finish ends with left > 0 while status
    stays 0 and eCE may be 1, so read left -- dense_reverse_finish has the rule); both -1 where the finish did not run --
    status != 0, or max_iter cut the forward solve -- and nothing of such a problem is touched.  It combines with every
    other keyword and with views; both errors= modes run the status call, then the finish ("raise": then
    raise_for_status) and return the status-mode dict.  Device input with dims= waits for nothing.  Numpy input, and a
    list of pairs, is uploaded once, takes the device route and comes back as numpy arrays (meta as batch_meta_to_host
    gives it).  Cold solves should keep fast=True from zero prices: that needs no finish.  Any other value raises
    ValueError.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    if finish is not None:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be None or 'reverse', got {finish!r}")
        return _solve_with_finish(loc, val, offsets, problem, eps_start, max_iter, fast, sizes, cardinality_check, prices,
                                  errors, dims, outside)
    if dims is not None and errors != "status" and outside is None:
        raise ValueError("dims is taken with errors='status' only")
    if isinstance(loc, (list, tuple)):
        if val is not None or offsets is not None:
            raise TypeError("a list of (loc, val) pairs takes no val / offsets; packed loc and val are numpy arrays or "
                            "device tensors")
        loc, val, offsets = _pack(loc)
    B, nnz, off, on_device, view = _check_input(loc, val, offsets)
    szs = _check_sizes(sizes, B, loc.device if on_device else None)
    if _is_device_tensor(off):
        if errors != "status" and outside is None:
            raise TypeError(_DEVICE_OFFSETS_DEFAULT_MODE)
        if dims is None:
            raise ValueError(_DEVICE_OFFSETS_NEED_DIMS)
    e = _eps(eps_start)
    if outside is not None:
        if fast is None:  # (resolved here: the library gets a plain flag)
            fast = not e > 0
        res = _solve_outside(loc, val, B, nnz, off, on_device, problem, e, max_iter, fast, szs, prices, dims, outside,
                             view)
        return raise_for_status(res) if errors == "raise" else res
    fast = bool(fast)  # (None: False, the call is what it was)
    if errors == "status" or view is not None or _is_device_tensor(szs):
        # (the default mode's own call reads compact int32 / float64 arrays and host offsets / sizes only)
        res = _solve_status(loc, val, B, nnz, off, on_device, problem, e, max_iter, fast, szs, cardinality_check, prices,
                            dims, view)
        return res if errors == "status" else raise_for_status(res)
    max_row, max_col, rows = _maxima(loc, off, on_device, per_problem=fast and szs is None)
    Nmax = min(max(max_row + 1, 1), MAX_DIM)  # (a problem beyond the cap is rejected by the library, in its order)
    Mmax = min(max(max_col + 1, 1), MAX_DIM)
    p, p_ptr, p_ld = _starting_prices(prices, B, Mmax, False, on_device, loc, "loc / val")  # (p lives through the call)
    if _is_device_tensor(prices) and prices.device != loc.device:
        raise ValueError(f"prices are on {prices.device}, loc on {loc.device}")
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
    dev = loc.device if on_device else None
    lc, vc = _contiguous(loc), _contiguous(val)  # (device tensors are: they are read in place)
    sol, pout = _empty((B, Nmax), np.int32, dev), _empty((B, Mmax), np.float64, dev)
    metas, info = _new_meta(B)
    _lib.check(_lib.load().misslap_solve_sparse_batch(
        B, C.c_void_p(_ptr(lc)), C.c_void_p(_ptr(vc)), off.ctypes.data, _ptr(szs), _ptr(eps_b),
        None if p_ptr is None else C.c_void_p(p_ptr), p_ld, 1 if cardinality_check else 0, C.byref(opts),
        C.c_void_p(_ptr(sol)), Nmax, C.c_void_p(_ptr(pout)), Mmax, 1 if on_device else 0, metas, C.byref(info)))
    return dict(sol=sol, prices=pout, meta=_decode_meta(metas, info))


def _check_dims(dims):
    try:
        ok = len(dims) == 2 and all(int(d) == d and 1 <= int(d) <= MAX_DIM for d in dims)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"dims must be (Nmax, Mmax), each an integer in 1 .. {MAX_DIM} (MISSLAP_SPARSE_BATCH_MAX_DIM), "
                         f"got {dims!r}")
    return int(dims[0]), int(dims[1])


def _status_prices(prices, B, on_device, loc):
    """Starting prices of a status-mode call: float64 (B, P), any P >= 1 (a problem with more columns gets its status)."""
    if prices is None:
        return None
    if isinstance(prices, np.ndarray):  # (with device input it is sent by the caller, from pinned memory)
        return _starting_prices(prices, B, 1, False, False, loc, "loc / val")[0]
    p = _starting_prices(prices, B, 1, False, on_device, loc, "loc / val")[0]
    if p.device != loc.device:
        raise ValueError(f"prices are on {p.device}, loc on {loc.device}")
    return p


def _solve_status(loc, val, B, nnz, off, on_device, problem, e, max_iter, fast, szs, cardinality_check, prices, dims,
                  view=None):
    """errors="status" of auction_solve_sparse_batch (misslap_solve_sparse_batch_status, or its view form)."""
    check = 1 if cardinality_check else 0
    p = _status_prices(prices, B, on_device, loc)  # (a host array, or with device input possibly a device tensor)
    Nmax, Mmax = _out_dims(dims, loc, off, on_device)
    opts = _solve_options(on_device, loc, problem, e, max_iter, _lib.DTYPE_F64 if view is None else view["dtype"])
    return _call(loc, val, B, nnz, off, on_device, opts, fast, szs, p, Nmax, Mmax, check, view=view)


def _out_dims(dims, loc, off, on_device, n_sized=0):
    """(Nmax, Mmax) of a status-mode call: dims, or as the default mode sizes its outputs (with device input this is the
    mode's one read-back); n_sized: the most rows sizes names, where they count."""
    if dims is not None:
        return _check_dims(dims)
    if _is_device_tensor(off):
        raise ValueError(_DEVICE_OFFSETS_NEED_DIMS)
    max_row, max_col, _ = _maxima(loc, off, on_device, per_problem=False)
    return min(max(max_row + 1, n_sized, 1), MAX_DIM), min(max(max_col + 1, 1), MAX_DIM)


def _view_head(B, nnz, loc, val, view, d_off):
    """The arguments of a view entry point that stand where the contiguous ones have (B, loc, val, offsets,
    offsets_dev): loc where it lies with its element strides, val, and the offsets on the device.  Nothing is copied."""
    se, sc = view["strides"]
    return (B, nnz, _ptr(loc), 1 if view["int64"] else 0, se, sc, _ptr(val), _ptr(d_off))


def _call(loc, val, B, nnz, off, on_device, opts, fast, szs, p, Nmax, Mmax, check, out_v=None, out_ld=0, view=None):
    """The call of misslap_solve_sparse_batch_status, or with outside values (out_v) of
    misslap_solve_sparse_batch_outside, in either mode, and its result dict.  There offsets is read on the host in both
    modes, and with device input a second time on the device.  With a view (_check_input) the call is the entry point's
    _view form: loc / val are read where they lie and offsets on the device only."""
    dev = loc.device if on_device else None
    lib = _lib.load()
    d_off = _send(off, dev) if on_device else None  # (a device tensor passes through)
    d_sizes, d_p, d_out = _send(szs, dev), _send(p, dev), _send(out_v, dev)
    p_ld, has_p = (0, 0) if p is None else (int(p.shape[1]), 1)
    if view is None:
        lc, vc = _contiguous(loc), _contiguous(val)  # (device tensors are: they are read in place)
        head = (B, _ptr(lc), _ptr(vc), off.ctypes.data, _ptr(d_off), _ptr(d_sizes), 1 if fast else 0, _ptr(d_p), p_ld)
        tag = ""
    else:
        head = (*_view_head(B, nnz, loc, val, view, d_off), _ptr(d_sizes), 1 if fast else 0, _ptr(d_p), p_ld)
        tag = "_view"
    if out_v is None:
        sizing = ("misslap_sparse_batch_workspace_bytes", (B, nnz, has_p, check)) if view is None else \
                 ("misslap_sparse_batch_view_workspace_bytes", (B, nnz, Nmax, has_p, check))
        call = _StatusCall(lib, opts, B, Nmax, Mmax, None, dev, *sizing)
        _lib.check(getattr(lib, "misslap_solve_sparse_batch_status" + tag)(*head, check, *call.way, Nmax, Mmax, *call.outs))
    else:
        call = _StatusCall(lib, opts, B, Nmax, Mmax, Nmax, dev, "misslap_sparse_batch_outside_workspace_bytes",
                           (B, Nmax, Mmax, has_p))
        _lib.check(getattr(lib, "misslap_solve_sparse_batch_outside" + tag)(*head, *call.way, Nmax, Mmax, _ptr(d_out),
                                                                            out_ld, *call.outs))
    return call.result((loc, val, d_off, d_sizes, d_p, d_out), layout="sparse", dims=(Nmax, Mmax), sizes=szs, offsets=off,
                       loc=loc, prices_ld=p_ld)


def _check_outside(outside, B, dev):
    """The outside values of a call, before Nmax is known: a finite float (broadcast to (B,) where the input lives), or
    float64 (B,) / (B, P) on the host or (with device input) on loc's device, a row of it with unit stride.  Returns
    (array or tensor, P or 0 for one value per problem, outside_ld)."""
    if _is_device_tensor(outside):
        import torch
        if dev is None:
            raise TypeError("outside on the device needs loc / val on the device")
        if outside.dtype != torch.float64:
            raise ValueError(f"outside must be float64, got {outside.dtype}")
        if outside.dim() not in (1, 2) or int(outside.shape[0]) != B or (outside.dim() == 2 and int(outside.shape[1]) < 1):
            raise ValueError(f"outside must have shape ({B},) or ({B}, P), got {tuple(outside.shape)}")
        if outside.device != dev:
            raise ValueError(f"outside is on {outside.device}, loc on {dev}")
        if outside.dim() == 1:
            if not outside.is_contiguous():
                raise ValueError("a device outside tensor of shape (B,) must be contiguous (it is read in place)")
            return outside, 0, 0
        P = int(outside.shape[1])
        ld = int(outside.stride(0)) if B > 1 else P
        if (P > 1 and outside.stride(1) != 1) or ld < P:
            raise ValueError("a device outside tensor of shape (B, P) must have unit stride along a row and rows that do "
                             "not overlap (it is read in place)")
        return outside, P, ld
    if isinstance(outside, np.ndarray):
        if outside.dtype != np.float64:
            raise ValueError(f"outside must be float64, got {outside.dtype.name}")
        if outside.ndim not in (1, 2) or outside.shape[0] != B or (outside.ndim == 2 and outside.shape[1] < 1):
            raise ValueError(f"outside must have shape ({B},) or ({B}, P), got {outside.shape}")
        o = np.ascontiguousarray(outside)
        return o, (o.shape[1] if o.ndim == 2 else 0), (o.shape[1] if o.ndim == 2 else 0)
    return _scalar_outside(outside, B, dev), 0, 0


def _solve_outside(loc, val, B, nnz, off, on_device, problem, e, max_iter, fast, szs, prices, dims, outside, view=None):
    """outside= of auction_solve_sparse_batch (misslap_solve_sparse_batch_outside, or its view form), in either mode."""
    dev = loc.device if on_device else None
    out_v, P, out_ld = _check_outside(outside, B, dev)
    p = _status_prices(prices, B, on_device, loc)  # (a host array, or with device input possibly a device tensor)
    # (sizes on the device without dims: read back with the maxima, the mode's one wait)
    Nmax, Mmax = _out_dims(dims, loc, off, on_device, int(szs[:, 1].max()) if szs is not None and dims is None else 0)
    if P and P < Nmax:
        raise ValueError(f"outside must have shape ({B},) or ({B}, P) with P >= Nmax = {Nmax}, got P = {P}")
    opts = _solve_options(on_device, loc, problem, e, max_iter, _lib.DTYPE_F64 if view is None else view["dtype"])
    return _call(loc, val, B, nnz, off, on_device, opts, fast, szs, p, Nmax, Mmax, None, out_v, out_ld, view=view)


def _reverse_finish_launch(res, problem, max_iter):
    """misslap_sparse_batch_reverse_finish on the device result `res` of a status-mode call, on the call's stream, with
    max_iter as the finish's budget: res's outputs are rewritten in place and res gains `reverse`.  The entries are read
    as a view -- packed arrays with their natural strides -- and the offsets are the device copy the call made."""
    _, loc, val, d_off, _, _, d_out = res["keep"][:7]
    import torch
    nnz, (Nmax, Mmax) = int(loc.shape[0]), res["dims"]
    dtype = _lib.DTYPE_F32 if val.dtype == torch.float32 else _lib.DTYPE_F64
    head = (int(res["status"].shape[0]), nnz, _ptr(loc), 1 if loc.dtype == torch.int64 else 0,
            *(int(x) for x in loc.stride()), _ptr(val), _ptr(d_off))
    return _list_finish_launch(res, "misslap_sparse_batch_reverse_finish", head, nnz, loc, problem, max_iter, dtype, Nmax,
                               Mmax, d_out if "outside_prices" in res else None)


def _solve_with_finish(loc, val, offsets, problem, eps_start, max_iter, fast, sizes, cardinality_check, prices, errors,
                       dims, outside):
    """auction_solve_sparse_batch(finish="reverse"): the status-mode call on device input, then the reverse finish on its
    outputs -- one more launch on the call's stream (misslap_sparse_batch_reverse_finish), nothing is waited for.  Numpy
    arrays and a list of pairs are uploaded once and their result brought back as numpy arrays."""
    if isinstance(loc, (list, tuple)):
        if val is not None or offsets is not None:
            raise TypeError("a list of (loc, val) pairs takes no val / offsets; packed loc and val are numpy arrays or "
                            "device tensors")
        loc, val, offsets = _pack(loc)
    on_device = _check_input(loc, val, offsets)[3]
    if not on_device:
        import os

        import torch

        from .auction_solve import _ENV_DEVICE
        dev = torch.device("cuda", int(os.environ.get(_ENV_DEVICE, 0)))
        loc, val = torch.from_numpy(np.ascontiguousarray(loc)).to(dev), torch.from_numpy(np.ascontiguousarray(val)).to(dev)
    res = auction_solve_sparse_batch(loc, val, offsets, problem, eps_start, max_iter, fast, sizes, cardinality_check, prices,
                                     "status", dims, outside)
    _reverse_finish_launch(res, problem, max_iter)
    if not on_device:
        res = _finished_to_host(res)
    return raise_for_status(res) if errors == "raise" else res


def _bad_slice(res, b):
    """The text for an unusable offsets[b] .. offsets[b + 1] of a result, or None where the slice is usable (device offsets
    are copied back here: the caller has synchronised)."""
    off, nnz = _host(res["offsets"]), int(res["loc"].shape[0])
    s, e = int(off[b]), int(off[b + 1])
    if 0 <= s <= e <= nnz and e - s < _INT_MAX:
        return None
    return (f"offsets[{b}] .. offsets[{b + 1}] = {s} .. {e} is not a slice of the {nnz} packed entries "
            f"(0 <= start <= end <= nnz, fewer than 2^31 - 1 entries)")


def _outside_error(res, b, code, n, m):
    """The exception of problem b of an outside-mode result (n, m: the record's n_rows and n_cols, m counting the n outside
    objects too)."""
    Nmax, Mmax = res["dims"]
    if m < _INT_MAX:
        m -= n
    if code == _lib.BATCH_STATUS_NO_ENTRIES:
        text = "no entries (and no sizes to name its rows)"
    elif code == _lib.BATCH_STATUS_NEGATIVE_INDEX:
        text = "loc holds a negative row or column index"
    elif code == _lib.BATCH_STATUS_BAD_SHAPE and _bad_slice(res, b):
        text = _bad_slice(res, b)
    elif code == _lib.BATCH_STATUS_BAD_SHAPE:
        text = f"sizes[{b}, 1] = {int(_host(res['sizes'])[b, 1])}: at least 1 and at least the last stored row + 1"
    elif code == _lib.BATCH_STATUS_INFINITE_VALUE:
        text = "val holds a NaN or an infinity (in an entry or in the outside value of a row)"
    elif code == _lib.BATCH_STATUS_TOO_LARGE:
        if m >= _INT_MAX:
            text = "column index too large (max + 1 must fit an int32)"
        else:
            text = f"{n} x {m} does not fit dims = ({Nmax}, {Mmax})"
    else:
        text = _STATUS_TEXT[code].format(N=n, n=n, m=m, card=-1, P=res["prices_ld"])
    return ValueError(f"problem {b}: {text}")


def _status_error(res, b, code, n, m, card):
    """The exception of problem b of a sparse status-mode result: what the default mode with cardinality_check=False
    raises for the same check (n, m: the record's n_rows and n_cols; card: its matching_size)."""
    if "outside_prices" in res:
        return _outside_error(res, b, code, n, m)
    if code == _lib.BATCH_STATUS_DIVISION_BY_ZERO:
        return ZeroDivisionError(f"problem {b}: division by zero")
    Nmax, Mmax = res["dims"]
    if code == _lib.BATCH_STATUS_BAD_SHAPE:  # (the view calls only: device offsets, judged per problem)
        text = _bad_slice(res, b) or "offsets name no usable slice"
    elif code == _lib.BATCH_STATUS_NEGATIVE_INDEX:
        last_row = int(res["loc"][int(_host(res["offsets"])[b + 1]) - 1, 0])
        text = "negative row index" if last_row < 0 else "loc holds a negative row or column index"
    elif code == _lib.BATCH_STATUS_TOO_LARGE:
        if m >= _INT_MAX:
            text = "column index too large (max + 1 must fit an int32)"
        elif n > MAX_DIM or m > MAX_DIM:
            text = (f"{n} x {m} exceeds MISSLAP_SPARSE_BATCH_MAX_DIM ({MAX_DIM}); solve it with from_sparse / "
                    f"solve_batch")
        else:
            text = f"{n} x {m} does not fit sol_ld = {Nmax} / prices_out_ld = {Mmax}"
    else:
        N = int(_host(res["sizes"])[b, 1]) if res["sizes"] is not None else n - 1  # from_sparse's N (sic, :592 / :594)
        text = _STATUS_TEXT[code].format(N=N, n=n, m=m, card=card, P=res["prices_ld"])
    return ValueError(f"problem {b}: {text}")


_STATUS_ERRORS["sparse"] = _status_error
