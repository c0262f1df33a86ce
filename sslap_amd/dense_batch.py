"""Many small dense assignment problems in one call (misslap_solve_dense_batch, include/misslap.h).

No counterpart in the reference, whose own benchmark solves small dense matrices one at a time
(benchmarking.py:146).  Problem b of a (B, N, M) stack is solved by one workgroup of one launch, and its result is
exactly what `auction_solve(mat=mats[b, :n_b, :m_b], ...)` returns (csrc/kernels_batch_solve.hpp,
csrc/kernels_dense_batch.hpp).

With `outside` every row also holds an outside option, so a row may stay unmatched (a partial assignment): problem b is
the dense matrix `dense_to_augmented` returns, its slice plus an n_b x n_b block with the outside values on the diagonal
and -1 elsewhere, and its result is the reference's on that n_b x (m_b + n_b) matrix (misslap_solve_dense_batch_outside).

With `finish="reverse"` every solved problem gets the reverse-auction clean-up behind its forward solve, which makes a
rectangular solve optimal from any starting prices (misslap_dense_batch_reverse_finish); `dense_reverse_finish` is its
definition in numpy.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .auction_solve import _ENV_DEVICE
from ._batch import (_STATUS_ERRORS, _StatusCall, _check_device_shapes, _check_outside, _check_shapes, _check_stack,
                     _decode_meta, _empty, _entries_flag, _eps, _host, _is_device_tensor, _new_meta, _ptr, _send, _solve_options,
                     _stack_strides, _starting_prices, batch_meta_to_host, raise_for_status)  # (the last two: also for import from here)

MAX_DIM = _lib.DENSE_BATCH_MAX_DIM


# what each status code of misslap_solve_dense_batch_status says in the default mode's words (abi_dense_batch.hpp,
# abi_batch_common.hpp: reject_bad_prices, _batch._check_shapes)
_STATUS_TEXT = {
    _lib.BATCH_STATUS_TOO_FEW_VALUES: "Matrix is infeasible - Fewer than {n} valid values provided for {n} rows.",
    _lib.BATCH_STATUS_EMPTY_ROW: "every row must have at least one valid (>= 0) entry",
    _lib.BATCH_STATUS_INFINITE_VALUE: "val holds a NaN or an infinity",
    _lib.BATCH_STATUS_INFEASIBLE: "Matrix is infeasible (Maximum matching possible only involves {card} out of {n} rows.)",
    _lib.BATCH_STATUS_PRICE_NOT_FINITE: "prices hold a NaN or an infinity",
    _lib.BATCH_STATUS_PRICE_NEGATIVE: "prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
    _lib.BATCH_STATUS_BAD_SHAPE: "shape ({n}, {m}) outside 1 .. {N} x 1 .. {M}",
    _lib.BATCH_STATUS_BAD_OUTSIDE: "the outside value of row {row} is {value!r}: it must be >= 0 (a negative value or a NaN "
                                   "would be an absent entry)",
}


def dense_to_augmented(mats, shapes=None, outside=0.):
    """(B, N, M) stack -> [aug_b float64 (n_b, m_b + n_b)]: the definition of auction_solve_batch(outside=).
    aug_b = hstack([mats[b, :n_b, :m_b] widened to float64, D_b]) with D_b holding row i's outside value at (i, i) and
    -1.0 elsewhere; problem b is auction_solve(mat=aug_b, ..., cardinality_check=False).  mats: a numpy array of any float
    type or a tensor; shapes: optional integer (B, 2); outside: a float, float64 (B,) or float64 (B, N)."""
    if hasattr(mats, "cpu"):
        mats = mats.double().cpu().numpy()
    mats = np.asarray(mats)
    if mats.ndim != 3:
        raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.ndim}")
    B, N, M = mats.shape
    shp = np.tile([N, M], (B, 1)) if shapes is None else np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes)
    o = np.asarray(outside.cpu() if hasattr(outside, "cpu") else outside, dtype=np.float64)
    if o.shape not in ((), (B,), (B, N)):
        raise ValueError(f"outside must be a float or have shape ({B},) or ({B}, {N}), got {o.shape}")
    o = np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, N))
    out = []
    for b in range(B):
        n, m = (max(int(x), 0) for x in shp[b])
        d = np.full((n, n), -1.0)
        d[np.arange(n), np.arange(n)] = o[b, :n]
        out.append(np.ascontiguousarray(np.hstack([mats[b, :n, :m].astype(np.float64), d])))
    return out


def dense_to_packed(mats, shapes=None, entries="nonneg"):
    """(B, N, M) stack -> [(loc_b int32 (k, 2), val_b float64 (k,))]: the entries of mats[b, :n_b, :m_b] in row-major
    order, widened to float64 -- the definition of auction_solve_batch(entries=).  entries="nonneg": v >= 0 is an entry
    (-0.0 and +inf included; a negative value or a NaN is not), what from_matrix keeps.  entries="finite": every element
    that is not a NaN is one, so negative values, -0.0, subnormals and both infinities are.  With entries="finite"
    problem b of the batch is auction_solve(loc=loc_b, val=val_b, ..., cardinality_check=False) on that pair (with fast,
    eps = 1 / n_b as ever), and hopcroft_solve_batch(mats=, entries="finite") is hopcroft_solve(loc=loc_b).  mats: a numpy
    array of any float type or a tensor; shapes: optional integer (B, 2)."""
    _entries_flag(entries)
    if hasattr(mats, "cpu"):
        mats = mats.double().cpu().numpy()
    mats = np.asarray(mats)
    if mats.ndim != 3:
        raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.ndim}")
    B, N, M = mats.shape
    shp = np.tile([N, M], (B, 1)) if shapes is None else np.asarray(shapes.cpu() if hasattr(shapes, "cpu") else shapes)
    out = []
    for b in range(B):
        n, m = (max(int(x), 0) for x in shp[b])
        v = mats[b, :n, :m].astype(np.float64)
        with np.errstate(invalid="ignore"):
            keep = ~np.isnan(v) if entries == "finite" else v >= 0
        ii, jj = np.nonzero(keep)  # (row-major)
        out.append((np.ascontiguousarray(np.stack([ii, jj], axis=1).astype(np.int32)), np.ascontiguousarray(v[ii, jj])))
    return out


def _reverse_finish_one(a, valid, p, p2o, eps, max_iter, trace=None):
    """The reverse finish of one problem, in place: a, valid (n, mo) the maximised values and which of them are entries;
    p (mo,) the prices; p2o (n,) the assignment, every row assigned; eps the forward solve's final eps.  Returns
    (its, left).  Every operation is a float64 one, in the order csrc/kernels_dense_batch.hpp makes them.  trace: a list
    that receives (j, i*, freed object, whether j was the object freed last) per iteration (-1: none; a stalled
    iteration, which ends the finish, has a row and no freed object)."""
    n, mo = a.shape
    o2p = np.full(mo, -1, dtype=np.int64)
    o2p[p2o] = np.arange(n)
    lam = p[p2o].min()
    with np.errstate(invalid="ignore"):
        pi = a[np.arange(n), p2o] - p[p2o]
    cursor, nxt, its = 0, -1, 0
    ninf = -np.inf
    while True:
        chained = nxt >= 0
        if chained:
            j, nxt = nxt, -1
        else:
            open_ = np.flatnonzero((o2p[cursor:] == -1) & (p[cursor:] > lam))
            if open_.size == 0:
                return its, 0
            j = cursor + int(open_[0])
            cursor = j + 1
        if its >= max_iter:
            return its, int(np.count_nonzero((o2p == -1) & (p > lam)))
        its += 1
        beta, omega, istar = ninf, ninf, -1
        rows = np.flatnonzero(valid[:, j])
        if rows.size:
            w = a[rows, j] - pi[rows]
            k = int(np.argmax(w))  # (the first maximum: the smallest row wins a tie)
            if w[k] > ninf:
                beta, istar = w[k], int(rows[k])
                if rows.size > 1:
                    omega = np.delete(w, k).max()  # (a second row at beta counts: omega == beta)
        if istar < 0 or lam >= beta - eps:
            p[j] = lam
            if trace is not None:
                trace.append((j, -1, -1, chained))
            continue
        t = omega - eps
        pj = t if t > lam else lam
        if not (a[istar, j] - pj > pi[istar]):  # a stall: eps is lost to rounding, the move would not raise the profit
            if trace is not None:
                trace.append((j, istar, -1, chained))
            return its, int(np.count_nonzero((o2p == -1) & (p > lam)))
        p[j] = pj
        pi[istar] = a[istar, j] - p[j]
        jo = int(p2o[istar])
        o2p[jo], o2p[j], p2o[istar] = -1, istar, j
        if p[jo] > lam:
            nxt = jo
        if trace is not None:
            trace.append((j, istar, jo, chained))


def dense_reverse_finish(mats, sol, prices, final_eps, problem="min", shapes=None, outside=None, outside_prices=None,
                         entries="nonneg", max_iter=1000000, run=None, trace=None):
    """The reverse-auction finish of auction_solve_batch(finish="reverse"), stated in numpy: its definition.

    Takes the outputs of a forward solve -- sol int (B, N), prices float64 (B, M), with `outside` also outside_prices
    float64 (B, N), and final_eps (B,): meta["final_eps_f32"], widened to float64 -- on the stack `mats` (a numpy array of
    any float type or a tensor, as dense_to_packed takes it) under the same problem, shapes, outside and entries, and
    runs on every problem b with run[b] the modified reverse auction with a fixed lambda (Bertsekas, Network
    Optimization, 7.2).  run: bool (B,), what the call uses: status == 0 and n_assigned == n_rows; by default every
    problem whose rows all hold an object.

    One problem: a[i][j] is the maximised value of entry (i, j) -- the element widened to float64, times -1.0 for
    problem="min" -- over the m_b real objects and, with outside, the object m_b + i of each row (its one entry is
    (i, outside value of row i)); p the prices over the same objects; p2o the augmented assignment (a row on its outside
    option holds m_b + i).  lambda = min_i p[p2o[i]], pi[i] = a[i][p2o[i]] - p[p2o[i]], cursor = 0.  Then, until no
    unassigned object with p > lambda is left (left = 0) or max_iter iterations were made (left = their number):
    j is the object the last iteration freed if that is still priced above lambda, else the first such object at or
    behind the cursor (cursor = j + 1); over the rows i that have entry (i, j), in ascending i, w = a[i][j] - pi[i], beta
    the largest (the smallest i wins a tie), omega the second largest (-inf without one); without an entry, or when
    lambda >= beta - eps, p[j] = lambda; otherwise pj = max(lambda, omega - eps) and, if a[i*][j] - pj > pi[i*],
    p[j] = pj, pi[i*] = a[i*][j] - p[j], and row i* moves to j, freeing its object.

    The stall rule: if a[i*][j] - pj > pi[i*] is false the finish ends there.  The iteration is counted in its, no cell
    changes, and left is the number of unassigned objects priced above lambda, j included (the budget's formula).  In
    exact arithmetic every move raises the moving row's profit by at least eps, which is why the loop ends; where eps is
    below one ulp of the profits a move can leave the profit unchanged, and two objects would hand one row back and
    forth until max_iter.  Inside max(|a|, |p|) * 2**-52 < eps no iteration stalls; outside it the finish promises
    nothing: status stays 0 and eCE may be 1, so a caller reads left.

    Returns dict(sol, prices, [outside_prices], obj_f64, obj_f32, eCE, reverse=dict(its=int64 (B,), left=int32 (B,)), ran):
    copies of the inputs rewritten where the finish ran (an outside object is -1 in sol), the objective summed in row
    order as the solve sums it, eCE at target_eps = float32(1 / n_b) with the solve's tolerance 1e-7; its = left = -1 and
    obj_f64 = NaN where it did not run (ran[b] False): nothing of such a problem changes.  Afterwards every row holds an
    object within eps of its best net value, and every unassigned object is priced at or below lambda: the assignment is
    optimal within n_b * eps, whatever prices the forward solve started from.  trace: an optional list that receives,
    per iteration, (b, j, i* or -1, the object i* left or -1, whether j was the object freed by the iteration before); a
    stalled iteration is the one entry with a row and no freed object."""
    flag = _entries_flag(entries)
    if hasattr(mats, "cpu"):
        mats = mats.double().cpu().numpy()
    mats = np.asarray(mats)
    if mats.ndim != 3:
        raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.ndim}")
    B, N, M = mats.shape
    shp = np.tile([N, M], (B, 1)) if shapes is None else np.asarray(_host(shapes))
    sol = np.array(_host(sol), dtype=np.int32).reshape(B, N)
    prices = np.array(_host(prices), dtype=np.float64).reshape(B, M)
    eps_b = np.asarray(_host(final_eps)).astype(np.float64).reshape(B)
    maximize = problem != "min"
    o = None
    if outside is not None:
        o = np.asarray(_host(outside) if hasattr(outside, "cpu") else outside, dtype=np.float64)
        if o.shape not in ((), (B,), (B, N)):
            raise ValueError(f"outside must be a float or have shape ({B},) or ({B}, {N}), got {o.shape}")
        o = np.broadcast_to(o if o.ndim != 1 else o[:, None], (B, N))
        if outside_prices is None:
            raise ValueError("with outside, the solve's outside_prices are needed")
        outside_prices = np.array(_host(outside_prices), dtype=np.float64).reshape(B, N)
    out = dict(sol=sol, prices=prices)
    if o is not None:
        out["outside_prices"] = outside_prices
    its, left = np.full(B, -1, dtype=np.int64), np.full(B, -1, dtype=np.int32)
    obj64, ece, ran = np.full(B, np.nan), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=bool)
    run = None if run is None else np.asarray(run.cpu() if hasattr(run, "cpu") else run).astype(bool).reshape(B)
    for b in range(B):
        n, m = (int(x) for x in shp[b])
        if not (1 <= n <= N and 1 <= m <= M):
            continue
        p2o = sol[b, :n].astype(np.int64)
        if o is not None:
            p2o = np.where(p2o < 0, m + np.arange(n), p2o)
        if (p2o < 0).any() or (run is not None and not run[b]):
            continue
        v = mats[b, :n, :m].astype(np.float64)
        with np.errstate(invalid="ignore"):
            valid = ~np.isnan(v) if flag else v >= 0
        p = prices[b, :m].copy()
        if o is not None:
            d = np.zeros((n, n))
            d[np.arange(n), np.arange(n)] = o[b, :n]
            v, valid, p = np.hstack([v, d]), np.hstack([valid, np.eye(n, dtype=bool)]), np.concatenate([p, outside_prices[b, :n]])
        a = v if maximize else v * -1.0
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
            # eCE_satisfied at target_eps (auction_.pyx:443-485) and get_obj (:489-523), as the solve makes them
            teps = float(np.float32(1.0 / np.float64(n)))
            lhs = a[np.arange(n), p2o] - p[p2o] + 1e-7
            ece[b] = 0 if (valid & (lhs[:, None] < (a - p[None, :]) - teps)).any() else 1
            obj = 0.0
            for i in range(n):
                val = float(a[i, p2o[i]])
                obj = obj + val if maximize else obj - val
        obj64[b] = obj
    with np.errstate(over="ignore"):  # (an objective beyond float32 is +-inf there, as the kernel's cast gives it)
        obj32 = obj64.astype(np.float32)
    out.update(obj_f64=obj64, obj_f32=obj32, eCE=ece, reverse=dict(its=its, left=left), ran=ran)
    return out


def auction_solve_batch(mats, problem="min", eps_start=0., max_iter=1000000, fast=None, cardinality_check=True,
                        shapes=None, prices=None, errors="raise", mat_dtype="float64", outside=None, entries="nonneg",
                        finish=None):
    """Solve B independent dense problems in one call, one workgroup per problem.

    mats: float64 (or mat_dtype, below) (B, N, M), a numpy array or a tensor on the device (read in place, whatever its
    strides: see "strided stacks" below; ordered behind torch.cuda.current_stream()); entries v >= 0 are edges, anything else (-1, NaN) is not.  shapes: optional int
    (B, 2); problem b is then mats[b, :n_b, :m_b].  prices: optional float64 (B, M) starting prices (of the maximised
    problem) as AuctionSolver.resolve takes them.  N, M <= MISSLAP_DENSE_BATCH_MAX_DIM.

    Returns dict(sol=int32 (B, N) with -1 beyond n_b, prices=float64 (B, M) with 0 beyond m_b, meta=dict of length-B
    arrays).  Device input gives device tensors for sol and prices.  All or nothing: a failing problem raises
    ValueError("problem <b>: <what from_matrix raises for that slice>") and nothing is solved.  The caller's arrays are
    never written.

    errors="status": a verdict per problem instead.  The call only raises for what is wrong with the whole call; the
    result also holds status (int32 (B,), the MISSLAP_BATCH_STATUS_* codes of include/misslap.h) and matching_size
    (int32 (B,), the guard's cardinality, -1 where it did not run).  Every problem with status 0 is solved, with exactly
    the default mode's results; the others have sol -1, prices 0 and a meta of n_rows, n_cols, nnz and zeros.
    mat_dtype: "float64" (default), "float32", "float16" or "bfloat16", or that numpy / torch dtype: the element type of
    mats, which must have exactly that dtype (nothing is converted; a mismatch raises ValueError).  The stack is read in
    place in its own type and every value is widened to float64 as it is read, which is exact: the result is bit for
    bit the float64 result on the widened stack (mats.astype(float64) / mats.double()).  An entry is valid iff it is
    >= 0 in its own type.  prices and every output keep their types.  numpy has no bfloat16, so a bfloat16 stack is a
    device tensor.  Only this call and hopcroft_solve_batch(mats=) take the keyword: auction_solve(mat=), from_matrix
    and the sparse batch take float64.

    Strided stacks: a device tensor of any non-negative element strides is read where it lies -- cost.transpose(1, 2)
    (more rows than columns: the solver assigns every row and needs n <= m), a slice of a wider buffer
    (buf[:, r0:r0 + N, c0:c0 + M], buf[::2], a padded leading dimension) or one.expand(B, N, M) (the same costs from B
    starting prices or outside values; batch stride 0) -- in every mode, with shapes (which refer to the view), prices,
    fast, outside and all four mat_dtypes, and in hopcroft_solve_batch(mats=).  The result is bit for bit that of the
    same call on mats.contiguous(); nothing is copied or converted, only elements of the view are read, and the tensor's
    storage is never written (misslap_solve_dense_batch_status_strided / _outside_strided).  A contiguous tensor takes
    exactly the calls it always took, and a numpy array is uploaded through np.ascontiguousarray as before.  The default
    mode's own call (all or nothing, with a host guard that reads the stack back) is not taught strides: for a strided
    device stack errors="raise" runs the errors="status" call and then raise_for_status, which raises the default
    mode's message for the first failing problem, and returns the status-mode dict (device tensors; meta through
    batch_meta_to_host).

    raise_for_status(res) raises what the default mode would have raised.  With a device stack the call is
    stream-ordered: its kernels go onto torch.cuda.current_stream(mats.device), it waits for nothing, and sol, prices,
    status, matching_size and the meta fields are device tensors ordered on that stream (batch_meta_to_host(res) gives
    the default mode's meta dict).  shapes and prices may then be device tensors; a device shapes entry outside the
    stack gives MISSLAP_BATCH_STATUS_BAD_SHAPE.  The matching guard always runs on the device in this mode, which at
    B = 1 is slower than the default mode's host guard.

    outside: partial assignments (misslap_solve_dense_batch_outside).  A finite float >= 0, float64 (B,) or float64
    (B, N) -- a numpy array or, with a device stack, a contiguous tensor on the same device: the outside value of every
    row, in the units of the stack (problem="min": the cost of leaving row i unmatched; "max": the value of doing so),
    always float64 whatever mat_dtype is.  Problem b is then aug_b = hstack([mats[b, :n_b, :m_b], D_b]), D_b holding the
    outside values on its diagonal and -1 elsewhere, and its result is bit for bit
    auction_solve(mat=aug_b, ..., cardinality_check=False) on dense_to_augmented(mats, shapes, outside); with prices the
    solve starts from [p0[b, :m_b], zeros(n_b)].  sol[b, i] is the real column, or -1 where row i took its outside option
    (and beyond n_b, on a condemned problem, or where max_iter cut the solve).  prices stays (B, M), the real columns; the
    new key outside_prices is float64 (B, N), the price of row i's outside object and 0 beyond n_b (a row without any valid
    entry bids +inf as a one-entry row of the reference does, so its outside price is +inf).  meta is the augmented
    problem's record (n_cols = m_b + n_b, nnz = valid entries + n_b; n_assigned counts rows on their outside option).
    Both errors= modes run the same call and return the status-mode dict; "raise" then applies raise_for_status.  An
    outside value is an entry of a dense matrix: -0.0 is valid, +inf gives MISSLAP_BATCH_STATUS_INFINITE_VALUE, and a
    negative value or a NaN in a row < n_b -- an absent entry, "this row must be matched": not offered -- gives
    MISSLAP_BATCH_STATUS_BAD_OUTSIDE (15).  The checks, in their order: BAD_SHAPE, BAD_OUTSIDE, INFINITE_VALUE,
    PRICE_NOT_FINITE, PRICE_NEGATIVE.  TOO_FEW_VALUES, EMPTY_ROW and INFEASIBLE cannot occur: fully gated rows, graphs
    without a complete matching and n_b > m_b are solved; the guard is not launched whatever cardinality_check says and
    matching_size is -1.  The values of rows >= n_b are never read.

    entries: "nonneg" (default) is the rule above, v >= 0, and the call takes exactly the path it always took.
    entries="finite" is for signed costs (a matcher's -prob + L1 - GIoU, a tracker's log-likelihood ratio), read in
    place without a shift by the minimum: an element is an entry iff it is not a NaN in its own type, so negative values,
    -0.0 and subnormals are entries and NaN is the one way to say "no edge" (cost.masked_fill(~gate, float("nan"))).
    An entry of +inf or -inf gives MISSLAP_BATCH_STATUS_INFINITE_VALUE.  Everything else is unchanged: n_cols is the
    largest column with an entry plus 1, C = max |v|, the checks and their order, shapes, prices, fast, eps_start,
    max_iter, problem, mat_dtype, strides, outside.  A problem with status 0 is bit for bit
    auction_solve(loc=loc_b, val=val_b, ..., cardinality_check=False) on dense_to_packed(mats, shapes, "finite")[b] (fast:
    eps = 1 / n_b).  With outside, an outside value may be any finite float64 (a NaN gives BAD_OUTSIDE, an infinity
    INFINITE_VALUE) and problem b is sparse_to_augmented of the packed problem: one entry (i, m_b + i) more per row,
    stored last in its row.  errors="raise" runs the status call and then raise_for_status, as for a strided stack, and
    returns the status-mode dict.  A contiguous stack in this mode is read by the kernels of the strided family with its
    natural strides (misslap_options.mat_dtype | MISSLAP_DENSE_ENTRIES_FINITE).

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
    reverse-auction clean-up behind its forward solve (misslap_dense_batch_reverse_finish: one more launch on the same
    stream, one workgroup per problem, waiting for nothing): lambda = the smallest price of an assigned object, and every
    unassigned object priced above lambda takes the row that values it most or drops to lambda.  Afterwards the
    assignment still satisfies eps-CS at the solve's final eps and no unassigned object is priced above lambda: optimal
    within n_b * final_eps from any starting prices and with any fast / eps_start.  The result is exactly
    dense_reverse_finish (its docstring is the definition) applied to the outputs of the same call with finish=None:
    sol, prices and outside_prices are rewritten, meta obj / obj_f64 and eCE recomputed, every other meta field stays the
    forward solve's, and the result gains reverse=dict(its=int64 (B,), left=int32 (B,)): the iterations made (0 for a
    square problem) and the unassigned objects still priced above lambda (0 unless max_iter, which is also the finish's
    own budget, cut it, or a stalled iteration ended it: where eps is lost to rounding, outside
    max(|a|, |p|) * 2**-52 < final_eps, a move may not raise the moving row's profit; the finish then ends with left > 0
    while status stays 0 and eCE may be 1, so read left -- dense_reverse_finish has the rule); both -1 where the finish did not run -- status != 0, or max_iter cut the forward solve -- and
    nothing of such a problem is touched.  It combines with every other keyword and with strided views; both errors=
    modes run the status call, then the finish ("raise": then raise_for_status) and return the status-mode dict.  A numpy
    stack is uploaded once, takes the device route and comes back as numpy arrays (meta as batch_meta_to_host gives it).
    Cold solves should keep fast=True from zero prices: that needs no finish, and behind the reference's eps-scaling the
    finish has far more to repair than a cold single phase has to do.  Any other value raises ValueError.
    """
    if errors not in ("raise", "status"):
        raise ValueError(f"errors must be 'raise' or 'status', got {errors!r}")
    if finish is not None:
        if not isinstance(finish, str) or finish != "reverse":
            raise ValueError(f"finish must be None or 'reverse', got {finish!r}")
        return _solve_with_finish(mats, problem, eps_start, max_iter, fast, cardinality_check, shapes, prices, errors,
                                  mat_dtype, outside, entries)
    flag = _entries_flag(entries)
    B, N, M, on_device, dtype = _check_stack(mats, mat_dtype)
    dtype |= flag  # (the option word carries the rule: the element type OR-ed with MISSLAP_DENSE_ENTRIES_FINITE)
    strides = _stack_strides(mats, on_device)
    if N > MAX_DIM or M > MAX_DIM:
        raise ValueError(f"problems of {N} x {M}: auction_solve_batch takes at most {MAX_DIM} x {MAX_DIM} "
                         f"(MISSLAP_DENSE_BATCH_MAX_DIM); solve larger problems with from_matrix / solve_batch")
    if outside is not None:
        res = _solve_outside(mats, B, N, M, on_device, problem, eps_start, max_iter, fast, shapes, prices, dtype, outside,
                             strides)
        return raise_for_status(res) if errors == "raise" else res
    if fast is None:  # (resolved here: the library gets a plain flag)
        fast = False
    # (the default mode's own call reads a contiguous stack under the "nonneg" rule only)
    if errors == "status" or strides is not None or flag:
        res = _solve_status(mats, B, N, M, on_device, problem, eps_start, max_iter, fast, cardinality_check, shapes,
                            prices, dtype, strides)
        return res if errors == "status" else raise_for_status(res)
    shp = _check_shapes(shapes, B, N, M, "problem")
    ns = shp[:, 0] if shp is not None else np.full(B, N, dtype=np.int32)
    e = _eps(eps_start)
    p, p_ptr, _ = _starting_prices(prices, B, M, True, on_device, mats, "mats")  # (p lives through the call)
    eps_b = None
    if fast:  # auction_.pyx:568-569: eps_start = 1 / N of each problem, as a C float
        eps_b = (1.0 / ns.astype(np.float64)).astype(np.float32)
    opts = _solve_options(on_device, mats, problem, e, max_iter, dtype)
    dev = mats.device if on_device else None
    mc = mats if on_device else np.ascontiguousarray(mats)
    sol, pout = _empty((B, N), np.int32, dev), _empty((B, M), np.float64, dev)
    metas, info = _new_meta(B)
    _lib.check(_lib.load().misslap_solve_dense_batch(
        B, N, M, C.c_void_p(_ptr(mc)), _ptr(shp), _ptr(eps_b), None if p_ptr is None else C.c_void_p(p_ptr),
        1 if cardinality_check else 0, C.byref(opts), C.c_void_p(_ptr(sol)), C.c_void_p(_ptr(pout)),
        1 if on_device else 0, metas, C.byref(info)))
    return dict(sol=sol, prices=pout, meta=_decode_meta(metas, info))


def _shapes(shapes, B, N, M, dev):
    """shapes of a status-mode call.  With a device stack (dev) a device tensor is read where it lies; a host array is
    validated as in the default mode and then sent from pinned memory without a wait."""
    if dev is not None and _is_device_tensor(shapes):
        return _check_device_shapes(shapes, B, dev)
    return _send(_check_shapes(shapes, B, N, M, "problem"), dev)


def _prices(prices, B, M, mats, dev):
    """Starting prices of a status-mode call, float64 (B, M), where the stack lives: a host array is checked (dtype and
    shape) and with a device stack sent from pinned memory without a wait."""
    if isinstance(prices, np.ndarray):
        return _send(_starting_prices(prices, B, M, True, False, mats, "mats")[0], dev)
    return _starting_prices(prices, B, M, True, dev is not None, mats, "mats")[0]


def _solve_status(mats, B, N, M, on_device, problem, eps_start, max_iter, fast, cardinality_check, shapes, prices,
                  dtype, strides=None):
    """errors="status" of auction_solve_batch (misslap_solve_dense_batch_status; with the strides of a non-contiguous
    device stack its strided form); the whole-call checks in the default mode's order: shapes, eps_start, prices."""
    dev = mats.device if on_device else None
    check = 1 if cardinality_check else 0
    shp = _shapes(shapes, B, N, M, dev)
    opts = _solve_options(on_device, mats, problem, _eps(eps_start), max_iter, dtype)
    p = _prices(prices, B, M, mats, dev)
    mc = mats if on_device else np.ascontiguousarray(mats)
    lib = _lib.load()
    call = _StatusCall(lib, opts, B, N, M, None, dev, "misslap_dense_batch_workspace_bytes",
                       (B, N, M, 0 if p is None else 1, check))
    rest = (_ptr(mc), _ptr(shp), 1 if fast else 0, _ptr(p), check, *call.way, *call.outs)
    if strides is None:
        _lib.check(lib.misslap_solve_dense_batch_status(B, N, M, *rest))
    else:
        _lib.check(lib.misslap_solve_dense_batch_status_strided(B, N, M, *strides, *rest))
    return call.result((mats, shp, p), shapes=shp, stack=(N, M))


def _solve_outside(mats, B, N, M, on_device, problem, eps_start, max_iter, fast, shapes, prices, dtype, outside,
                   strides=None):
    """auction_solve_batch(outside=) in either mode (misslap_solve_dense_batch_outside; with the strides of a
    non-contiguous device stack its strided form): the result dict of the status mode plus outside_prices.  The whole-call checks in the status mode's order, then outside."""
    dev = mats.device if on_device else None
    shp = _shapes(shapes, B, N, M, dev)
    e = _eps(eps_start)
    p = _prices(prices, B, M, mats, dev)
    finite = bool(dtype & _lib.DENSE_ENTRIES_FINITE)  # (then an outside value may have either sign)
    out_v, out_ld = _check_outside(outside, B, N, dev, "mats", "mats", not finite)
    if fast is None:
        fast = not e > 0
    opts = _solve_options(on_device, mats, problem, e, max_iter, dtype)
    mc = mats if on_device else np.ascontiguousarray(mats)
    d_out = _send(out_v, dev)
    lib = _lib.load()
    call = _StatusCall(lib, opts, B, N, M, N, dev, "misslap_dense_batch_outside_workspace_bytes",
                       (B, N, M, 0 if p is None else 1))
    rest = (_ptr(mc), _ptr(shp), 1 if fast else 0, _ptr(p), *call.way, _ptr(d_out), out_ld, *call.outs)
    if strides is None:
        _lib.check(lib.misslap_solve_dense_batch_outside(B, N, M, *rest))
    else:
        _lib.check(lib.misslap_solve_dense_batch_outside_strided(B, N, M, *strides, *rest))
    own = dict(entries="finite") if finite else {}  # (raise_for_status words a bad outside value by the rule)
    return call.result((mats, shp, p, d_out), shapes=shp, stack=(N, M), outside=d_out, **own)


def _reverse_finish_launch(stack, res, problem, max_iter, dtype):
    """misslap_dense_batch_reverse_finish on the device result `res` of a status-mode call on the device stack `stack`
    (dtype: its option word), on the call's stream: res's outputs are rewritten in place and res gains `reverse`."""
    import torch
    B, N, M = (int(d) for d in stack.shape)
    dev = stack.device
    opts = _solve_options(True, stack, problem, 0.0, max_iter, dtype)
    with torch.cuda.device(dev):
        its, left = _empty(B, np.int64, dev), _empty(B, np.int32, dev)
    d_out = res.get("outside") if "outside_prices" in res else None
    _lib.check(_lib.load().misslap_dense_batch_reverse_finish(
        B, N, M, *(int(x) for x in stack.stride()), C.c_void_p(_ptr(stack)), _ptr(res["shapes"]), _ptr(d_out),
        0 if d_out is None or d_out.dim() == 1 else N, C.byref(opts), C.c_void_p(int(res["stream"].cuda_stream)),
        _ptr(res["status"]), _ptr(res["sol"]), _ptr(res["prices"]), _ptr(res.get("outside_prices")), _ptr(res["records"]),
        _ptr(its), _ptr(left)))
    res["reverse"] = dict(its=its, left=left)
    return its, left


def _solve_with_finish(mats, problem, eps_start, max_iter, fast, cardinality_check, shapes, prices, errors, mat_dtype,
                       outside, entries):
    """auction_solve_batch(finish="reverse"): the status-mode call of a device stack, then the reverse finish on its
    outputs -- one more launch on the call's stream (misslap_dense_batch_reverse_finish), nothing is waited for.  A numpy
    stack is uploaded once and its result brought back as numpy arrays."""
    flag = _entries_flag(entries)
    B, N, M, on_device, dtype = _check_stack(mats, mat_dtype)
    stack = mats
    if not on_device:
        import torch
        dev = torch.device("cuda", int(os.environ.get(_ENV_DEVICE, 0)))
        stack = torch.from_numpy(np.ascontiguousarray(mats)).to(dev)
    res = auction_solve_batch(stack, problem, eps_start, max_iter, fast, cardinality_check, shapes, prices, "status",
                              mat_dtype, outside, entries)
    its, left = _reverse_finish_launch(stack, res, problem, max_iter, dtype | flag)
    if not on_device:
        meta = batch_meta_to_host(res)  # (waits for the call's stream once)
        res = {k: v for k, v in res.items() if k not in ("records", "info", "stream", "keep")}
        res = {k: _host(v) if _is_device_tensor(v) else v for k, v in res.items()}
        res.update(meta=meta, reverse=dict(its=_host(its), left=_host(left)))
    return raise_for_status(res) if errors == "raise" else res


def _status_error(res, b, code, n, m, card):
    """The exception of problem b of a dense result: what the default mode raises for that slice (n: the record's
    n_rows; card: its matching_size)."""
    N, M = res["stack"]
    m = 0  # (only a bad shape names its columns)
    if code == _lib.BATCH_STATUS_BAD_SHAPE:
        n, m = (int(x) for x in _host(res["shapes"])[b])
    row, value = 0, 0.0
    if code == _lib.BATCH_STATUS_BAD_OUTSIDE:  # the first row < n_b whose outside value is no entry
        o = _host(res["outside"])[b]
        o = np.broadcast_to(o, (n,)) if o.ndim == 0 else o[:n]
        finite = res.get("entries") == "finite"
        with np.errstate(invalid="ignore"):
            row = int(np.flatnonzero(np.isnan(o) if finite else ~(o >= 0))[0])
        value = float(o[row])
        if finite:  # (the one outside value this rule refuses)
            return ValueError(f"problem {b}: the outside value of row {row} is {value!r}: it must not be a NaN (a NaN "
                              "would be an absent entry)")
    text = _STATUS_TEXT[code].format(n=n, m=m, N=N, M=M, card=card, row=row, value=value)
    if code == _lib.BATCH_STATUS_INFINITE_VALUE and "outside_prices" in res:
        text += " (in an entry or in the outside value of a row)"
    return ValueError(f"problem {b}: {text}")


_STATUS_ERRORS["dense"] = _status_error

