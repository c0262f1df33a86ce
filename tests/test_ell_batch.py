"""auction_solve_ell_batch on the GPU (misslap_solve_ell_batch): the batch solve from padded candidate lists, cols / vals
of shape (B, N, K) with negative columns as holes.

  parity        every problem is the oracle's result bit for bit on ell_to_packed's (loc_b, val_b) with
                size=(m_b, n_b) -- at the lane and second-slot edges of the wave scan (K = 1 .. 129), at the
                workgroup-size steps (N = 256, 257, 513), with holes between tied entries, repeated columns, short
                problems in a tall stack, both problems, `fast`, eps_start, max_iter and starting prices -- from numpy
                arrays and from device tensors, for every pair of index and value type.
  cross-layout  the same batch through auction_solve_sparse_batch(errors="status") on the packed form: identical outputs.
  verdicts      on the mixed batch of tests/_ell_fixture.py status and matching_size are those derived on the CPU; healthy
                problems equal the oracle, condemned ones have exactly the defined outputs; the default mode raises.
  safety        the device tensors are slices of larger buffers that hold column INT_MAX and +inf outside them, as do the
                rows beyond rows[b]; inputs are never written; once more in a fresh process whose device blocks are
                poisoned.
  no wait       with n_cols, behind >= 200 ms of queued work the call returns in less than a quarter of that time.
"""
import faulthandler
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from sslap_amd import (auction_solve_ell_batch, auction_solve_sparse_batch, batch_meta_to_host, ell_to_packed,
                       raise_for_status)
from tests import _ell_fixture as fxt
from tests._batch_shapes import (bits, sparse_compare, sparse_expect, sparse_pack, sparse_problem, sparse_problem_distinct,
                                 threads_for)
from tests.test_dense_batch_status import _busy

pytestmark = pytest.mark.gpu

ZERO_META = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "obj_f64", "start_eps", "final_eps",
             "start_eps_f32", "final_eps_f32", "bids_made")
DTYPE_IDS = ["i32-f64", "i64-f32", "i64-f64", "i32-f32"]


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _typed(cols, vals, itype, vtype):
    """The int64 / float64 stack in the call's types: for int32 a column beyond it becomes INT_MAX (as far beyond every
    bound), values are rounded to vtype (a hole's 1e300 becomes +inf: it is never interpreted)."""
    if itype is np.int32:
        cols = np.minimum(cols, fxt.INT_MAX)
    with np.errstate(over="ignore"):
        return np.array(cols, dtype=itype), np.array(vals, dtype=vtype)


def _to_host(res):
    """A result with numpy arrays and the host meta dict, whichever way it was computed."""
    if isinstance(res["sol"], np.ndarray):
        return res
    meta = batch_meta_to_host(res)
    for k, v in res["meta"].items():  # the device views hold the same records
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), meta[k]), k
    return dict(res, sol=res["sol"].cpu().numpy(), prices=res["prices"].cpu().numpy(), status=res["status"].cpu().numpy(),
                matching_size=res["matching_size"].cpu().numpy(), meta=meta)


def _device(cols, vals, pad=4096):
    """cols / vals on the device as slices of larger buffers: outside the slices cols is INT_MAX and vals is +inf."""
    import torch

    def inside(a, fill):
        buf = np.full(a.size + 2 * pad, fill, dtype=a.dtype)
        buf[pad:pad + a.size] = a.ravel()
        t = torch.from_numpy(buf).cuda()[pad:pad + a.size].view(a.shape)
        assert t.is_contiguous() and t.data_ptr() != t.untyped_storage().data_ptr()
        return t
    return inside(cols, fxt.INT_MAX), inside(vals, np.inf)


def _both(cols, vals, rows=None, prices=None, device_prices=False, n_cols=None, **kw):
    """The same batch from numpy arrays, and from device tensors (rows and prices on the host, or on the device)."""
    import torch
    before = (cols.copy(), vals.copy())
    yield auction_solve_ell_batch(cols, vals, rows=rows, prices=prices, n_cols=n_cols, errors="status", **kw)
    assert np.array_equal(cols, before[0]) and np.array_equal(vals.view(np.uint8), before[1].view(np.uint8))
    dc, dv = _device(cols, vals)
    dp = prices if prices is None or not device_prices else torch.from_numpy(np.array(prices)).cuda()
    dr = rows if rows is None or not device_prices else torch.from_numpy(np.array(rows)).cuda()
    res = auction_solve_ell_batch(dc, dv, rows=dr, prices=dp, n_cols=n_cols, errors="status", **kw)
    for k in ("sol", "prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == dc.device, k
    assert res["layout"] == "ell"
    yield _to_host(res)
    assert np.array_equal(dc.cpu().numpy(), cols)  # never written
    assert np.array_equal(dv.cpu().numpy().view(np.uint8), vals.view(np.uint8))


# ---- the parity cases: name -> (cols int64 (B, N, K), vals float64, rows or None), built once

def _ladder(K, n=40):
    """Three problems at K slots: distinct uniform columns, `ints` (ties; columns may repeat), and a short rectangular
    one; about a quarter of the slots are holes, except that the problems at K >= 64 include one without any."""
    rng = np.random.default_rng([21, K])
    k = 1 if K == 1 else max(K * 3 // 4, 2)
    m = max(n, K) + 7
    probs = [fxt.widen(*sparse_problem_distinct(rng, n, m, k, "uniform"), n, K, rng),
             fxt.widen(*sparse_problem(rng, n, m, k, "ints"), n, K, rng),
             fxt.widen(*sparse_problem(rng, n - 7, m + 30, K if K >= 64 else k, "uniform"), n - 7, K, rng)]
    return fxt.stack(probs, n, K, fill_col=fxt.INT_MAX, fill_val=np.inf)


def _tall(N, K, k):
    rng = np.random.default_rng([22, N, K])
    probs = [fxt.widen(*sparse_problem_distinct(rng, N, N, k, "uniform"), N, K, rng),
             fxt.widen(*sparse_problem(rng, N, N + 11, k, "ints"), N, K, rng)]
    return fxt.stack(probs, N, K)


def _short_rows(N=70, K=8):
    """rows of (1, 2, 63, N) in one batch; the rows beyond them hold column INT_MAX and +inf"""
    rng = np.random.default_rng([23])
    probs = [fxt.widen(*sparse_problem(rng, n, 80, 4, kind), n, K, rng)
             for n, kind in ((1, "uniform"), (2, "uniform"), (63, "ints"), (N, "uniform"))]
    return fxt.stack(probs, N, K, fill_col=fxt.INT_MAX, fill_val=np.inf)


def _repeated(N=30, K=12):
    """Every other row repeats one of its columns in its last hole: with another value (`ints`), or with the same value,
    a tie of the column with itself (`uniform`)."""
    rng = np.random.default_rng([24])
    probs = []
    for kind in ("ints", "uniform"):
        c, v = fxt.widen(*sparse_problem_distinct(rng, N, N + 5, 6, kind), N, K, rng)
        for i in range(0, N, 2):
            at = np.flatnonzero(c[i] >= 0)
            free = np.flatnonzero(c[i] < 0)
            src = at[int(rng.integers(len(at)))]
            c[i, free[-1]] = c[i, src]
            v[i, free[-1]] = v[i, src] + (1.0 if kind == "ints" else 0.0)  # (uniform: the same value twice, a tie)
        probs.append((c, v))
    return fxt.stack(probs, N, K)


CASES = {f"K{K}": functools.partial(_ladder, K) for K in (1, 8, 63, 64, 65, 129)}
CASES.update({f"N{N}": functools.partial(_tall, N, 8, 5) for N in (256, 257, 513)})
CASES["N257_K65"] = functools.partial(_tall, 257, 65, 40)
CASES["short_rows"] = _short_rows
CASES["repeated"] = _repeated


@functools.lru_cache(maxsize=None)
def _case(name):
    cols, vals, rows = CASES[name]()
    for a in (cols, vals, rows):
        a.setflags(write=False)
    return cols, vals, rows


@functools.lru_cache(maxsize=None)
def _expect(name, vtype, problem, opts=(), with_prices=False):
    """The oracle's result for every problem of a case whose values were rounded to vtype (then widened: exact)."""
    cols, vals, rows = _case(name)
    _, v = _typed(cols, vals, np.int64, vtype)
    p0 = _prices(name) if with_prices else None
    out = []
    for b, (loc, val) in enumerate(ell_to_packed(cols, v, rows)):
        assert loc.shape[0] >= rows[b] and np.isfinite(val).all()
        out.append(sparse_expect(loc, val, problem, size=(int(loc[:, 1].max()) + 1, int(rows[b])),
                                 p0=None if p0 is None else p0[b], **dict(opts)))
    return out


@functools.lru_cache(maxsize=None)
def _prices(name):
    cols = _case(name)[0]
    p = np.random.default_rng([25]).uniform(0, 20, (cols.shape[0], int(cols[cols < fxt.INT_MAX].max()) + 4))
    p[0, ::3] = 0.0
    p.setflags(write=False)
    return p


def _parity(name, problem, opts=(), with_prices=False, dtypes=fxt.DTYPES, with_n_cols=(False, True)):
    cols64, vals64, rows = _case(name)
    B, N, K = cols64.shape
    m = int(cols64[cols64 < fxt.INT_MAX].max()) + 1
    p0 = _prices(name) if with_prices else None
    for k, (itype, vtype) in enumerate(dtypes):
        cols, vals = _typed(cols64, vals64, itype, vtype)
        want = _expect(name, vtype, problem, opts, with_prices)
        n_cols = m + 3 if with_n_cols[k % len(with_n_cols)] else None
        for res in _both(cols, vals, rows=rows, prices=p0, device_prices=bool(k % 2), n_cols=n_cols, problem=problem,
                         **dict(opts)):
            assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
            assert np.array_equal(res["matching_size"], rows)  # the guard matched every row of every problem
            # (without n_cols: the maximum of the whole of cols, the rows beyond rows[b] included, clipped to the cap)
            assert res["sol"].shape == (B, N) and res["prices"].shape == (B, n_cols or min(int(cols64.max()) + 1, fxt.CAP))
            assert res["meta"]["gpu"]["threads"] == threads_for(N)
            for b in range(B):
                sparse_compare(res, b, want[b])
                assert want[b]["N"] == rows[b]


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("K")])
def test_parity_at_the_lane_and_slot_edges(name, problem):
    cols, _, rows = _case(name)
    K = cols.shape[2]
    valid = np.stack([cols[b, :rows[b]] >= 0 for b in (0, 1)])
    assert valid[..., K - 1].any() and valid[..., 0].any()  # the first and the last slot hold entries somewhere
    if K > 1:
        assert (~valid[..., K - 1]).any() and (~valid[..., 0]).any() and (~valid[..., 1:K - 1]).any()  # ... and holes
    _parity(name, problem)


@pytest.mark.parametrize("name", ["N256", "N257", "N513", "N257_K65"])
def test_parity_at_the_workgroup_size_steps(name):
    _parity(name, "min", dtypes=fxt.DTYPES[:2])
    _parity(name, "max", dtypes=fxt.DTYPES[2:])


def _tied_across_a_hole(cols, vals, rows, problem):
    """Whether some row holds its best value twice with a hole between the two slots."""
    for b in range(cols.shape[0]):
        for i in range(int(rows[b])):
            ok = cols[b, i] >= 0
            v = vals[b, i][ok]
            at = np.flatnonzero(ok)[v == (v.max() if problem == "max" else v.min())]
            if len(at) >= 2 and (~ok[at[0]:at[-1]]).any():
                return True
    return False


@pytest.mark.parametrize("problem", ["min", "max"])
def test_parity_with_holes_between_tied_entries_and_repeated_columns(problem):
    for name in ("K8", "repeated", "short_rows"):
        cols, vals, rows = _case(name)
        assert _tied_across_a_hole(cols, vals, rows, problem), name
    cols, _, rows = _case("repeated")
    assert all(len(np.unique(c[c >= 0])) < (c >= 0).sum() for c in cols[0, ::2])  # a repeated column
    _parity("repeated", problem)
    _parity("short_rows", problem)
    assert list(_case("short_rows")[2]) == [1, 2, 63, 70]


@pytest.mark.parametrize("opts", [dict(fast=True), dict(eps_start=0.5), dict(max_iter=0), dict(max_iter=1),
                                  dict(max_iter=7)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_parity_fast_eps_and_max_iter(opts):
    key = tuple(sorted(opts.items()))
    _parity("K8", "min", key, dtypes=fxt.DTYPES[:2])
    _parity("short_rows", "max", key, dtypes=fxt.DTYPES[2:])  # fast: 1 / n_b of each problem, n_b = 1 included


@pytest.mark.parametrize("problem", ["min", "max"])
def test_parity_with_starting_prices(problem):
    _parity("K8", problem, with_prices=True)
    _parity("K65", problem, (("eps_start", 0.25),), with_prices=True, dtypes=fxt.DTYPES[1:3])


def test_without_the_guard_and_more_problems_than_compute_units():
    rng = np.random.default_rng(26)
    probs = [fxt.widen(*sparse_problem(rng, int(n), 16, 3, "ints"), int(n), 5, rng) for n in rng.integers(1, 17, 1024)]
    cols, vals, rows = fxt.stack(probs, 16, 5)
    want = [sparse_expect(loc, val, "min", size=(int(loc[:, 1].max()) + 1, int(rows[b])))
            for b, (loc, val) in enumerate(ell_to_packed(cols, vals, rows))]
    for guard in (True, False):
        for res in _both(*_typed(cols, vals, np.int64, np.float32), rows=rows, n_cols=16, cardinality_check=guard):
            assert (res["status"] == 0).all()
            assert np.array_equal(res["matching_size"], rows if guard else np.full(1024, -1))
            for b in range(1024):
                sparse_compare(res, b, want[b])


# ---- cross-layout: the one test that needs no oracle

@pytest.mark.parametrize("name", ["K65", "short_rows", "repeated"])
def test_same_outputs_as_the_sparse_batch_on_the_packed_form(name):
    cols64, vals64, rows = _case(name)
    B, N, K = cols64.shape
    cols, vals = _typed(cols64, vals64, np.int64, np.float64)
    packed = ell_to_packed(cols, vals, rows)
    sizes = np.array([[int(loc[:, 1].max()) + 1, int(rows[b])] for b, (loc, _) in enumerate(packed)])
    M = int(sizes[:, 0].max())
    p0 = _prices(name)
    for kw in (dict(), dict(fast=True, problem="max"), dict(prices=p0, max_iter=9)):
        ref = auction_solve_sparse_batch(*sparse_pack(packed), sizes=sizes, errors="status", dims=(N, M), **kw)
        for res in _both(cols, vals, rows=rows, n_cols=M, **kw):
            for k in ("sol", "status", "matching_size"):
                assert np.array_equal(res[k], ref[k]), k
            assert np.array_equal(bits(res["prices"]), bits(ref["prices"]))
            for k, v in ref["meta"].items():
                if k not in ("timer", "gpu"):
                    assert np.array_equal(np.asarray(res["meta"][k]).view(np.uint8), np.asarray(v).view(np.uint8)), k


# ---- verdicts

def _check_verdicts(res, cols, vals, rows, prices, want, want_size, counts, n_cols, expect):
    status, meta = res["status"], res["meta"]
    assert np.array_equal(status, want), [(b, status[b], want[b]) for b in np.flatnonzero(status != want)]
    assert np.array_equal(res["matching_size"], want_size), np.flatnonzero(res["matching_size"] != want_size)
    assert res["sol"].shape == (cols.shape[0], cols.shape[1]) and res["prices"].shape[1] == n_cols
    for b in range(cols.shape[0]):
        if status[b] == 0:  # a healthy neighbour is intact: the oracle's result, bit for bit
            sparse_compare(res, b, expect[b])
            continue
        assert (res["sol"][b] == -1).all() and np.array_equal(bits(res["prices"][b]), bits(np.zeros(n_cols))), b
        assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == tuple(counts[b]), b
        for k in ZERO_META:
            assert meta[k][b] == 0, (b, k)


@functools.lru_cache(maxsize=None)
def _mixed_expect(vtype, cardinality_check, max_iter=200):
    fx = fxt.mixed_batch()
    cols, vals = _typed(fx["cols"], fx["vals"], np.int64, vtype)
    want, size, counts = fxt.expected_status(cols, vals, fx["rows"], fxt.MIXED_COLS, fx["prices"], cardinality_check)
    packed = ell_to_packed(cols, vals, fx["rows"].clip(0, cols.shape[1]))
    expect = [sparse_expect(packed[b][0], packed[b][1], "min", size=(int(counts[b, 1]), int(counts[b, 0])),
                            p0=fx["prices"][b], max_iter=max_iter) if want[b] == 0 else None for b in range(len(want))]
    return want, size, counts, expect


@pytest.mark.parametrize("dtypes", fxt.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cardinality_check", [True, False])
def test_verdicts_on_the_mixed_batch(dtypes, cardinality_check):
    fx = fxt.mixed_batch()
    rows, prices = fx["rows"], fx["prices"]
    cols, vals = _typed(fx["cols"], fx["vals"], *dtypes)
    want, size, counts, expect = _mixed_expect(dtypes[1], cardinality_check)
    # (the rounding to float32 and the clipping of 2^31 + 5 to INT_MAX change no verdict and no count)
    assert np.array_equal(want, fxt.expected_status(cols, vals, rows, fxt.MIXED_COLS, prices, cardinality_check)[0])
    if cardinality_check:
        assert np.array_equal(want, fx["kinds"])
    for res in _both(cols, vals, rows=rows, prices=prices, device_prices=dtypes[0] is np.int64, n_cols=fxt.MIXED_COLS,
                     cardinality_check=cardinality_check, max_iter=200):
        _check_verdicts(res, cols, vals, rows, prices, want, size, counts, fxt.MIXED_COLS, expect)
    # the default mode runs the same call and raises for the first bad problem
    for a, b in ((cols, vals), _device(cols, vals)):
        with pytest.raises(ValueError, match=r"^problem 1: rows = 0 outside 1 \.\. 24$"):
            auction_solve_ell_batch(a, b, rows=rows, prices=prices, n_cols=fxt.MIXED_COLS,
                                    cardinality_check=cardinality_check, max_iter=200)


_TEXTS = {fxt.BAD_SHAPE: r"rows = -?\d+ outside 1 \.\. 24", fxt.EMPTY_ROW: r"every row 0\.\.N-1 must have at least one entry",
          fxt.INFINITE_VALUE: r"val holds a NaN or an infinity",
          fxt.TOO_LARGE: r"\d+ x \d+ does not fit n_cols = 40|column index too large",
          fxt.PRICES_TOO_NARROW: r"prices hold 36 columns, the problem has 38",
          fxt.INFEASIBLE: r"Matrix is infeasible \(Maximum matching possible only involves \d+ out of 11 rows\.\)",
          fxt.PRICE_NOT_FINITE: r"prices hold a NaN or an infinity", fxt.PRICE_NEGATIVE: r"prices must be >= 0"}


def test_each_condemned_problem_alone_raises_its_own_text():
    """Each condemned problem of the mixed batch behind one healthy neighbour: the same verdict as in the batch, and the
    default mode (and raise_for_status) name the failed check with the `problem <b>: ` prefix."""
    fx = fxt.mixed_batch()
    want = fx["kinds"]
    for b in np.flatnonzero(want):
        sl = slice(b - 1, b + 1)
        args = (fx["cols"][sl], fx["vals"][sl])
        kw = dict(rows=fx["rows"][sl], prices=fx["prices"][sl], n_cols=fxt.MIXED_COLS, max_iter=200)
        res = auction_solve_ell_batch(*args, errors="status", **kw)
        assert list(res["status"]) == [0, want[b]], b
        for call in (lambda: raise_for_status(res), lambda: auction_solve_ell_batch(*args, **kw)):
            with pytest.raises(ValueError, match=r"^problem 1: (" + _TEXTS[int(want[b])] + ")"):
                call()
    good = auction_solve_ell_batch(fx["cols"][::2], fx["vals"][::2], rows=fx["rows"][::2], n_cols=fxt.MIXED_COLS)
    assert (good["status"] == 0).all() and raise_for_status(good) is good  # nothing to raise: the result comes back


@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_single_defects(itype):
    n, K = 6, 4
    cols = np.full((1, n, K), -1, dtype=np.int64)
    vals = np.full((1, n, K), np.nan)
    for i in range(n):  # row i: column i in slot i % K, and column (i + 1) % n behind it where a slot is left
        cols[0, i, i % K], vals[0, i, i % K] = i, 1.0 + i
        if i % K + 1 < K:
            cols[0, i, i % K + 1], vals[0, i, i % K + 1] = (i + 1) % n, 7.5 - i
    (loc, val), = ell_to_packed(cols, vals)
    want = sparse_expect(loc, val, "min", size=(n, n))

    def run(c, v=vals, **kw):
        out = [_to_host(auction_solve_ell_batch(*pair, errors="status", **kw))
               for pair in ((c.astype(itype), v), _device(c.astype(itype), v.astype(np.float32)))]
        for k in ("status", "matching_size", "sol"):
            assert np.array_equal(out[0][k], out[1][k]), k
        return out[0]

    # NaN (and infinities, and huge values) in holes condemn nothing: the problem is solved, and equals the oracle
    res = run(cols)
    assert res["status"][0] == 0 and res["matching_size"][0] == n
    sparse_compare(res, 0, want)
    assert res["prices"].shape == (1, n)  # without n_cols: the maximum of cols
    # a column equal to n_cols is too large, one below it is not
    assert run(cols, n_cols=n)["status"][0] == 0
    res = run(cols, n_cols=n - 1)
    assert res["status"][0] == fxt.TOO_LARGE and res["matching_size"][0] == -1
    assert (res["meta"]["n_rows"][0], res["meta"]["n_cols"][0], res["meta"]["nnz"][0]) == (n, n, len(val))
    # a NaN in an entry does condemn
    bad = vals.copy()
    bad[0, 2, 2] = np.nan
    assert cols[0, 2, 2] >= 0 and run(cols, v=bad)["status"][0] == fxt.INFINITE_VALUE
    # two rows whose only entry is the same column: infeasible, all rows but one matched
    same = cols.copy()
    same[0, 4], same[0, 5] = -1, -1
    same[0, 4, 3], same[0, 5, 0] = 4, 4
    v2 = vals.copy()
    v2[0, 4, 3], v2[0, 5, 0] = 1.0, 2.0
    res = run(same, v=v2)
    assert res["status"][0] == fxt.INFEASIBLE and res["matching_size"][0] == n - 1
    assert run(same, v=v2, cardinality_check=False, max_iter=20)["status"][0] == 0  # (unguarded: rounds until max_iter)
    with pytest.raises(ValueError, match=rf"^problem 0: Matrix is infeasible \(Maximum matching possible only involves "
                                         rf"{n - 1} out of {n} rows\.\)$"):
        auction_solve_ell_batch(same.astype(itype), v2)
    # the largest int32, and beyond it: too large, not a hole and not a small column
    big = cols.copy()
    big[0, 3, 3] = fxt.INT_MAX if itype is np.int32 else 2**31 + 5
    for kw in (dict(), dict(n_cols=fxt.CAP), dict(n_cols=n)):
        res = run(big, **kw)
        assert res["status"][0] == fxt.TOO_LARGE and res["meta"]["n_cols"][0] == fxt.INT_MAX, kw
        assert res["meta"]["nnz"][0] == len(val) and (res["sol"] == -1).all()
    with pytest.raises(ValueError, match=r"^problem 0: column index too large"):
        auction_solve_ell_batch(big.astype(itype), vals)


# ---- safety

def test_poisoned_device_blocks_change_nothing():
    """The mixed batch in a fresh process with MISSLAP_DEBUG_POISON=0xFF (every block the library hands out is filled with
    NaN / -1 patterns first; the numpy route takes its whole scratch from those): the same verdicts and outputs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys
for p in ({root!r}, {os.path.join(root, 'tests')!r}, {os.path.join(root, 'tests', 'golden')!r}):
    sys.path.insert(0, p)
import numpy as np
from tests import test_ell_batch as t
fx = t.fxt.mixed_batch()
for dtypes in t.fxt.DTYPES[:2]:
    cols, vals = t._typed(fx['cols'], fx['vals'], *dtypes)
    want, size, counts, expect = t._mixed_expect(dtypes[1], True)
    for rep in range(2):  # (the second call takes the blocks the first one gave back)
        for res in t._both(cols, vals, rows=fx['rows'], prices=fx['prices'], n_cols=t.fxt.MIXED_COLS, max_iter=200):
            t._check_verdicts(res, cols, vals, fx['rows'], fx['prices'], want, size, counts, t.fxt.MIXED_COLS, expect)
print('OK', int((want == 0).sum()))
"""
    env = dict(os.environ, MISSLAP_DEBUG_POISON="0xFF")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=280, env=env)
    n_ok = int((fxt.mixed_batch()["kinds"] == 0).sum())
    assert p.returncode == 0 and f"OK {n_ok}" in p.stdout, (p.stdout[-300:], p.stderr[-1500:])


# ---- the call does not wait

def _run_behind_busy_stream(stream):
    import torch
    rng = np.random.default_rng(31)
    B, N, K, M = 96, 48, 8, 48
    probs = [fxt.widen(*sparse_problem(rng, int(n), M, 5), int(n), K, rng) for n in rng.integers(10, N + 1, B)]
    cols, vals, rows = fxt.stack(probs, N, K)
    vals = np.where(cols >= 0, vals, -1.0)  # (finite everywhere: the NaN fill below is then the only source of a status 3)
    p0 = rng.uniform(0, 5, (B, M))
    want = [sparse_expect(loc, val, "min", size=(int(loc[:, 1].max()) + 1, int(rows[b])), p0=p0[b], fast=True)
            for b, (loc, val) in enumerate(ell_to_packed(cols, vals, rows))]
    kw = dict(n_cols=M, fast=True, errors="status")
    with torch.cuda.stream(stream):
        csrc, vsrc = torch.from_numpy(cols).cuda(), torch.from_numpy(vals).cuda()
        pd, rd = torch.from_numpy(p0).cuda(), torch.from_numpy(rows).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        cx, vx = csrc.clone(), vsrc.clone()
        auction_solve_ell_batch(cx, vx, rows=rd, prices=pd, **kw)  # the warm-up call
        _busy(w, 2)
        torch.cuda.synchronize()
        # the length of the queue: sized from a short chain, then measured on the chain the call will wait behind
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        _busy(w, 8)
        e[1].record()
        torch.cuda.synchronize()
        reps = int(np.ceil(8 * 400.0 / e[0].elapsed_time(e[1])))
        e[2].record()
        _busy(w, reps)
        e[3].record()
        torch.cuda.synchronize()
        D = e[2].elapsed_time(e[3])
        assert D >= 200.0, D
        vx.fill_(float("nan"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(w, reps)
        vx.copy_(vsrc, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_ell_batch(cx, vx, rows=rd, prices=pd, **kw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _to_host(res)
    assert (got["status"] == 0).all() and np.array_equal(got["matching_size"], rows)
    for b in range(B):
        sparse_compare(got, b, want[b])


def test_the_call_does_not_wait_on_the_null_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.default_stream())


def test_the_call_does_not_wait_on_a_side_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.Stream())
