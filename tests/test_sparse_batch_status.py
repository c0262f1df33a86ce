"""auction_solve_sparse_batch(errors="status") on the GPU (misslap_solve_sparse_batch_status): a verdict per problem, and
with loc / val on the device a call that is ordered on the caller's stream and, given dims, waits for nothing.

  parity    on batches without a defect every status is 0 and every problem is the oracle's result bit for bit (the
            comparison of tests/test_sparse_batch.py), from numpy arrays and from device tensors, with and without dims.
  verdicts  on the mixed batch of tests/_sparse_status_fixture.py status and matching_size are those the fixture derives
            on the CPU; status[b] is the code of what the DEFAULT mode raises for problem b alone; the healthy problems
            equal the oracle, the condemned ones have exactly the defined outputs, and raise_for_status raises the
            default mode's exception.
  safety    the packed arrays lie between +inf values at column indices beyond every carve, condemned neighbours hold
            indices up to INT_MAX, a problem beyond dims is TOO_LARGE and not solved; once more in a fresh process whose
            every device block is poisoned.
  no wait   with dims, behind >= 200 ms of queued work the call returns in less than a quarter of that time.
"""
import faulthandler
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from sslap_amd import auction_solve_sparse_batch, batch_meta_to_host, raise_for_status
from tests import _sparse_status_fixture as fxt
from tests._sparse_status_fixture import DIMS, expected_status, graph_is_clean, mixed_batch, pack
from tests.test_dense_batch_status import _busy
from tests.test_sparse_batch import CAP, _bits, _check_all, _check_problem, _pack, _problem

pytestmark = pytest.mark.gpu

ZERO_META = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "obj_f64", "start_eps", "final_eps",
             "start_eps_f32", "final_eps_f32", "bids_made")


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _to_host(res):
    """A status-mode result with numpy arrays and the default mode's meta dict, whichever way it was computed."""
    if isinstance(res["sol"], np.ndarray):
        return res
    meta = batch_meta_to_host(res)
    for k, v in res["meta"].items():  # the device views hold the same records
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), meta[k]), k
    return dict(res, sol=res["sol"].cpu().numpy(), prices=res["prices"].cpu().numpy(), status=res["status"].cpu().numpy(),
                matching_size=res["matching_size"].cpu().numpy(), meta=meta)


def _device(loc, val, pad=64):
    """loc / val on the device, between `pad` entries of +inf at column INT_MAX on either side"""
    import torch
    guard_l, guard_v = np.full((pad, 2), fxt.INT_MAX, dtype=np.int32), np.full(pad, np.inf)
    dl = torch.from_numpy(np.concatenate([guard_l, loc, guard_l])).cuda()[pad:pad + len(loc)]
    dv = torch.from_numpy(np.concatenate([guard_v, val, guard_v])).cuda()[pad:pad + len(val)]
    assert dl.is_contiguous() and dv.is_contiguous()
    return dl, dv


def _both(probs, prices=None, device_prices=False, **kw):
    """The same batch from numpy arrays and from device tensors (prices on the host, or on the device)."""
    import torch
    loc, val, offsets = _pack(probs)
    before = (loc.copy(), val.copy())
    yield auction_solve_sparse_batch(loc, val, offsets, prices=prices, errors="status", **kw)
    assert np.array_equal(loc, before[0]) and np.array_equal(_bits(val), _bits(before[1]))  # never written
    dl, dv = _device(loc, val)
    dp = prices if prices is None or not device_prices else torch.from_numpy(prices).cuda()
    res = auction_solve_sparse_batch(dl, dv, offsets, prices=dp, errors="status", **kw)
    for k in ("sol", "prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == dl.device, k
    yield _to_host(res)
    assert np.array_equal(dl.cpu().numpy(), loc) and np.array_equal(_bits(dv.cpu().numpy()), _bits(val))


def _parity(probs, problem, sizes=None, prices=None, cardinality_check=True, dims=None, device_prices=False, **kw):
    """Every problem of a batch without a defect: status 0, the guard's full cardinality, and the oracle's result."""
    n = np.array([int(lo[:, 0].max()) + 1 for lo, _ in probs])
    m = np.array([int(lo[:, 1].max()) + 1 for lo, _ in probs])
    for res in _both(probs, prices=prices, problem=problem, sizes=sizes, cardinality_check=cardinality_check, dims=dims,
                     device_prices=device_prices, **kw):
        assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
        assert np.array_equal(res["matching_size"], n if cardinality_check else np.full(len(probs), -1))
        want = dims if dims is not None else (min(n.max(), CAP), min(m.max(), CAP))
        assert res["sol"].shape == (len(probs), want[0]) and res["prices"].shape == (len(probs), want[1])
        _check_all(res, probs, problem, sizes=sizes, prices=prices, **kw)  # every problem, none left out


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("kind", ["uniform", "ints", "fp32"])
def test_parity_value_kinds(problem, kind):
    rng = np.random.default_rng(hash((problem, kind)) % 2**32)
    probs = [_problem(rng, int(rng.integers(5, 40)), 45, 6, kind) for _ in range(8)]
    _parity(probs, problem, cardinality_check=(kind != "ints"))
    _parity(probs, problem, dims=(48, 64))


@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(fast=True), dict(max_iter=1), dict(max_iter=7),
                                  dict(max_iter=7, problem="max")])
def test_parity_eps_fast_and_max_iter(opts):
    rng = np.random.default_rng(7)
    probs = [_problem(rng, int(rng.integers(20, 41)), 50, 8) for _ in range(5)]
    opts = dict(opts)
    problem = opts.pop("problem", "min")
    _parity(probs, problem, **opts)
    _parity(probs, problem, dims=(40, 50), **opts)  # the carve exactly as large as the largest problem may be


@pytest.mark.parametrize("device_prices", [False, True])
def test_parity_sizes_fast_and_starting_prices(device_prices):
    rng = np.random.default_rng(8)
    probs = [_problem(rng, 30, 40, 5) for _ in range(4)] + [_problem(rng, 7, 9, 3)]
    sizes = np.array([[40, 30], [40, 17], [3, 30], [40, 12], [9, 7]])
    p0 = rng.uniform(0, 20, (5, 44))
    p0[1] = 0.0
    p0[2, ::3] = 0.0
    for problem in ("min", "max"):
        _parity(probs, problem, sizes=sizes, fast=True)  # 1 / sizes[b][1] formed in the kernel
        _parity(probs, problem, fast=True, dims=(32, 40))  # 1 / max row
        _parity(probs, problem, sizes=sizes, prices=p0, eps_start=0.25, device_prices=device_prices)
        _parity(probs, problem, prices=p0, dims=(30, 41), device_prices=device_prices)
    # prices exactly as wide as the widest problem
    _parity(probs, "min", prices=np.ascontiguousarray(p0[:, :40]), device_prices=device_prices)


def test_parity_row_patterns():
    rng = np.random.default_rng(11)
    probs = [_problem(rng, 30, 30, 10, shuffle=True), _problem(rng, 30, 30, 10, shuffle=False)]
    loc, val = _problem(rng, 30, 30, 8, "ints")
    dup = rng.random(loc.shape[0]) < 0.3  # duplicate (i, j) entries, with other values, at the end of their row
    loc2 = np.concatenate([loc, loc[dup]])
    val2 = np.concatenate([val, val[dup] + rng.integers(-1, 2, int(dup.sum()))])
    order = np.argsort(loc2[:, 0], kind="stable")
    probs.append((np.ascontiguousarray(loc2[order]), np.ascontiguousarray(np.abs(val2[order]))))
    probs.append(_problem(rng, 20, 20, 1))       # one entry per row: +inf bids and prices
    probs.append(_problem(rng, 12, 300, 200))    # rows longer than 64 entries
    probs.append(_problem(rng, 10, 90, 30))      # rectangular n < m
    probs.append((np.array([[0, 0]], dtype=np.int32), np.array([3.0])))
    for problem in ("min", "max"):
        _parity(probs, problem)
        _parity(probs, problem, dims=(64, 512))


def test_parity_at_the_cap():
    rng = np.random.default_rng(3)
    probs = [_problem(rng, CAP, CAP, 16), _problem(rng, 3, 3, 3)]
    _parity(probs, "max", cardinality_check=False)
    _parity(probs, "max", dims=(CAP, CAP))


def test_more_problems_than_compute_units():
    rng = np.random.default_rng(13)
    probs = [_problem(rng, int(rng.integers(1, 17)), 16, 6, "ints") for _ in range(1024)]
    _parity(probs, "min", dims=(16, 16))


# ---- verdicts

_TEXTS = [(fxt.NO_ENTRIES, r"^problem 0: no entries$"), (fxt.TOO_FEW_VALUES, r"Fewer than -?\d+ valid values"),
          (fxt.INFEASIBLE, r"Maximum matching possible only involves"),
          (fxt.NEGATIVE_INDEX, r"negative row index|loc holds a negative row or column index"),
          (fxt.ROWS_UNSORTED, r"rows must be sorted in ascending order \(auction_"),
          (fxt.ROW_GAP, r"every row 0\.\.N-1 must have"), (fxt.INFINITE_VALUE, r"val holds a NaN or an infinity"),
          (fxt.TOO_LARGE, r"exceeds MISSLAP_SPARSE_BATCH_MAX_DIM|column index too large"),
          (fxt.PRICES_TOO_NARROW, r"^prices must have shape"), (fxt.PRICE_NOT_FINITE, r"prices hold a NaN or an infinity"),
          (fxt.PRICE_NEGATIVE, r"prices must be >= 0")]


def _alone(fx, b, widen=False, **kw):
    """Problem b as a batch of its own: the arguments of auction_solve_sparse_batch.  widen: for the default mode, whose
    front-end wants prices as wide as the batch's largest column count clipped to the cap, as a whole-call check ahead
    of every per-problem one.  For a problem BEYOND the cap, which the library then rejects as too large, the prices
    get zero columns up to the cap so that the library is reached at all."""
    loc, val = fx["probs"][b]
    prices = fx["prices"][b:b + 1]
    if widen and len(loc) and loc[:, 1].max() >= CAP:
        prices = np.concatenate([prices, np.zeros((1, CAP - prices.shape[1]))], axis=1)
    return (loc, val, np.array([0, len(val)])), dict(sizes=fx["sizes"][b:b + 1], prices=prices, **kw)


def _default_mode_says(fx, b, fast, cardinality_check):
    """(status code, exception or None) of problem b, from what the DEFAULT mode does with that problem alone: with the
    call's own guard setting where the graph is clean and within the cap (the guard then judges the graph), without the
    guard elsewhere (the host guard would speak first, in its own words: the one documented difference)."""
    loc = fx["probs"][b][0]
    clean = graph_is_clean(loc) and loc.max(initial=0) < CAP
    args, kw = _alone(fx, b, widen=True, fast=fast, cardinality_check=cardinality_check and clean, max_iter=200)
    try:
        auction_solve_sparse_batch(*args, **kw)
    except ZeroDivisionError as e:
        assert str(e) == "problem 0: division by zero"
        return fxt.DIVISION_BY_ZERO, e
    except ValueError as e:
        codes = [c for c, pat in _TEXTS if re.search(pat, str(e))]
        assert len(codes) == 1, str(e)
        assert str(e).startswith("problem 0: ") or codes[0] == fxt.PRICES_TOO_NARROW, str(e)
        return codes[0], e
    return 0, None


def _check_verdicts(res, fx, want, want_size, dims, **kw):
    probs, sizes, prices = fx["probs"], fx["sizes"], fx["prices"]
    status, meta = res["status"], res["meta"]
    assert np.array_equal(status, want), [(b, status[b], want[b]) for b in np.flatnonzero(status != want)]
    assert np.array_equal(res["matching_size"], want_size), np.flatnonzero(res["matching_size"] != want_size)
    assert res["sol"].shape[1] == dims[0] and res["prices"].shape[1] == dims[1]
    for b, (loc, val) in enumerate(probs):
        if status[b] == 0:  # a healthy neighbour is intact: the oracle's result, bit for bit
            _check_problem(res, b, loc, val, "min", size=tuple(int(x) for x in sizes[b]), p0=prices[b], **kw)
            continue
        assert (res["sol"][b] == -1).all() and np.array_equal(_bits(res["prices"][b]), _bits(np.zeros(dims[1]))), b
        n_rows = n_cols = 0
        if len(loc):
            n_rows = min(max(int(loc[:, 0].max()) + 1, 0), fxt.INT_MAX)
            n_cols = min(max(int(loc[:, 1].max()) + 1, 0), fxt.INT_MAX)
        assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (n_rows, n_cols, len(loc)), b
        for k in ZERO_META:
            assert meta[k][b] == 0, (b, k)


def _expected_error(fx, b, said, dims):
    """What raise_for_status raises for problem b at index `at` of a batch: the default mode's exception for the problem
    alone, except where the default mode has no such check of its own (prices narrower than the batch are a whole-call
    error there, and it has no dims): the library's texts for those."""
    loc = fx["probs"][b][0]
    n, m = int(loc[:, 0].max()) + 1 if len(loc) else 0, int(loc[:, 1].max()) + 1 if len(loc) else 0
    code, exc = said
    if code == fxt.PRICES_TOO_NARROW:
        return ValueError, f"prices hold {fxt.P} columns, the problem has {m}"
    if exc is None:  # beyond dims only
        return ValueError, f"{n} x {m} does not fit sol_ld = {dims[0]} / prices_out_ld = {dims[1]}"
    return type(exc), str(exc)[len("problem 0: "):]


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("cardinality_check", [True, False])
def test_verdicts_on_the_mixed_batch(fast, cardinality_check):
    fx = mixed_batch()
    probs, sizes, prices = fx["probs"], fx["sizes"], fx["prices"]
    B = len(probs)
    kw = dict(fast=fast, cardinality_check=cardinality_check, max_iter=200)
    want, size = expected_status(probs, sizes, prices, fast=fast, cardinality_check=cardinality_check, dims=DIMS)
    wide, wide_size = expected_status(probs, sizes, prices, fast=fast, cardinality_check=cardinality_check)
    if fast and cardinality_check:
        assert np.array_equal(want, fx["kinds"]) and set(want) == set(fxt.ORDER) | {0}
    # each problem alone in the default mode (which has no dims) says what the CPU derivation says
    said = [_default_mode_says(fx, b, fast, cardinality_check) for b in range(B)]
    assert np.array_equal(np.array([c for c, _ in said]), wide)
    over = np.flatnonzero(want != wide)  # beyond DIMS and within the cap
    assert len(over) >= 2 and (want[over] == fxt.TOO_LARGE).all()

    # ... and so does the status mode for the problem alone, code and exception
    for b in range(1, B, 2):
        args, akw = _alone(fx, b, **kw)
        one = auction_solve_sparse_batch(*args, errors="status", **akw)
        assert one["status"][0] == wide[b] and one["matching_size"][0] == wide_size[b], b
        if wide[b] == 0:
            assert raise_for_status(one) is one
            continue
        kind, text = _expected_error(fx, b, said[b], None)
        with pytest.raises(kind) as e:
            raise_for_status(one)
        assert str(e.value) == "problem 0: " + text, b

    # the whole batch, from numpy arrays and from device tensors between guards, with dims and without
    loc, val, offsets = pack(probs)
    dl, dv = _device(loc, val)
    front = tuple(min(max(int(loc[:, c].max()) + 1, 1), CAP) for c in (0, 1))  # the outputs' widths without dims
    for dims, w, ws in ((DIMS, want, size), (None, wide, wide_size)):
        for a, b_ in ((loc, val), (dl, dv)):
            res = auction_solve_sparse_batch(a, b_, offsets, sizes=sizes, prices=prices, errors="status", dims=dims, **kw)
            host = _to_host(res)
            _check_verdicts(host, fx, w, ws, dims or front, **kw)
            first = int(np.flatnonzero(w)[0])
            kind, text = _expected_error(fx, first, said[first], dims)
            with pytest.raises(kind) as e:
                raise_for_status(res)
            assert str(e.value) == f"problem {first}: " + text
    # a problem beyond dims is TOO_LARGE and not solved; raise_for_status names the dims it did not fit
    b = int(over[0])
    sub = dict(probs=probs[b - 1:b + 2], sizes=sizes[b - 1:b + 2], prices=prices[b - 1:b + 2])
    res = auction_solve_sparse_batch(*_device(*pack(sub["probs"])[:2]), pack(sub["probs"])[2], sizes=sub["sizes"],
                                     prices=sub["prices"], errors="status", dims=DIMS, **kw)
    _check_verdicts(_to_host(res), sub, want[b - 1:b + 2], size[b - 1:b + 2], DIMS, **kw)
    with pytest.raises(ValueError, match=rf"^problem 1: \d+ x \d+ does not fit sol_ld = {DIMS[0]} / prices_out_ld = {DIMS[1]}$"):
        raise_for_status(res)
    # a result without a defect comes back as it is
    good = probs[0:16:2]
    res = auction_solve_sparse_batch(*_device(*_pack(good)[:2]), _pack(good)[2], errors="status", dims=DIMS)
    assert raise_for_status(res) is res


def test_default_mode_is_unchanged():
    fx = mixed_batch()
    loc, val, offsets = pack(fx["probs"])
    with pytest.raises(ValueError, match=r"^problem 1: no entries$"):
        auction_solve_sparse_batch(loc, val, offsets, sizes=fx["sizes"])
    with pytest.raises(ZeroDivisionError, match=r"^problem 3: division by zero$"):
        auction_solve_sparse_batch(loc, val, offsets, sizes=fx["sizes"], fast=True)
    with pytest.raises(ValueError, match="dims"):
        auction_solve_sparse_batch(loc, val, offsets, dims=DIMS)


def test_poisoned_device_blocks_change_nothing():
    """The mixed batch in a fresh process with MISSLAP_DEBUG_POISON=0xFF (every block the library hands out is filled with
    NaN / -1 patterns first; the numpy route takes its whole scratch from those): the same verdicts and outputs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys
for p in ({root!r}, {os.path.join(root, 'tests')!r}, {os.path.join(root, 'tests', 'golden')!r}):
    sys.path.insert(0, p)
import numpy as np
from tests import test_sparse_batch_status as t
fx = t.mixed_batch()
kw = dict(fast=True, cardinality_check=True, max_iter=200)
want, size = t.expected_status(fx['probs'], fx['sizes'], fx['prices'], fast=True, dims=t.DIMS)
loc, val, offsets = t.pack(fx['probs'])
for a, b in ((loc, val), t._device(loc, val)):
    for rep in range(2):  # (the second call takes the blocks the first one gave back)
        res = t.auction_solve_sparse_batch(a, b, offsets, sizes=fx['sizes'], prices=fx['prices'], errors='status',
                                           dims=t.DIMS, **kw)
        t._check_verdicts(t._to_host(res), fx, want, size, t.DIMS, **kw)
print('OK', int((want == 0).sum()))
"""
    env = dict(os.environ, MISSLAP_DEBUG_POISON="0xFF")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=280, env=env)
    assert p.returncode == 0 and "OK 72" in p.stdout, (p.stdout[-300:], p.stderr[-1500:])


# ---- the call does not wait

def _run_behind_busy_stream(stream):
    import torch
    rng = np.random.default_rng(31)
    probs = [_problem(rng, int(rng.integers(10, 48)), 48, 7) for _ in range(96)]
    loc, val, offsets = _pack(probs)
    sizes = np.array([[48, int(lo[:, 0].max()) + 1] for lo, _ in probs])
    p0 = rng.uniform(0, 5, (96, 48))
    kw = dict(sizes=sizes, fast=True, errors="status", dims=(48, 48))
    with torch.cuda.stream(stream):
        lsrc, vsrc, pd = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda(), torch.from_numpy(p0).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        lx, vx = lsrc.clone(), vsrc.clone()
        auction_solve_sparse_batch(lx, vx, offsets, prices=pd, **kw)  # the warm-up call
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
        res = auction_solve_sparse_batch(lx, vx, offsets, prices=pd, **kw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _to_host(res)
    assert (got["status"] == 0).all()
    _check_all(got, probs, "min", sizes=sizes, prices=p0, fast=True)


def test_the_call_does_not_wait_on_the_null_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.default_stream())


def test_the_call_does_not_wait_on_a_side_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.Stream())
