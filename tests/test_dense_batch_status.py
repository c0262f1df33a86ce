"""auction_solve_batch(errors="status") on the GPU (misslap_solve_dense_batch_status): a verdict per problem, and with a
device stack a call that is ordered on the caller's stream and waits for nothing.

  parity    on batches without a defect every status is 0 and every slice is the oracle's result bit for bit (the
            comparison of tests/test_dense_batch.py), from a numpy stack and from a device stack.
  verdicts  on the mixed batch of tests/_status_fixture.py status[b] is the code of the error the DEFAULT mode raises
            for problem b alone, the healthy problems equal the oracle, the condemned ones have exactly the defined
            outputs, and raise_for_status raises what the default mode raises for the batch.
  no wait   behind >= 200 ms of queued work the call returns in less than a quarter of that time.
"""
import faulthandler
import re
import time

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, batch_meta_to_host, raise_for_status
from tests._status_fixture import expected_status, mixed_batch
from tests.test_dense_batch import _bits, _check_all, _check_problem, _values

pytestmark = pytest.mark.gpu


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
    return dict(sol=res["sol"].cpu().numpy(), prices=res["prices"].cpu().numpy(), status=res["status"].cpu().numpy(),
                matching_size=res["matching_size"].cpu().numpy(), meta=meta)


def _both(mats, shapes=None, prices=None, device_shapes=False, **kw):
    """The same batch from a numpy stack and from a device stack (shapes / prices on the host, or on the device)."""
    import torch
    yield auction_solve_batch(mats, shapes=shapes, prices=prices, errors="status", **kw)
    d = torch.from_numpy(mats).cuda()
    ds = shapes if shapes is None or not device_shapes else torch.from_numpy(np.ascontiguousarray(shapes, np.int32)).cuda()
    dp = prices if prices is None or not device_shapes else torch.from_numpy(prices).cuda()
    res = auction_solve_batch(d, shapes=ds, prices=dp, errors="status", **kw)
    for k in ("sol", "prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == d.device, k
    yield _to_host(res)


def _parity(mats, problem, shapes=None, prices=None, cardinality_check=True, device_shapes=False, **kw):
    for res in _both(mats, shapes=shapes, prices=prices, problem=problem, cardinality_check=cardinality_check,
                     device_shapes=device_shapes, **kw):
        assert res["status"].dtype == np.int32 and (res["status"] == 0).all()
        n = np.full(len(mats), mats.shape[1]) if shapes is None else np.asarray(shapes)[:, 0]
        assert np.array_equal(res["matching_size"], n if cardinality_check else np.full(len(mats), -1))
        _check_all(res, mats, problem, shapes=shapes, prices=prices, **kw)


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("kind", ["uniform", "ints", "fp32", "holes"])
def test_parity_value_kinds(problem, kind):
    rng = np.random.default_rng(hash((problem, kind)) % 2**32)
    _parity(_values(kind, (6, 24, 31), rng), problem, cardinality_check=(kind != "ints"))


@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(fast=True), dict(max_iter=1), dict(max_iter=7),
                                  dict(max_iter=7, problem="max"), dict(max_iter=0)])
def test_parity_eps_and_max_iter(opts):
    rng = np.random.default_rng(7)
    opts = dict(opts)
    _parity(_values("uniform", (5, 40, 40), rng), opts.pop("problem", "min"), **opts)


@pytest.mark.parametrize("device_shapes", [False, True])
def test_parity_mixed_shapes_fast_and_prices(device_shapes):
    rng = np.random.default_rng(5)
    B, N, M = 9, 30, 40
    shapes = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1)
    shapes[:, 1] = np.maximum(shapes[:, 1], shapes[:, 0])
    mats = np.full((B, N, M), np.inf)  # +inf would be reported if it were read
    for b, (n, m) in enumerate(shapes):
        mats[b, :n, :m] = _values("holes" if b % 3 == 0 else "uniform", (n, m), rng)
    p0 = rng.uniform(0, 20, (B, M))
    p0[1] = 0.0
    for problem in ("min", "max"):
        _parity(mats, problem, shapes=shapes, device_shapes=device_shapes)
        _parity(mats, problem, shapes=shapes, device_shapes=device_shapes, fast=True)  # 1 / n_b formed in the kernel
        _parity(mats, problem, shapes=shapes, prices=p0, device_shapes=device_shapes, eps_start=0.25)


def test_parity_cap_shape():
    rng = np.random.default_rng(3)
    _parity(_values("ints", (1, 1024, 1024), rng), "max", cardinality_check=False)
    _parity(_values("uniform", (2, 1, 1), rng), "max")


# ---- verdicts

_TEXTS = [(1, r"Fewer than \d+ valid values"), (2, r"every row must have"), (3, r"val holds a NaN or an infinity"),
          (4, r"Maximum matching possible only involves"), (5, r"prices hold a NaN or an infinity"),
          (6, r"prices must be >= 0"), (7, r"shape \(-?\d+, -?\d+\) outside")]


def _default_mode_code(mats, shapes, prices, b, **kw):
    """The status code of problem b, from what the DEFAULT mode does with that problem alone."""
    try:
        auction_solve_batch(mats[b:b + 1], shapes=shapes[b:b + 1], prices=prices[b:b + 1], **kw)
    except ValueError as e:
        msg = str(e)
        assert msg.startswith("problem 0: "), msg
        codes = [c for c, pat in _TEXTS if re.search(pat, msg)]
        assert len(codes) == 1, msg
        return codes[0], msg
    return 0, None


def _check_verdicts(res, mats, shapes, prices, want, cardinality_check=True):
    B, N, M = mats.shape
    status, meta = res["status"], res["meta"]
    assert np.array_equal(status, want), np.flatnonzero(status != want)
    _, size = expected_status(mats, shapes, prices, cardinality_check)
    assert np.array_equal(res["matching_size"], size)
    for b in range(B):
        n, m = int(shapes[b, 0]), int(shapes[b, 1])
        if status[b] == 0:
            _check_problem(res, b, mats[b, :n, :m], "min", n, m, p0=prices[b])
            continue
        assert (res["sol"][b] == -1).all() and np.array_equal(_bits(res["prices"][b]), _bits(np.zeros(M))), b
        if status[b] == 7:
            n_rows = n_cols = nnz = 0
        else:
            with np.errstate(invalid="ignore"):
                valid = mats[b, :n, :m] >= 0
            n_rows, nnz = n, int(valid.sum())
            n_cols = int(np.flatnonzero(valid.any(axis=0)).max()) + 1 if nnz else 0
        assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (n_rows, n_cols, nnz), b
        for k in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "obj_f64", "start_eps", "final_eps",
                  "start_eps_f32", "final_eps_f32", "bids_made"):
            assert meta[k][b] == 0, (b, k)


def _error_of(f):
    with pytest.raises(ValueError) as e:
        f()
    return str(e.value)


def test_verdicts_on_the_mixed_batch():
    import torch
    fx = mixed_batch()
    mats, shapes, prices = fx["mats"], fx["shapes"], fx["prices"]
    B = mats.shape[0]
    want = np.array([_default_mode_code(mats, shapes, prices, b)[0] for b in range(B)], dtype=np.int32)
    assert np.array_equal(want, expected_status(mats, shapes, prices)[0])  # (pinned on the CPU as well)
    assert set(want) == set(range(8)) and B >= 96

    # device stack and device shapes: the shapes of code 7 reach the kernels.  The stack lies between +inf guards.
    pad = np.full((B + 2,) + mats.shape[1:], np.inf)
    pad[1:-1] = mats
    d = torch.from_numpy(pad).cuda()[1:-1]
    res = auction_solve_batch(d, shapes=torch.from_numpy(shapes).cuda(), prices=torch.from_numpy(prices).cuda(),
                              errors="status")
    _check_verdicts(_to_host(res), mats, shapes, prices, want)
    first = int(np.flatnonzero(want)[0])
    assert want[first] != 7
    with pytest.raises(ValueError) as e:
        raise_for_status(res)
    assert str(e.value) == f"problem {first}: " + _default_mode_code(mats, shapes, prices, first)[1][len("problem 0: "):]

    # without the shapes of code 7 the default mode takes the whole batch (B >= 64: its guard runs on the device), and
    # raise_for_status raises what it raises -- numpy stack and device stack
    keep = want != 7
    m2, s2, p2 = mats[keep], shapes[keep], prices[keep]
    assert len(m2) >= 96
    text = _error_of(lambda: auction_solve_batch(m2, shapes=s2, prices=p2))
    for r in (auction_solve_batch(m2, shapes=s2, prices=p2, errors="status"),
              auction_solve_batch(torch.from_numpy(m2).cuda(), shapes=s2, prices=p2, errors="status")):
        assert _error_of(lambda: raise_for_status(r)) == text
        _check_verdicts(_to_host(r), m2, s2, p2, want[keep])
    # ... and from the first shape of code 7 on, the text of the default mode's host check
    b7 = int(np.flatnonzero(want == 7)[0])
    text7 = _error_of(lambda: auction_solve_batch(mats[b7:], shapes=shapes[b7:], prices=prices[b7:]))
    r7 = auction_solve_batch(torch.from_numpy(mats[b7:]).cuda(), shapes=torch.from_numpy(shapes[b7:]).cuda(),
                             prices=torch.from_numpy(prices[b7:]).cuda(), errors="status")
    assert _error_of(lambda: raise_for_status(r7)) == text7
    # a result without a defect comes back as it is
    good = auction_solve_batch(mats[want == 0], shapes=shapes[want == 0], errors="status")
    assert raise_for_status(good) is good


def test_verdicts_below_the_default_modes_device_guard():
    """B < 64: the default mode guards on the host, the status mode on the device; the verdicts are the same."""
    fx = mixed_batch()
    keep = np.flatnonzero(fx["kinds"] != 7)[:40]
    mats, shapes, prices = fx["mats"][keep], fx["shapes"][keep], fx["prices"][keep]
    want = np.array([_default_mode_code(mats, shapes, prices, b)[0] for b in range(len(keep))], dtype=np.int32)
    assert set(want) == set(range(7))
    text = _error_of(lambda: auction_solve_batch(mats, shapes=shapes, prices=prices))
    for res in _both(mats, shapes=shapes, prices=prices):
        _check_verdicts(res, mats, shapes, prices, want)
        assert _error_of(lambda: raise_for_status(dict(res, stack=mats.shape[1:], shapes=shapes))) == text


def test_without_the_guard_code_4_never_appears():
    fx = mixed_batch()
    keep = fx["kinds"] != 7
    mats, shapes, prices = fx["mats"][keep], fx["shapes"][keep], fx["prices"][keep]
    want = np.array([_default_mode_code(mats, shapes, prices, b, cardinality_check=False, max_iter=200)[0]
                     for b in range(len(mats))], dtype=np.int32)
    assert not (want == 4).any() and (want == 0).sum() > (fx["kinds"][keep] == 0).sum()
    for res in _both(mats, shapes=shapes, prices=prices, cardinality_check=False, max_iter=200):
        assert np.array_equal(res["status"], want) and (res["matching_size"] == -1).all()
        # (an infeasible problem that is solved anyway stops at max_iter: no error, as in the default mode)
        b = int(np.flatnonzero((fx["kinds"][keep] == 4) & (want == 0))[0])
        assert res["meta"]["its"][b] == 200 and res["meta"]["soln_found"][b] == 0


def test_default_mode_is_unchanged():
    fx = mixed_batch()
    keep = fx["kinds"] != 7
    with pytest.raises(ValueError, match=r"^problem 1: Matrix is infeasible - Fewer than"):
        auction_solve_batch(fx["mats"][keep], shapes=fx["shapes"][keep], prices=fx["prices"][keep])


# ---- the call does not wait

def _busy(x, reps):
    for _ in range(reps):
        x = x @ x
        x = x / x.norm()  # (keeps the values finite)
    return x


def _run_behind_busy_stream(stream):
    import torch
    rng = np.random.default_rng(31)
    host = _values("holes", (96, 48, 48), rng)
    p0 = rng.uniform(0, 5, (96, 48))
    with torch.cuda.stream(stream):
        src, pd = torch.from_numpy(host).cuda(), torch.from_numpy(p0).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        x = torch.full_like(src, -1.0)
        x.copy_(src)
        auction_solve_batch(x, prices=pd, errors="status")  # the warm-up call
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
        x.fill_(-1.0)  # read before the copy below lands, every problem would have status 1
        torch.cuda.synchronize()
        _busy(w, reps)
        x.copy_(src, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_batch(x, prices=pd, errors="status")
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _to_host(res)
    assert (got["status"] == 0).all()
    _check_all(got, host, "min", prices=p0)


def test_the_call_does_not_wait_on_the_null_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.default_stream())


def test_the_call_does_not_wait_on_a_side_stream():
    import torch
    _run_behind_busy_stream(torch.cuda.Stream())
