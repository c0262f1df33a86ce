"""auction_solve_points_batch(whiten=W) and points_candidates(whiten=W) on the GPU (misslap_solve_points_batch_whitened,
misslap_points_batch_candidates_whitened): Mahalanobis costs |W_i (x_i - y_j)|^2 from a lower-triangular matrix per row,
the cost stack never stored.  Every comparison is bit for bit.

  parity       every problem is the oracle's result on points_to_dense(whiten=)'s slice: the mixed shapes of
               test_points_batch.py in one 300 x 300 call, D = 1 .. 4, both types, uniform and grid draws, min and max,
               from numpy arrays and from device tensors (for float64 the fused chain differs on the uniform draw).
  cross-check  the dense batch on the stored whitened stack, also with prices=, eps_start=, fast=True and max_iter cuts.
  identity     W = I (NaN above the diagonal) gives the plain call's bits in every output and meta field.
  outside      70 rows, m = 1 .. 130, an outside value equal to a cost, the three forms -- against the dense outside call
               and the oracle on dense_to_augmented.
  sizes        N = 256, 257, 512, 513 at D = 4; one 2048 x 2048 problem, D = 4, float64, outside (the 155 648-byte carve).
  verdicts     a mixed batch, statuses derived on the CPU from the definition alone.
  views        W inside a poisoned buffer, transposed in its last two dimensions, expanded over N and over B.
  builder      points_candidates(whiten=) is points_to_ell(whiten=); the keyword route is the ELL call on those lists.
  no wait      behind >= 200 ms of queued work the device call returns at once.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import (auction_solve_batch, auction_solve_ell_batch, auction_solve_points_batch, points_candidates,
                       points_to_dense, points_to_ell, raise_for_status)
from tests._batch_shapes import bits, dense_compare, dense_expect, threads_for
from tests._points_candidates import KEYS, counted_rows, same_bytes, tied_rows
from tests._points_fixture import DTYPES, draw, outside_rows
from tests._points_whiten import (WHITEN_DIMS, draw_whiten, expected_status, identity_whiten, inf_minus_inf_case,
                                  verdict_batch, whitened_fused_by_loops)
from tests.test_dense_batch_status import _busy
from tests.test_dense_outside import compare as outside_compare, expect as outside_expect
from tests.test_points_batch import (MIXED_M, MIXED_N, MIXED_SHAPES, OUT_M, OUT_N, _condemned, _dev, _host, _raw, _same,
                                     check_plain, mixed_points, outside_points)
from tests.test_points_candidates import _lists, _same_as_ell

pytestmark = pytest.mark.gpu
KINDS = ("uniform", "grid")


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@functools.lru_cache(maxsize=None)
def mixed_whiten(kind, D, dtype):
    """W for mixed_points(kind, D, dtype): NaN above every diagonal and in the rows beyond every shape."""
    rng = np.random.default_rng([23, KINDS.index(kind), D, DTYPES.index(dtype)])
    w = np.full((len(MIXED_SHAPES), MIXED_N, D, D), np.nan, dtype=dtype)
    for b, (n, _) in enumerate(MIXED_SHAPES):
        w[b, :n] = draw_whiten(kind, (n, D, D), dtype, rng)
    w.setflags(write=False)
    return w


# ---- parity with the oracle on the definition

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_parity_with_the_oracle_on_the_definition(D, dtype, kind):
    x, y = mixed_points(kind, D, dtype)
    w = mixed_whiten(kind, D, dtype)
    cost = points_to_dense(x, y, MIXED_SHAPES, whiten=w)
    if kind == "uniform" and dtype == "float64" and D >= 2:  # a contracted chain is another function on this draw
        b = 5
        n, m = MIXED_SHAPES[b]
        fused = whitened_fused_by_loops(x[b:b + 1, :n], y[b:b + 1, :m], np.where(np.isnan(w[b:b + 1, :n]), 0, w[b:b + 1, :n]))
        assert (bits(fused) != bits(cost[b:b + 1, :n, :m])).any()
    dx, dy, dw = _dev(x), _dev(y), _dev(w)
    for problem in ("min", "max"):
        got = auction_solve_points_batch(x, y, problem=problem, shapes=MIXED_SHAPES, errors="status", whiten=w)
        assert got["layout"] == "points" and got["meta"]["gpu"]["threads"] == threads_for(MIXED_N)
        check_plain(got, cost, MIXED_SHAPES, problem)
        dev = auction_solve_points_batch(dx, dy, problem=problem, shapes=_dev(MIXED_SHAPES), errors="status", whiten=dw)
        assert dev["sol"].is_cuda
        _same(_host(dev), got, matching_size=True)


# ---- cross-check with the dense batch on the stored whitened stack

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_dense_batch_on_the_stored_whitened_stack_gives_the_same_bits(dtype):
    x, y = mixed_points("uniform", 3, dtype)
    w = mixed_whiten("uniform", 3, dtype)
    dx, dy, dw, ds = _dev(x), _dev(y), _dev(w), _dev(MIXED_SHAPES)
    dc = _dev(points_to_dense(x, y, MIXED_SHAPES, whiten=w))
    p0 = np.random.default_rng(5).uniform(0, 2, (len(MIXED_SHAPES), MIXED_M))

    def pair(**kw):
        a = _host(auction_solve_points_batch(dx, dy, shapes=ds, errors="status", whiten=dw, **kw))
        b = _host(auction_solve_batch(dc, shapes=ds, errors="status", cardinality_check=False, **kw))
        assert (a["status"] == 0).all()
        _same(a, b)
        return a

    full = pair()
    pair(problem="max")
    pair(prices=_dev(p0))
    pair(eps_start=0.01)
    pair(fast=True)
    pair(fast=True, prices=p0)
    its = full["meta"]["its"]
    for cut in sorted({0, 1, 10, int(its[9]) - 1, int(its[6]) - 1}):
        cut_res = pair(max_iter=cut)
        assert (cut_res["meta"]["its"] <= max(cut, 1)).all()


# ---- the identity

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_the_identity_gives_the_plain_calls_bits(D, dtype):
    x, y = mixed_points("uniform", D, dtype)
    w = identity_whiten(len(MIXED_SHAPES), MIXED_N, D, dtype)
    dx, dy, ds = _dev(x), _dev(y), _dev(MIXED_SHAPES)
    p0 = np.random.default_rng(6).uniform(0, 2, (len(MIXED_SHAPES), MIXED_M))
    for kw in (dict(), dict(problem="max"), dict(prices=p0, outside=0.5), dict(outside=0.25, fast=False)):
        plain = _host(auction_solve_points_batch(dx, dy, shapes=ds, errors="status", **kw))
        white = _host(auction_solve_points_batch(dx, dy, shapes=ds, errors="status", whiten=_dev(w), **kw))
        _same(white, plain, matching_size=True)


# ---- outside

@functools.lru_cache(maxsize=None)
def outside_whitened(dtype):
    """outside_points' point sets with a matrix per row; per-row outside values, one in three equal to a whitened cost."""
    x, y, shapes, _, _ = outside_points(dtype)
    rng = np.random.default_rng([24, DTYPES.index(dtype)])
    B = len(shapes)
    w = draw_whiten("uniform", (B, OUT_N, 3, 3), dtype, rng)
    cost = points_to_dense(x, y, shapes, whiten=w)
    outside = rng.uniform(0.0, 1.5, (B, OUT_N))
    for b, (n, m) in enumerate(shapes):
        i = np.arange(0, n, 3)
        outside[b, i] = cost[b, i, rng.integers(0, m, i.size)]
        outside[b, n:] = np.nan
        w[b, n:] = np.nan
    for a in (w, cost, outside):
        a.setflags(write=False)
    return x, y, w, shapes, cost, outside


@pytest.mark.parametrize("dtype", DTYPES)
def test_outside_at_every_lane_of_the_virtual_entry(dtype):
    x, y, w, shapes, cost, outside = outside_whitened(dtype)
    got = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, errors="status", whiten=w)
    assert (got["status"] == 0).all() and (got["matching_size"] == -1).all()
    for b, (want, m, n) in enumerate(outside_expect(cost, shapes, outside, "min", fast=True)):
        outside_compare(got, b, want, m, n)
    assert (got["sol"] == -1).any() and (got["sol"] >= 0).any() and (shapes[:, 0] > shapes[:, 1]).any()
    dx, dy, dw, ds, do = _dev(x), _dev(y), _dev(w), _dev(shapes), _dev(outside)
    _same(_host(auction_solve_points_batch(dx, dy, shapes=ds, outside=do, errors="status", whiten=dw)), got, matching_size=True)
    _same(_host(auction_solve_batch(_dev(cost), shapes=ds, outside=do, errors="status")), got, matching_size=True)


@pytest.mark.parametrize("form", ["scalar", "per_problem"])
def test_outside_forms_against_the_dense_outside_call(form):
    x, y, w, shapes, cost, _ = outside_whitened("float64")
    rng = np.random.default_rng(9)
    B = len(shapes)
    outside = 0.75 if form == "scalar" else rng.uniform(0.0, 2.0, B)
    p0 = rng.uniform(0, 1, (B, OUT_M))
    dx, dy, dw, dc, ds = _dev(x), _dev(y), _dev(w), _dev(cost), _dev(shapes)
    for kw in (dict(), dict(eps_start=0.05), dict(prices=p0), dict(problem="max", max_iter=5)):
        o = _dev(outside) if form != "scalar" else outside
        got = _host(auction_solve_points_batch(dx, dy, shapes=ds, outside=o, errors="status", whiten=dw, **kw))
        dense = _host(auction_solve_batch(dc, shapes=ds, outside=o, errors="status", **kw))
        assert (got["status"] == 0).all()
        _same(got, dense, matching_size=True)
    host = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, errors="status", whiten=w)
    _same(host, _host(auction_solve_batch(dc, shapes=ds, outside=outside, errors="status")), matching_size=True)


# ---- the workgroup sizes and the caps

@pytest.mark.parametrize("N", [256, 257, 512, 513])
def test_each_workgroup_size_at_four_coordinates(N):
    rng = np.random.default_rng([42, N])
    M = N + 3
    x, y = draw("uniform", (2, N, 4), "float32", rng), draw("uniform", (2, M, 4), "float32", rng)
    x[1], y[1] = draw("grid", (N, 4), "float32", rng), draw("grid", (M, 4), "float32", rng)
    w = draw_whiten("uniform", (2, N, 4, 4), "float32", rng)
    w[1] = draw_whiten("grid", (N, 4, 4), "float32", rng)
    shapes = np.array([[N, M], [N - 1, N - 1]], dtype=np.int32)
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), shapes=shapes, errors="status", whiten=_dev(w)))
    assert got["meta"]["gpu"]["threads"] == threads_for(N)
    check_plain(got, points_to_dense(x, y, shapes, whiten=w), shapes, "min")


def test_the_caps_2048_x_2048_with_outside_at_four_coordinates():
    rng = np.random.default_rng(35)
    x, y = draw("uniform", (1, 2048, 4), "float64", rng), draw("uniform", (1, 2048, 4), "float64", rng)
    w = draw_whiten("uniform", (1, 2048, 4, 4), "float64", rng)
    outside = rng.uniform(0.0, 0.3, (1, 2048))
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), fast=True, errors="status",
                                           whiten=_dev(w)))
    assert got["meta"]["gpu"]["lds_bytes"] == 155648 and got["meta"]["gpu"]["threads"] == 1024 and got["status"][0] == 0
    ((want, m, n),) = outside_expect(points_to_dense(x, y, whiten=w), None, outside, "min", fast=True)
    outside_compare(got, 0, want, m, n)
    assert (got["sol"][0] == -1).any() and (got["sol"][0] >= 0).any()


# ---- verdicts

@pytest.mark.parametrize("with_outside", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_verdicts_of_a_mixed_whitened_batch(dtype, with_outside):
    v = verdict_batch(dtype)
    x, y, w, shapes, kinds = v["x"], v["y"], v["w"], v["shapes"], v["kinds"]
    outside = v["outside"] if with_outside else None
    B, N = x.shape[:2]
    status, size = expected_status(x, y, w, shapes, outside=outside)
    for b, kind in enumerate(kinds):  # the table, from the definition alone
        want = {"ok": 0, "nan_upper_only": 0, "nan_rows_beyond": 0, "shape_0_5": 7,
                "bad_outside": 15 if with_outside else 3}.get(kind, 3)
        assert status[b] == want, (b, kind, status[b])
    cost = points_to_dense(x, y, shapes, whiten=w)
    dx, dy, dw, ds = _dev(x), _dev(y), _dev(w), _dev(shapes)
    do = None if outside is None else _dev(outside)
    res = auction_solve_points_batch(dx, dy, shapes=ds, outside=do, errors="status", whiten=dw)
    got = _host(res)
    assert np.array_equal(got["status"], status), (got["status"], status)
    assert np.array_equal(got["matching_size"], size)
    o = None if outside is None else outside_rows(outside, B, N)
    for b in range(B):
        n, m = (int(s) for s in shapes[b])
        if status[b] == 0 and outside is None:
            dense_compare(got, b, dense_expect(cost[b, :n, :m], "min", cardinality_check=False), n, m)
        elif status[b] == 0:
            ((want, m_, n_),) = outside_expect(cost[b:b + 1], shapes[b:b + 1], o[b:b + 1], "min", fast=True)
            one = {k: (a[b:b + 1] if isinstance(a, np.ndarray) else a) for k, a in got.items() if k != "meta"}
            one["meta"] = {k: a[b:b + 1] for k, a in got["meta"].items() if isinstance(a, np.ndarray)}
            outside_compare(one, 0, want, m_, n_)
        elif status[b] == 7:
            _condemned(got, b, 0, 0, 0)
        else:
            _condemned(got, b, n, m + n if with_outside else m, n * m + (n if with_outside else 0))
    first = int(np.flatnonzero(status)[0])
    with pytest.raises(ValueError, match=f"problem {first}: .*whitening matrix"):
        raise_for_status(res)
    with pytest.raises(ValueError, match=f"problem {first}: "):
        auction_solve_points_batch(dx, dy, shapes=ds, outside=do, whiten=dw)
    keep = np.flatnonzero(status != 7)  # (host shapes are checked before the library)
    host = auction_solve_points_batch(np.ascontiguousarray(x[keep]), np.ascontiguousarray(y[keep]), shapes=shapes[keep],
                                      outside=None if outside is None else outside[keep], errors="status",
                                      whiten=np.ascontiguousarray(w[keep]))
    assert np.array_equal(host["status"], status[keep]) and np.array_equal(host["sol"], got["sol"][keep])
    assert np.array_equal(bits(host["prices"]), bits(got["prices"][keep]))


# ---- views

@pytest.mark.parametrize("dtype", DTYPES)
def test_views_of_the_matrices_are_read_where_they_lie(dtype):
    import torch
    rng = np.random.default_rng([52, DTYPES.index(dtype)])
    B, N, M, D = 5, 70, 130, 3
    x, y = draw("uniform", (B, N, D), dtype, rng), draw("uniform", (B, M, D), dtype, rng)
    w = draw_whiten("uniform", (B, N, D, D), dtype, rng)
    shapes = np.array([[70, 130], [64, 65], [1, 1], [33, 129], [70, 70]], dtype=np.int32)
    outside = rng.uniform(0.0, 1.0, (B, N))
    dx, dy, ds, do = _dev(x), _dev(y), _dev(shapes), _dev(outside)
    want = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, errors="status", whiten=w)
    assert (want["status"] == 0).all()
    tdt = getattr(torch, dtype)
    # W: a corner of a poisoned (B + 2, N + 2, 7, 7) covariance buffer
    cov = torch.full((B + 2, N + 2, 7, 7), float("nan"), dtype=tdt)
    cov[1:B + 1, 1:N + 1, :D, :D] = torch.from_numpy(w.copy())
    cov = cov.cuda()
    wv = cov[1:B + 1, 1:N + 1, :D, :D]
    # W: stored transposed in its last two dimensions
    wt_store = torch.from_numpy(np.ascontiguousarray(w.transpose(0, 1, 3, 2))).cuda()
    wt = wt_store.transpose(2, 3)
    assert not wv.is_contiguous() and wt.stride(3) != 1 and tuple(wt.shape) == (B, N, D, D)
    before = (_raw(cov), _raw(wt_store))
    for view in (wv, wt):
        got = _host(auction_solve_points_batch(dx, dy, shapes=ds, outside=do, errors="status", whiten=view))
        _same(got, want, matching_size=True)
        lists = _lists(points_candidates(dx, dy, 8, shapes=ds, limit=do, whiten=view))
        assert same_bytes(lists, points_to_ell(x, y, 8, shapes, outside, whiten=w))
    assert (_raw(cov), _raw(wt_store)) == before
    # one matrix per problem, and one for the whole call: expanded, strides of 0
    for src in (w[:, :1], w[:1, :1]):
        ev = _dev(src).expand(B, N, D, D)
        assert ev.stride(1) == 0 and (src.shape[0] == B or ev.stride(0) == 0)
        full = np.ascontiguousarray(np.broadcast_to(src, (B, N, D, D)))
        want_e = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, errors="status", whiten=full)
        _same(_host(auction_solve_points_batch(dx, dy, shapes=ds, outside=do, errors="status", whiten=ev)), want_e,
              matching_size=True)
        lists = _lists(points_candidates(dx, dy, 8, shapes=ds, limit=do, whiten=ev))
        assert same_bytes(lists, points_to_ell(x, y, 8, shapes, outside, whiten=full))


# ---- the builder

def check_builder(x, y, w, k, shapes=None, limit=None):
    """points_candidates(whiten=) on device tensors is points_to_ell(whiten=)."""
    lim = _dev(limit) if isinstance(limit, np.ndarray) else limit
    got = _lists(points_candidates(_dev(x), _dev(y), k, shapes=shapes, limit=lim, whiten=_dev(w)))
    want = points_to_ell(x, y, k, shapes, limit, whiten=w)
    for key in KEYS:
        assert got[key].tobytes() == want[key].tobytes(), (key, k, np.flatnonzero(got[key].ravel() != want[key].ravel())[:8])
    return got


def _grid_problem(rng, B, N, M, D, dtype):
    return (rng.integers(0, 5, (B, N, D)).astype(dtype), rng.integers(0, 5, (B, M, D)).astype(dtype),
            draw_whiten("grid", (B, N, D, D), dtype, rng))


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_builder_lane_and_step_edges(gpu_lib, M, N):
    rng = np.random.default_rng([2, M, N])
    x, y, w = _grid_problem(rng, 3, N, M, 2, "float32")
    cost = points_to_dense(x, y, whiten=w)
    per_row = np.sort(cost, axis=2)[:, :, min(M - 1, 2)] + np.array([0.0, 0.25, -1.0, np.nan, np.inf])[np.arange(N) % 5]
    for k in (1, 8, 64):
        for limit in (None, per_row, 9.0, np.array([4.0, -0.0, 100.0])):
            check_builder(x, y, w, k, limit=limit)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", WHITEN_DIMS)
def test_builder_every_d_both_types_and_shapes(gpu_lib, dtype, D):
    rng = np.random.default_rng([3, D])
    x, y = draw("uniform", (4, 9, D), dtype, rng), draw("uniform", (4, 70, D), dtype, rng)
    w = draw_whiten("uniform", (4, 9, D, D), dtype, rng)
    shapes = np.array([[9, 70], [3, 64], [0, 5], [9, 1]], dtype=np.int32)
    w[1, 3:] = np.nan
    for k in (1, 8, 64):
        check_builder(x, y, w, k, shapes=_dev(shapes), limit=0.8)
        check_builder(x, y, w, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 8, 64])
def test_builder_zero_k_and_k_plus_one_candidates_and_ties(gpu_lib, dtype, k):
    for M in (k + 3, 130):
        x, y, lim, counts = counted_rows(dtype, k, M)  # D = 1: the cost is (w00 * j)^2
        w = np.full((1, 4, 1, 1), 2.0, dtype=dtype)
        got = check_builder(x, y, w, k, limit=lim * 4.0)
        assert got["counts"][0].tolist() == counts.tolist()
    for M in (11, 65, 131):  # ties straddle the k-th key: a rotation keeps every ring point at distance 1
        x, y = tied_rows(dtype, M)
        w = np.zeros((1, 2, 2, 2), dtype=dtype)
        w[0, :, 0, 0] = w[0, :, 1, 1] = 1.0
        w[0, :, 0, 1] = np.nan
        got = check_builder(x, y, w, k)
        if k < M:
            assert got["cols"][0, 0].tolist() == sorted([M - 1] + list(range(k - 1))), (M, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_builder_costs_that_are_not_finite(gpu_lib, dtype):
    v = verdict_batch(dtype, D=2)
    for limit in (None, -1.0, 0.7, float("nan")):
        for k in (1, 3, 11):
            got = check_builder(v["x"], v["y"], v["w"], k, shapes=_dev(v["shapes"]), limit=limit)
            assert not np.isnan(got["vals"]).any()
    bad = [b for b, kind in enumerate(v["kinds"]) if kind in ("nan_triangle", "inf_w000", "overflow", "inf_minus_inf")]
    for b in bad:
        assert np.isposinf(got["vals"][b]).any(), v["kinds"][b]
    if dtype == "float64":
        x, y, w = inf_minus_inf_case()
        got = check_builder(x, y, w, 1, limit=-1.0)
        assert got["counts"][0, 0] == 1 and np.isposinf(got["vals"][0, 0, 0])


def test_builder_2048_by_2048_with_64_candidates(gpu_lib):
    rng = np.random.default_rng(8)
    x, y = rng.random((1, 2048, 4), dtype=np.float32), rng.random((1, 2048, 4), dtype=np.float32)
    w = draw_whiten("uniform", (1, 2048, 4, 4), "float32", rng)
    cost = points_to_dense(x, y, whiten=w)
    # the limit of a row is its r-th smallest cost, r = 40 .. 89: r + 1 in-gate columns, both paths at the last step
    limit = np.take_along_axis(np.sort(cost[0], axis=1), rng.integers(40, 90, (2048, 1)), axis=1)[:, 0][None]
    got = check_builder(x, y, w, 64, limit=np.ascontiguousarray(limit))
    assert (got["counts"] > 64).sum() > 100 and (got["counts"] < 64).sum() > 100


# ---- end to end: the keyword route

def test_the_keyword_route_is_the_ell_call_on_the_whitened_lists(gpu_lib):
    rng = np.random.default_rng(14)
    B, N, M, D = 5, 9, 13, 3
    x, y, w = _grid_problem(rng, B, N, M, D, "float32")
    outside = rng.integers(1, 40, (B, N)).astype(np.float64)
    prices = rng.integers(0, 9, (B, M)).astype(np.float64)
    shapes = np.array([[9, 13], [4, 13], [9, 5], [1, 1], [9, 12]])
    dx, dy, dw, do = _dev(x), _dev(y), _dev(w), _dev(outside)
    for k in (3, 13):
        for kw in (dict(), dict(shapes=shapes), dict(prices=_dev(prices), finish="reverse"), dict(finish="reverse")):
            res = auction_solve_points_batch(dx, dy, outside=do, candidates=k, errors="status", whiten=dw, **kw)
            ell = points_to_ell(x, y, k, kw.get("shapes"), outside, whiten=w)
            ekw = {key: v for key, v in kw.items() if key != "shapes"}
            ref = auction_solve_ell_batch(_dev(ell["cols"]), _dev(ell["vals"]), rows=_dev(ell["rows"]), n_cols=M,
                                          problem="min", outside=do, errors="status", **ekw)
            _same_as_ell(res, ref, reverse="finish" in kw)
            assert same_bytes(_lists(res["candidates"]), ell)
            assert res["truncated"].cpu().numpy().tolist() == (ell["counts"] > k).sum(axis=1).tolist()
    # where nothing was truncated the objective is the full whitened call's
    res = auction_solve_points_batch(dx, dy, outside=do, candidates=13, errors="status", whiten=dw)
    full = _host(auction_solve_points_batch(dx, dy, outside=do, errors="status", whiten=dw))
    assert (res["truncated"].cpu().numpy() == 0).all() and (full["status"] == 0).all()
    assert np.array_equal(res["meta"]["obj_f64"].cpu().numpy(), full["meta"]["obj_f64"])
    host = auction_solve_points_batch(x, y, outside=outside, candidates=13, errors="status", whiten=w)
    assert isinstance(host["sol"], np.ndarray) and np.array_equal(host["sol"], res["sol"].cpu().numpy())


# ---- no wait

def test_the_whitened_device_call_does_not_wait():
    import torch
    rng = np.random.default_rng(62)
    B, N, M, D = 96, 48, 64, 3
    x, y = draw("uniform", (B, N, D), "float32", rng), draw("uniform", (B, M, D), "float32", rng)
    w = draw_whiten("uniform", (B, N, D, D), "float32", rng)
    outside = rng.uniform(0.0, 1.0, (B, N))
    want = auction_solve_points_batch(x, y, outside=outside, errors="status", whiten=w)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sw, dx, dy, do = _dev(w), _dev(x), _dev(y), _dev(outside)
        dw = torch.full_like(sw, float("nan"))
        dw.copy_(sw)
        busy = torch.randn(4096, 4096, device="cuda")
        first = auction_solve_points_batch(dx, dy, outside=do, errors="status", whiten=dw)  # the warm-up call
        _busy(busy, 2)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        _busy(busy, 8)
        e[1].record()
        torch.cuda.synchronize()
        reps = int(np.ceil(8 * 400.0 / e[0].elapsed_time(e[1])))
        e[2].record()
        _busy(busy, reps)
        e[3].record()
        torch.cuda.synchronize()
        queued = e[2].elapsed_time(e[3])
        assert queued >= 200.0, queued
        dw.fill_(float("nan"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(busy, reps)
        dw.copy_(sw, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_points_batch(dx, dy, outside=do, errors="status", whiten=dw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {queued:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < queued / 4, (t_call, queued)
    assert pending
    got = _host(res)
    assert (got["status"] == 0).all()
    _same(got, want, matching_size=True)
    _same(_host(first), want, matching_size=True)
