"""Candidate lists from two point sets on the GPU (misslap_points_batch_candidates): points_candidates against the numpy
definition points_to_ell, and auction_solve_points_batch(candidates=K) against auction_solve_ell_batch on that
definition's lists.  Every comparison is bit for bit.

  builder   M = 1, 63, 64, 65, 129 (lane and step edges) x N = 1, 3, 4, 5 (rows per workgroup) x k = 1, 2, 63, 64;
            2048 x 2048 with k = 64 once (the 32nd column of a lane, the largest output); both coordinate types x
            D = 1, 2, 3, 8 x the four forms of the limit; cropped shapes from the host and the device and a bad device
            shape; three strided views, read where they lie and never written; integer-grid ties that straddle the k-th
            key; rows with 0, k, k + 1 and all candidates in one workgroup, so both paths run side by side; limits of
            -0.0, -1, NaN, +inf and one equal to a cost; NaN and infinite coordinates and a float64 overflow.
  keyword   candidates=K equals the ELL call on the uploaded lists of the definition in sol, prices, outside_prices,
            status, matching_size and every record field: with outside, with prices= and finish="reverse" (reverse
            too), without outside (where the guard says INFEASIBLE); a NaN coordinate condemns its problem only; a bad
            device shape; truncated; numpy input; errors="raise".
  routes    on an integer grid with fast=True, outside and nothing truncated, obj_f64 equals the points call's without
            candidates.
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import (_lib, auction_solve_ell_batch, auction_solve_points_batch, batch_meta_to_host, points_candidates,
                       points_to_ell)
from tests._points_candidates import (DTYPES, FORMS, KEYS, counted_rows, grid, limit_of, non_finite_batch, same_bytes,
                                      tied_rows)

pytestmark = pytest.mark.gpu

RECORD_KEYS = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj_f64", "start_eps_f32", "final_eps_f32",
               "n_rows", "n_cols", "nnz", "bids_made")


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lists(got):
    """A builder result as numpy arrays; device tensors of the stated types."""
    import torch
    want = dict(cols=torch.int32, vals=torch.float64, counts=torch.int32, rows=torch.int32)
    for key in KEYS:
        assert got[key].is_cuda and got[key].dtype == want[key] and got[key].is_contiguous(), key
    return {key: got[key].cpu().numpy() for key in KEYS}


def check(x, y, k, shapes=None, limit=None, xd=None, yd=None, device_shapes=False):
    """points_candidates on device tensors (xd / yd: views of x / y made by the caller) is points_to_ell on x, y."""
    xd, yd = _dev(x) if xd is None else xd, _dev(y) if yd is None else yd
    lim = _dev(limit) if isinstance(limit, np.ndarray) else limit
    shp = _dev(np.asarray(shapes, dtype=np.int32)) if device_shapes else shapes
    got = _lists(points_candidates(xd, yd, k, shapes=shp, limit=lim))
    want = points_to_ell(x, y, k, shapes, limit)
    for key in KEYS:
        assert got[key].tobytes() == want[key].tobytes(), (key, k, np.flatnonzero(got[key].ravel() != want[key].ravel())[:8])
    return got


# ---- the builder

@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_lane_and_step_edges(gpu_lib, M, N):
    rng = np.random.default_rng([1, M, N])
    x, y = grid((3, N, 2), "float32", rng, 5), grid((3, M, 2), "float32", rng, 5)
    per_row = limit_of("per_row", x, y, rng)
    for k in (1, 2, 63, 64):
        for limit in (None, per_row, 4.0):
            check(x, y, k, limit=limit)


def test_2048_by_2048_with_64_candidates(gpu_lib):
    rng = np.random.default_rng(7)
    x, y = rng.random((1, 2048, 3), dtype=np.float32), rng.random((1, 2048, 3), dtype=np.float32)
    limit = (0.15 + 0.1 * rng.random((1, 2048))) ** 2  # around 64 in-gate columns per row: both paths, at the last step
    got = check(x, y, 64, limit=limit)
    assert (got["counts"] > 64).sum() > 100 and (got["counts"] < 64).sum() > 100
    assert got["cols"].max() == 2047 and (got["cols"][0, :, 0] >= 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_both_types_every_d_and_the_four_limit_forms(gpu_lib, dtype, D):
    rng = np.random.default_rng([2, D])
    B, N, M = 4, 6, 70
    shapes = np.array([[6, 70], [5, 64], [1, 1], [6, 65]])
    for draw in ("grid", "uniform"):
        if draw == "grid":
            x, y = grid((B, N, D), dtype, rng, 6), grid((B, M, D), dtype, rng, 6)
        else:
            x, y = rng.random((B, N, D)).astype(dtype), rng.random((B, M, D)).astype(dtype)
        for form in FORMS:
            limit = limit_of(form, x, y, rng)
            for k in (3, 64):
                check(x, y, k, limit=limit)
                check(x, y, k, shapes=shapes, limit=limit)
        bad = np.array([[6, 70], [7, 70], [0, 3], [6, 71]])  # only a device array can carry these
        got = check(x, y, 5, shapes=bad, limit=limit_of("per_row", x, y, rng), device_shapes=True)
        assert got["rows"].tolist() == [6, 0, 0, 0] and (got["cols"][1:] == -1).all() and not got["counts"][1:].any()
        check(x, y, 5, shapes=shapes, device_shapes=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_views_are_read_where_they_lie(gpu_lib, dtype):
    import torch
    rng = np.random.default_rng(3)
    B, N, M = 3, 5, 67
    state = _dev(grid((B, N, 7), dtype, rng, 6))  # a coordinate slice of a track state
    buf = _dev(grid((B, 2, M), dtype, rng, 6))  # a (B, D, M) buffer, transposed
    one = _dev(grid((1, M, 2), dtype, rng, 6))  # one point set for every problem
    keep = [t.clone() for t in (state, buf, one)]
    xs, yt, ye = state[..., :2], buf.transpose(1, 2), one.expand(B, M, 2)
    assert not xs.is_contiguous() and not yt.is_contiguous() and ye.stride(0) == 0
    for xd, yd in ((xs, yt), (xs, ye)):
        x, y = xd.cpu().numpy().copy(), yd.cpu().numpy().copy()
        for k, limit in ((4, None), (64, 5.0), (2, limit_of("per_row", x, y, rng))):
            check(x, y, k, limit=limit, xd=xd, yd=yd)
    torch.cuda.synchronize()
    for t, was in zip((state, buf, one), keep):
        assert torch.equal(t, was)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2, 5, 63, 64])
def test_zero_k_and_k_plus_one_candidates_in_one_workgroup(gpu_lib, dtype, k):
    x, y, lim, counts = counted_rows(dtype, k, k + 3)
    got = check(x, y, k, limit=lim)
    assert got["counts"][0].tolist() == counts.tolist()
    x, y, lim, counts = counted_rows(dtype, k, 130)  # the truncated rows scan three steps
    check(x, y, k, limit=lim)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_that_straddle_the_kth_key(gpu_lib, dtype):
    for M in (11, 64, 65, 131):
        x, y = tied_rows(dtype, M)
        for k in (1, 2, 3, 10, 63, 64):
            got = check(x, y, k)
            if k < M:
                assert got["cols"][0, 0].tolist() == sorted([M - 1] + list(range(k - 1))), (M, k)
    rng = np.random.default_rng(4)
    x, y = grid((3, 4, 3), dtype, rng, 3), grid((3, 129, 3), dtype, rng, 3)  # 27 distinct points: long runs of equal costs
    for k in (1, 7, 33, 64):
        got = check(x, y, k)
        assert (got["counts"] == 129).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_limit_edge_values(gpu_lib, dtype):
    x = np.zeros((1, 6, 2), dtype=dtype)
    y = np.array([[[0, 0], [1, 0], [0, 0], [1, 1]]], dtype=dtype)
    lim = np.array([[-0.0, 1.0, np.nan, np.inf, -1e-300, np.nextafter(1.0, 0.0)]])
    got = check(x, y, 4, limit=lim)
    assert got["counts"][0].tolist() == [2, 3, 0, 4, 0, 2]
    for scalar in (-0.0, float("nan"), float("inf"), -1.0, float("-inf"), 0.0):
        check(x, y, 2, limit=scalar)
    check(x, y, 4, limit=np.array([-np.nan]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_costs_that_are_not_finite(gpu_lib, dtype):
    x, y = non_finite_batch(dtype)
    for limit in (None, -1.0, 2.0, float("nan")):
        for k in (1, 2, 5):
            got = check(x, y, k, limit=limit)
            assert not np.isnan(got["vals"]).any() and np.isposinf(got["vals"][0, 1]).all()
    y2 = y.copy()
    y2[3, :, 1] = np.nan  # a whole problem of NaN costs: every column of every row, stored as +inf
    got = check(x, y2, 3)
    assert (got["counts"][3] == 5).all() and np.isposinf(got["vals"][3]).all()


# ---- the keyword

def _problem(seed, B=5, N=9, M=13, D=2, dtype="float32", hi=6):
    rng = np.random.default_rng(seed)
    x, y = grid((B, N, D), dtype, rng, hi), grid((B, M, D), dtype, rng, hi)
    outside = rng.integers(1, 12, (B, N)).astype(np.float64)
    return rng, x, y, outside


def _same_as_ell(res, ref, reverse=False):
    """A candidates= result holds the bits of the ELL call's result `ref` (both on the device)."""
    assert res["layout"] == ref["layout"] == "ell"
    for key in ("sol", "prices", "status", "matching_size") + (("outside_prices",) if "outside_prices" in ref else ()):
        assert res[key].cpu().numpy().tobytes() == ref[key].cpu().numpy().tobytes(), key
    assert ("outside_prices" in res) == ("outside_prices" in ref)
    for key in RECORD_KEYS:
        assert res["meta"][key].cpu().numpy().tobytes() == ref["meta"][key].cpu().numpy().tobytes(), key
    assert ("reverse" in res) == reverse
    if reverse:
        for key in ("its", "left"):
            assert res["reverse"][key].cpu().numpy().tobytes() == ref["reverse"][key].cpu().numpy().tobytes(), key


def _ell_on_definition(x, y, k, M, shapes=None, outside=None, **kw):
    ell = points_to_ell(x, y, k, shapes, outside)
    ref = auction_solve_ell_batch(_dev(ell["cols"]), _dev(ell["vals"]), rows=_dev(ell["rows"]), n_cols=M, problem="min",
                                  outside=_dev(outside), errors="status", **kw)
    return ell, ref


@pytest.mark.parametrize("k", [3, 13])
def test_the_keyword_is_the_ell_call_on_the_definition(gpu_lib, k):
    rng, x, y, outside = _problem(11)
    shapes = np.array([[9, 13], [4, 13], [9, 5], [1, 1], [9, 12]])
    for shp in (None, shapes):
        res = auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), candidates=k, shapes=shp, errors="status")
        ell, ref = _ell_on_definition(x, y, k, 13, shp, outside)
        _same_as_ell(res, ref)
        assert same_bytes(_lists(res["candidates"]), ell)
        assert res["truncated"].cpu().numpy().tolist() == (ell["counts"] > k).sum(axis=1).tolist()
        assert res["truncated"].dtype == res["status"].dtype and (res["status"].cpu().numpy() == 0).all()
    assert (ell["counts"] > 3).any() and not (ell["counts"] > 13).any()


def test_the_keyword_with_prices_and_the_reverse_finish(gpu_lib):
    rng, x, y, outside = _problem(12)
    prices = rng.integers(0, 9, (5, 13)).astype(np.float64)
    for kw in (dict(prices=_dev(prices), finish="reverse"), dict(prices=_dev(prices), finish="reverse", fast=False, eps_start=0.5),
               dict(finish="reverse"), dict(prices=_dev(prices))):
        res = auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), candidates=6, errors="status", **kw)
        _, ref = _ell_on_definition(x, y, 6, 13, None, outside, **kw)
        _same_as_ell(res, ref, reverse="finish" in kw)
    assert (res["status"].cpu().numpy() == 0).all()


def test_the_keyword_without_outside(gpu_lib):
    rng, x, y, _ = _problem(13)
    shapes = np.array([[9, 13], [9, 5], [4, 4], [13 - 4, 9], [2, 13]])  # problem 1: n > m, which the guard condemns
    for k in (2, 13):
        res = auction_solve_points_batch(_dev(x), _dev(y), candidates=k, shapes=shapes, errors="status")
        _, ref = _ell_on_definition(x, y, k, 13, shapes)
        _same_as_ell(res, ref)
        status = res["status"].cpu().numpy()
        assert status[1] == _lib.BATCH_STATUS_INFEASIBLE and "outside_prices" not in res
    assert status[0] == 0 and status[4] == 0  # (k = 13: every pair is an edge)


def test_a_nan_coordinate_a_bad_shape_and_errors_raise(gpu_lib):
    rng, x, y, outside = _problem(14)
    x[1, 2, 0] = np.nan
    y[3, 0, 1] = np.inf
    shapes = np.array([[9, 13], [9, 13], [10, 13], [9, 13], [9, 13]], dtype=np.int32)
    res = auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), candidates=5, shapes=_dev(shapes), errors="status")
    _, ref = _ell_on_definition(x, y, 5, 13, shapes, outside)
    _same_as_ell(res, ref)
    assert res["status"].cpu().numpy().tolist() == [0, _lib.BATCH_STATUS_INFINITE_VALUE, _lib.BATCH_STATUS_BAD_SHAPE,
                                                   _lib.BATCH_STATUS_INFINITE_VALUE, 0]
    assert res["candidates"]["rows"].cpu().numpy().tolist() == [9, 9, 0, 9, 9]
    with pytest.raises(ValueError, match=r"problem 1: val holds a NaN or an infinity"):
        auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), candidates=5, shapes=_dev(shapes))
    with pytest.raises(ValueError, match=r"problem 0: rows = 0 outside 1 \.\. 9"):
        auction_solve_points_batch(_dev(x[2:]), _dev(y[2:]), outside=2.0, candidates=5, shapes=_dev(shapes[2:]))
    good = auction_solve_points_batch(_dev(x[4:]), _dev(y[4:]), outside=_dev(outside[4:]), candidates=5)  # errors="raise"
    assert good["sol"].cpu().numpy().tobytes() == res["sol"][4:].cpu().numpy().tobytes()


def test_numpy_input_comes_back_as_numpy(gpu_lib):
    rng, x, y, outside = _problem(15)
    prices = rng.integers(0, 9, (5, 13)).astype(np.float64)
    for kw in (dict(), dict(prices=prices, finish="reverse")):
        res = auction_solve_points_batch(x, y, outside=outside, candidates=4, errors="status", **kw)
        ell, ref = _ell_on_definition(x, y, 4, 13, None, outside, **{k: _dev(v) if k == "prices" else v for k, v in kw.items()})
        meta = batch_meta_to_host(ref)
        for key in ("sol", "prices", "outside_prices", "status", "matching_size", "truncated"):
            assert isinstance(res[key], np.ndarray), key
        for key in ("sol", "prices", "outside_prices", "status", "matching_size"):
            assert res[key].tobytes() == ref[key].cpu().numpy().tobytes(), key
        for key in RECORD_KEYS:
            assert np.asarray(res["meta"][key]).tobytes() == np.asarray(meta[key]).tobytes(), key
        assert same_bytes(res["candidates"], ell) and "records" not in res and "stream" not in res
        assert res["truncated"].tolist() == (ell["counts"] > 4).sum(axis=1).tolist()
        if "finish" in kw:
            assert res["reverse"]["its"].tobytes() == ref["reverse"]["its"].cpu().numpy().tobytes()
            assert res["reverse"]["left"].tobytes() == ref["reverse"]["left"].cpu().numpy().tobytes()
    got = points_candidates(x, y, 4, limit=outside)
    assert all(isinstance(got[key], np.ndarray) for key in KEYS) and same_bytes(got, ell)


# ---- where both routes exist

@pytest.mark.parametrize("dtype", DTYPES)
def test_untruncated_lists_give_the_optimum_of_the_points_call(gpu_lib, dtype):
    """Integer-grid coordinates, integer outside values, fast=True: both routes end with exact optima (integers,
    n * eps < 1), and with nothing truncated the optimum of the lists is that of the full problem."""
    rng = np.random.default_rng(16)
    B, N, M = 24, 44, 43
    x, y = grid((B, N, 3), dtype, rng, 8), grid((B, M, 3), dtype, rng, 8)
    outside = rng.integers(0, 30, (B, N)).astype(np.float64)
    shapes = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1)
    full = auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), shapes=shapes, fast=True, errors="status")
    lists = auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), shapes=shapes, fast=True, candidates=43,
                                       errors="status")
    assert (lists["truncated"].cpu().numpy() == 0).all()
    assert (full["status"].cpu().numpy() == 0).all() and (lists["status"].cpu().numpy() == 0).all()
    a, b = full["meta"]["obj_f64"].cpu().numpy(), lists["meta"]["obj_f64"].cpu().numpy()
    assert a.tobytes() == b.tobytes(), (a, b)
    assert (a > 0).sum() > B // 2
    assert (lists["candidates"]["counts"].cpu().numpy() < shapes[:, 1:2]).any()  # the gate removed pairs
