"""auction_solve_points_batch on the GPU (misslap_solve_points_batch): costs |x_i - y_j|^2 formed from the coordinates,
the distance stack never stored.  Every comparison is bit for bit.

  parity       every problem is the oracle's result on points_to_dense's slice (from_matrix(c_b).solve()): mixed shapes in
               one (B, 300, 300)-sized call, D = 1, 2, 3, 8, both coordinate types, min and max, uniform coordinates (for
               float64 the fused chain differs on the draw: a contracted kernel would fail), an integer grid (exact ties)
               and repeated points -- from numpy arrays and from device tensors.
  cross-check  the dense batch on the stored float64 stack: every output and every meta field, also with prices=,
               eps_start=, fast=True and max_iter cut at 0, 1, 10 and its - 1.
  outside      m = 1 .. 130 under 70 rows, n_b > m_b, an outside value equal to a cost, the three forms of outside on the
               host and on the device -- against the dense call with outside= and the oracle on dense_to_augmented.
  beyond the dense cap   1025 x 1100, 2048 x 2048 and 2048 x 2048 with outside (the 155 648-byte carve).
  workgroup sizes        N = 256, 257, 512, 513 in calls of their own.
  verdicts     a mixed batch: the statuses derived on the CPU, healthy problems equal the oracle, condemned ones have
               exactly the defined outputs; errors="raise" raises the first one's message.
  views        slices, transposes and expanded tensors are read where they lie and never written.
  no wait      behind >= 200 ms of queued work the device call returns at once; the same call twice gives the same bits.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import (auction_solve_batch, auction_solve_points_batch, batch_meta_to_host, points_to_dense,
                       raise_for_status)
from tests._batch_shapes import META_KEYS, bits, dense_compare, dense_expect, threads_for
from tests._points_fixture import DTYPES, KINDS, draw, expected_status, fused_by_loops, outside_rows, verdict_batch
from tests.test_dense_batch_status import _busy
from tests.test_dense_outside import compare as outside_compare, expect as outside_expect
from tests.test_ell_batch import ZERO_META

pytestmark = pytest.mark.gpu

RECORD_KEYS = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj_f64", "start_eps_f32", "final_eps_f32",
               "n_rows", "n_cols", "nnz", "bids_made")
MIXED_SHAPES = np.array([(1, 1), (1, 2), (2, 2), (3, 64), (5, 65), (63, 63), (64, 65), (65, 129), (70, 130), (257, 257)],
                        dtype=np.int32)
MIXED_N = MIXED_M = 300


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def _host(res):
    """A result with numpy arrays and the host meta dict, whichever way it was computed."""
    if isinstance(res["sol"], np.ndarray):
        return res
    meta = batch_meta_to_host(res)
    for k, v in res["meta"].items():  # the device views hold the same records
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), meta[k]), k
    out = dict(res, meta=meta)
    for k in ("sol", "prices", "outside_prices", "status", "matching_size"):
        if k in res:
            assert res[k].is_cuda and res[k].device == res["sol"].device, k
            out[k] = res[k].cpu().numpy()
    return out


def _same(a, b, matching_size=False):
    """Two host results hold the same bits in every output and every field of the records."""
    keys = ["sol", "status"] + (["matching_size"] if matching_size else [])
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    for k in ("prices", "outside_prices"):
        assert (k in a) == (k in b), k
        if k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in RECORD_KEYS + META_KEYS:
        assert np.array_equal(np.asarray(a["meta"][k]).view(np.uint8), np.asarray(b["meta"][k]).view(np.uint8)), k


@functools.lru_cache(maxsize=None)
def mixed_points(kind, D, dtype):
    """(x, y): MIXED_SHAPES' problems in one call; beyond a shape the coordinates are NaN, which a kernel that read them
    would turn into a verdict."""
    rng = np.random.default_rng([21, KINDS.index(kind), D, DTYPES.index(dtype)])
    B = len(MIXED_SHAPES)
    x, y = np.full((B, MIXED_N, D), np.nan, dtype=dtype), np.full((B, MIXED_M, D), np.nan, dtype=dtype)
    for b, (n, m) in enumerate(MIXED_SHAPES):
        x[b, :n], y[b, :m] = draw(kind, (n, D), dtype, rng), draw(kind, (m, D), dtype, rng)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def check_plain(res, cost, shapes, problem, p0=None, size=True, **opts):
    """Every problem of a host result without outside against the oracle on its slice of the cost stack."""
    B, N, M = cost.shape
    assert (res["status"] == 0).all(), res["status"]
    assert res["sol"].shape == (B, N) and res["prices"].shape == (B, M) and "outside_prices" not in res
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        want = dense_expect(cost[b, :n, :m], problem, p0=None if p0 is None else p0[b], cardinality_check=False, **opts)
        dense_compare(res, b, want, n, m, p0=None if p0 is None else p0[b])
        assert res["meta"]["nnz"][b] == n * m and res["meta"]["bids_made"][b] == want["extra"]["bids_made"], b
        if size:
            assert res["matching_size"][b] == min(n, m), b


# ---- parity with the oracle on points_to_dense

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_parity_with_the_oracle_on_the_definition(D, dtype, kind):
    x, y = mixed_points(kind, D, dtype)
    cost = points_to_dense(x, y, MIXED_SHAPES)
    if kind == "uniform" and dtype == "float64" and D >= 2:  # a contracted chain is another function on this draw
        b = 5
        n, m = MIXED_SHAPES[b]
        fused = fused_by_loops(x[b:b + 1, :n], y[b:b + 1, :m])
        assert (bits(fused) != bits(cost[b:b + 1, :n, :m])).any()
    dx, dy = _dev(x), _dev(y)
    for problem in ("min", "max"):
        got = auction_solve_points_batch(x, y, problem=problem, shapes=MIXED_SHAPES, errors="status")
        assert got["layout"] == "points" and got["meta"]["gpu"]["threads"] == threads_for(MIXED_N)
        check_plain(got, cost, MIXED_SHAPES, problem)
        dev = auction_solve_points_batch(dx, dy, problem=problem, shapes=_dev(MIXED_SHAPES), errors="status")
        assert dev["sol"].is_cuda and dev["layout"] == "points"
        _same(_host(dev), got, matching_size=True)
        raised = auction_solve_points_batch(dx, dy, problem=problem, shapes=MIXED_SHAPES)  # errors="raise": the same dict
        _same(_host(raised), got, matching_size=True)


# ---- cross-check with the dense batch on the stored stack

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_dense_batch_on_the_stored_stack_gives_the_same_bits(dtype):
    x, y = mixed_points("uniform", 3, dtype)
    dx, dy, dc, ds = _dev(x), _dev(y), _dev(points_to_dense(x, y, MIXED_SHAPES)), _dev(MIXED_SHAPES)
    rng = np.random.default_rng(5)
    p0 = rng.uniform(0, 2, (len(MIXED_SHAPES), MIXED_M))

    def pair(**kw):
        a = _host(auction_solve_points_batch(dx, dy, shapes=ds, errors="status", **kw))
        b = _host(auction_solve_batch(dc, shapes=ds, errors="status", cardinality_check=False, **kw))
        assert (a["status"] == 0).all()
        _same(a, b)
        return a

    full = pair()
    pair(problem="max")
    pair(prices=_dev(p0))
    pair(prices=p0, problem="max")
    pair(eps_start=0.01)
    pair(fast=True)
    pair(fast=True, prices=p0)
    its = full["meta"]["its"]
    for cut in sorted({0, 1, 10, int(its[9]) - 1, int(its[6]) - 1}):
        cut_res = pair(max_iter=cut)
        assert (cut_res["meta"]["its"] <= max(cut, 1)).all()
    assert full["meta"]["n_assigned"][9] == 257 and pair(max_iter=int(its[9]) - 1)["meta"]["n_assigned"][9] < 257


# ---- outside

OUT_N, OUT_M = 70, 130


@functools.lru_cache(maxsize=None)
def outside_points(dtype):
    """130 problems of 70 rows with m_b = 1 .. 130 columns (n_b > m_b below 70; the virtual entry's lane (m + i) & 63
    walks every lane), every third problem with fewer rows; per-row outside values, one per row equal to a cost."""
    rng = np.random.default_rng([22, DTYPES.index(dtype)])
    B = OUT_M
    x, y = draw("uniform", (B, OUT_N, 3), dtype, rng), draw("uniform", (B, OUT_M, 3), dtype, rng)
    shapes = np.array([(OUT_N if b % 3 else 1 + (7 * b) % OUT_N, b + 1) for b in range(B)], dtype=np.int32)
    cost = points_to_dense(x, y, shapes)
    outside = rng.uniform(0.0, 1.5, (B, OUT_N))
    for b, (n, m) in enumerate(shapes):
        i = np.arange(0, n, 3)
        outside[b, i] = cost[b, i, rng.integers(0, m, i.size)]  # a tie between an entry and the outside entry
        outside[b, n:] = np.nan
    for a in (x, y, shapes, cost, outside):
        a.setflags(write=False)
    return x, y, shapes, cost, outside


@pytest.mark.parametrize("dtype", DTYPES)
def test_outside_at_every_lane_of_the_virtual_entry(dtype):
    x, y, shapes, cost, outside = outside_points(dtype)
    B = len(shapes)
    got = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, errors="status")
    assert (got["status"] == 0).all() and (got["matching_size"] == -1).all() and got["layout"] == "points"
    assert got["outside_prices"].shape == (B, OUT_N)
    for b, (want, m, n) in enumerate(outside_expect(cost, shapes, outside, "min", fast=True)):
        outside_compare(got, b, want, m, n)
    assert (got["sol"] == -1).any() and (got["sol"] >= 0).any()
    dx, dy, ds, do = _dev(x), _dev(y), _dev(shapes), _dev(outside)
    dev = _host(auction_solve_points_batch(dx, dy, shapes=ds, outside=do, errors="status"))
    _same(dev, got, matching_size=True)
    _same(_host(auction_solve_batch(_dev(cost), shapes=ds, outside=do, errors="status")), got, matching_size=True)


@pytest.mark.parametrize("form", ["scalar", "per_problem"])
@pytest.mark.parametrize("problem", ["min", "max"])
def test_outside_forms_and_options(form, problem):
    x, y, shapes, cost, _ = outside_points("float64")
    rng = np.random.default_rng(9)
    B = len(shapes)
    outside = 0.75 if form == "scalar" else rng.uniform(0.0, 2.0, B)
    p0 = rng.uniform(0, 1, (B, OUT_M))
    dx, dy, dc, ds = _dev(x), _dev(y), _dev(cost), _dev(shapes)
    for kw in (dict(), dict(eps_start=0.05), dict(fast=False), dict(prices=p0), dict(max_iter=5)):
        for on_device in (False, True):
            o = _dev(outside) if on_device and form != "scalar" else outside
            if on_device:
                got = _host(auction_solve_points_batch(dx, dy, shapes=ds, outside=o, problem=problem, errors="status", **kw))
            else:
                got = auction_solve_points_batch(x, y, shapes=shapes, outside=o, problem=problem, errors="status", **kw)
            dense = _host(auction_solve_batch(dc, shapes=ds, outside=o, problem=problem, errors="status", **kw))
            assert (got["status"] == 0).all()
            _same(got, dense, matching_size=True)
    # ... and the oracle on dense_to_augmented, for the call as the front end resolves it (fast=True)
    got = auction_solve_points_batch(x, y, shapes=shapes, outside=outside, problem=problem, errors="status")
    pick = [0, 1, 63, 64, 69, 70, 129]
    sub = np.ascontiguousarray(cost[pick])
    o = outside if form == "scalar" else outside[pick]
    for k, (want, m, n) in enumerate(outside_expect(sub, shapes[pick], o, problem, fast=True)):
        one = {key: (v[pick] if isinstance(v, np.ndarray) else v) for key, v in got.items() if key != "meta"}
        one["meta"] = {key: v[pick] for key, v in got["meta"].items() if isinstance(v, np.ndarray)}
        outside_compare(one, k, want, m, n)


# ---- beyond the dense batch's cap

def _one(n, m, D, dtype, seed):
    rng = np.random.default_rng(seed)
    return draw("uniform", (1, n, D), dtype, rng), draw("uniform", (1, m, D), dtype, rng)


def test_beyond_the_dense_cap_1025_x_1100():
    x, y = _one(1025, 1100, 2, "float64", 31)
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), errors="status"))
    assert got["meta"]["gpu"]["threads"] == 1024
    check_plain(got, points_to_dense(x, y), None, "min")


def test_beyond_the_dense_cap_2048_x_2048_float32():
    x, y = _one(2048, 2048, 3, "float32", 32)
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), errors="status"))
    assert got["meta"]["gpu"]["lds_bytes"] == 24 * 2048 + 28 * 2048
    check_plain(got, points_to_dense(x, y), None, "min")


def test_beyond_the_dense_cap_2048_x_2048_with_outside():
    x, y = _one(2048, 2048, 3, "float64", 33)
    outside = np.random.default_rng(34).uniform(0.0, 0.05, (1, 2048))
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), outside=_dev(outside), fast=True, errors="status"))
    assert got["meta"]["gpu"]["lds_bytes"] == 155648 and got["status"][0] == 0
    ((want, m, n),) = outside_expect(points_to_dense(x, y), None, outside, "min", fast=True)
    outside_compare(got, 0, want, m, n)
    assert (got["sol"][0] == -1).any() and (got["sol"][0] >= 0).any()


# ---- the workgroup sizes

@pytest.mark.parametrize("N", [256, 257, 512, 513])
def test_each_workgroup_size(N):
    rng = np.random.default_rng([41, N])
    M = N + 3
    x, y = draw("uniform", (2, N, 2), "float32", rng), draw("uniform", (2, M, 2), "float32", rng)
    y[1] = draw("grid", (M, 2), "float32", rng)
    x[1] = draw("grid", (N, 2), "float32", rng)
    shapes = np.array([[N, M], [N - 1, N - 1]], dtype=np.int32)
    got = _host(auction_solve_points_batch(_dev(x), _dev(y), shapes=shapes, errors="status"))
    assert got["meta"]["gpu"]["threads"] == threads_for(N)
    check_plain(got, points_to_dense(x, y, shapes), shapes, "min")


# ---- verdicts

def _condemned(res, b, n_rows, n_cols, nnz):
    assert (res["sol"][b] == -1).all(), b
    assert (bits(res["prices"][b]) == 0).all(), b
    if "outside_prices" in res:
        assert (bits(res["outside_prices"][b]) == 0).all(), b
    meta = res["meta"]
    assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (n_rows, n_cols, nnz), b
    for k in ZERO_META:
        assert meta[k][b] == 0, (b, k)


@pytest.mark.parametrize("with_outside", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_verdicts_of_a_mixed_batch(dtype, with_outside):
    v = verdict_batch(dtype)
    x, y, shapes, prices = v["x"], v["y"], v["shapes"], v["prices"]
    outside = v["outside"] if with_outside else None
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    status, size = expected_status(x, y, shapes, prices, outside)
    assert len(set(status.tolist())) >= 5
    cost = points_to_dense(x, y)
    dx, dy, ds, dp = _dev(x), _dev(y), _dev(shapes), _dev(prices)
    do = None if outside is None else _dev(outside)
    res = auction_solve_points_batch(dx, dy, shapes=ds, prices=dp, outside=do, errors="status")
    got = _host(res)
    assert np.array_equal(got["status"], status), (got["status"], status)
    assert np.array_equal(got["matching_size"], size), (got["matching_size"], size)
    o = None if outside is None else outside_rows(outside, B, N)
    for b in range(B):
        n, m = (int(s) for s in shapes[b])
        if status[b] == 0 and outside is None:
            want = dense_expect(cost[b, :n, :m], "min", p0=prices[b], cardinality_check=False)
            dense_compare(got, b, want, n, m, p0=prices[b])
        elif status[b] == 0:
            ((want, m_, n_),) = outside_expect(cost[b:b + 1], shapes[b:b + 1], o[b:b + 1], "min", p0=prices[b:b + 1], fast=True)
            one = {k: (a[b:b + 1] if isinstance(a, np.ndarray) else a) for k, a in got.items() if k != "meta"}
            one["meta"] = {k: a[b:b + 1] for k, a in got["meta"].items() if isinstance(a, np.ndarray)}
            outside_compare(one, 0, want, m_, n_)
        elif status[b] == 7:
            _condemned(got, b, 0, 0, 0)
        else:
            _condemned(got, b, n, m + n if with_outside else m, n * m + (n if with_outside else 0))
    first = int(np.flatnonzero(status)[0])
    with pytest.raises(ValueError, match=f"problem {first}: "):
        raise_for_status(res)
    with pytest.raises(ValueError, match=f"problem {first}: "):
        auction_solve_points_batch(dx, dy, shapes=ds, prices=dp, outside=do)
    # the problems a host call can take (host shapes are checked before the library): the same verdicts from numpy arrays
    keep = np.flatnonzero(status != 7)
    host = auction_solve_points_batch(np.ascontiguousarray(x[keep]), np.ascontiguousarray(y[keep]), shapes=shapes[keep],
                                      prices=prices[keep], outside=None if outside is None else outside[keep],
                                      errors="status")
    assert np.array_equal(host["status"], status[keep]) and np.array_equal(host["matching_size"], size[keep])
    assert np.array_equal(host["sol"], got["sol"][keep])
    for k in ("prices",) + (("outside_prices",) if with_outside else ()):
        assert np.array_equal(bits(host[k]), bits(got[k][keep])), k


def test_the_messages_of_raise_for_status():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1, 1, (1, 3, 2)), rng.uniform(-1, 1, (1, 4, 2))

    def message(x=x, y=y, **kw):
        with pytest.raises(ValueError) as e:
            auction_solve_points_batch(_dev(x), _dev(y), **kw)
        return str(e.value)
    bad = x.copy()
    bad[0, 1, 1] = np.nan
    assert "problem 0: a cost |x_i - y_j|^2 is not finite" in message(x=bad)
    assert "or an outside value is +inf" in message(outside=np.array([np.inf]))
    assert "Maximum matching possible only involves 2 out of 3 rows" in message(shapes=_dev(np.array([[3, 2]], dtype=np.int32)))
    assert "shape (0, 5) outside 1 .. 3 x 1 .. 4" in message(shapes=_dev(np.array([[0, 5]], dtype=np.int32)))
    assert "the outside value of row 1 is -2.0" in message(outside=np.array([[1.0, -2.0, 1.0]]))
    assert "prices hold a NaN" in message(prices=np.array([[0.0, np.nan, 0.0, 0.0]]))
    assert "prices must be >= 0" in message(prices=np.array([[0.0, 1.0, -0.0, 0.0]]))


# ---- views

def _raw(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_outside", [False, True])
def test_views_are_read_where_they_lie(dtype, with_outside):
    import torch
    rng = np.random.default_rng([51, DTYPES.index(dtype)])
    B, N, M, D = 5, 70, 130, 3
    x, y = draw("uniform", (B, N, D), dtype, rng), draw("uniform", (B, M, D), dtype, rng)
    shapes = np.array([[70, 130], [64, 65], [1, 1], [33, 129], [70, 70]], dtype=np.int32)
    outside = rng.uniform(0.0, 1.0, (B, N)) if with_outside else None
    p0 = rng.uniform(0, 1, (B, M))
    want = auction_solve_points_batch(x, y, shapes=shapes, prices=p0, outside=outside, errors="status")
    assert (want["status"] == 0).all()
    tdt = getattr(torch, dtype)
    # x: the first D columns of a (B, N, 7) track state; y: the transpose of a (B, D, M) buffer; both inside poisoned
    # storage (NaN: a coordinate read from it would condemn the problem)
    state = torch.full((B + 2, N + 2, 7), float("nan"), dtype=tdt)
    state[1:B + 1, 1:N + 1, :D] = torch.from_numpy(x.copy())
    state = state.cuda()
    xv = state[1:B + 1, 1:N + 1, :D]
    buf = torch.full((B, D + 1, M + 5), float("nan"), dtype=tdt)
    buf[:, :D, 2:M + 2] = torch.from_numpy(y.copy()).transpose(1, 2)
    buf = buf.cuda()
    yv = buf[:, :D, 2:M + 2].transpose(1, 2)
    assert tuple(xv.shape) == (B, N, D) and tuple(yv.shape) == (B, M, D) and not xv.is_contiguous() and yv.stride(2) != 1
    pbuf = torch.full((B, M + 8), float("nan"), dtype=torch.float64)
    pbuf[:, 4:M + 4] = torch.from_numpy(p0)
    pv = pbuf.cuda()[:, 4:M + 4]
    before = (_raw(state), _raw(buf))
    do = None if outside is None else _dev(outside)
    got = _host(auction_solve_points_batch(xv, yv, shapes=_dev(shapes), prices=pv, outside=do, errors="status"))
    _same(got, want, matching_size=True)
    assert (_raw(state), _raw(buf)) == before
    # one point set expanded over B (batch stride 0), different starting prices per problem
    one_y = _dev(y[:1]).expand(B, M, D)
    assert one_y.stride(0) == 0
    full = np.ascontiguousarray(np.broadcast_to(y[:1], (B, M, D)))
    want = auction_solve_points_batch(x, full, shapes=shapes, prices=p0, outside=outside, errors="status")
    got = _host(auction_solve_points_batch(xv, one_y, shapes=shapes, prices=p0, outside=do, errors="status"))
    _same(got, want, matching_size=True)
    assert len({want["prices"][b].tobytes() for b in (0, 4)}) == 2
    assert (_raw(state), _raw(buf)) == before


# ---- no wait

def test_the_device_call_does_not_wait_and_repeats_its_bits():
    import torch
    rng = np.random.default_rng(61)
    B, N, M, D = 96, 48, 64, 3
    x, y = draw("uniform", (B, N, D), "float32", rng), draw("uniform", (B, M, D), "float32", rng)
    outside = rng.uniform(0.0, 1.0, (B, N))
    want = auction_solve_points_batch(x, y, outside=outside, errors="status")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sx, dy, do = _dev(x), _dev(y), _dev(outside)
        dx = torch.full_like(sx, float("nan"))
        dx.copy_(sx)
        w = torch.randn(4096, 4096, device="cuda")
        first = auction_solve_points_batch(dx, dy, outside=do, errors="status")  # the warm-up call
        _busy(w, 2)
        torch.cuda.synchronize()
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
        queued = e[2].elapsed_time(e[3])
        assert queued >= 200.0, queued
        dx.fill_(float("nan"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(w, reps)
        dx.copy_(sx, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_points_batch(dx, dy, outside=do, errors="status")
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {queued:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < queued / 4, (t_call, queued)
    assert pending  # the producer chain was still running when the call came back
    got = _host(res)
    assert (got["status"] == 0).all()
    _same(got, want, matching_size=True)
    _same(_host(first), want, matching_size=True)
