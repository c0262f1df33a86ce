"""auction_solve_boxes_batch and boxes_candidates on the GPU (misslap_solve_boxes_batch, misslap_boxes_batch_candidates):
costs 1 - IoU and 1 - GIoU formed from the boxes, the cost stack never stored.  Every comparison is bit for bit, against
the oracle or the dense call on boxes_to_dense, and against boxes_to_ell.

  lane edges   both metrics x both types x plain / outside at M = 1, 63, 64, 65, 129 under N <= 9 rows with ragged shapes,
               the selects' pairs among them (for float64 the fused chain differs on the draw).
  outside      a scalar, (B,) and (B, N); m + i walks 72 consecutive values, so the virtual entry sits on every lane.
  sizes        N = 256, 257, 512, 513 (B = 1, M = N); one 2048 x 2048 problem with outside, "giou", fast=True.
  verdicts     a mixed batch: each status on one problem among solved ones, statuses derived on the CPU.
  views        a slice of a wider poisoned buffer, a transposed buffer, expanded boxes; nothing else is read or written.
  builder      lane / step edges; K = 1, 8, 64 with 0, K and K + 1 in-gate columns and ties; non-finite and bad-box
               pairs; 2048 x 2048 x 64.
  route        candidates=K is the ELL call on boxes_to_ell's lists, with prices= and finish="reverse".
  no wait      behind >= 200 ms of queued work the device call returns at once.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import (auction_solve_batch, auction_solve_boxes_batch, auction_solve_ell_batch, boxes_candidates,
                       boxes_to_dense, boxes_to_ell, raise_for_status)
from tests._batch_shapes import bits, dense_compare, dense_expect, threads_for
from tests._boxes_fixture import (DTYPES, METRICS, dense_by_loops, draw_boxes, expected_status, outside_rows, special_boxes,
                                  verdict_batch, verdict_table)
from tests._points_candidates import KEYS, same_bytes
from tests.test_dense_batch_status import _busy
from tests.test_dense_outside import compare as outside_compare, expect as outside_expect
from tests.test_points_batch import _condemned, _dev, _host, _raw, _same, check_plain
from tests.test_points_candidates import _lists, _same_as_ell

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- the lane edges, ragged shapes, the selects' pairs

EDGE_N, EDGE_M = 9, 129
EDGE_SHAPES = np.array([(1, 1), (9, 63), (9, 64), (8, 65), (9, 129), (5, 129), (3, 64), (2, 63), (7, 9), (1, 65), (9, 9)],
                       dtype=np.int32)


@functools.lru_cache(maxsize=None)
def edge_boxes(dtype):
    """(a, b): EDGE_SHAPES' problems in one call, NaN beyond every shape (a kernel that read it would report it); the
    last problem holds special_boxes' pairs, which take both branches of every select."""
    rng = np.random.default_rng([71, DTYPES.index(dtype)])
    B = len(EDGE_SHAPES)
    a, b = np.full((B, EDGE_N, 4), np.nan, dtype=dtype), np.full((B, EDGE_M, 4), np.nan, dtype=dtype)
    for p, (n, m) in enumerate(EDGE_SHAPES):
        kind = "grid" if p % 3 == 2 else "uniform"
        a[p, :n], b[p, :m] = draw_boxes(kind, (n, 4), dtype, rng), draw_boxes(kind, (m, 4), dtype, rng)
    sa, sb = special_boxes(dtype)
    a[-1, :7], b[-1, :9] = sa[0], sb[0]
    a[-1, 7:9] = draw_boxes("uniform", (2, 4), dtype, rng)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_edges_and_ragged_shapes_against_the_oracle(dtype, metric):
    a, b = edge_boxes(dtype)
    cost = boxes_to_dense(a, b, EDGE_SHAPES, metric)
    if dtype == "float64":  # a contracted chain is another function on this draw
        n, m = EDGE_SHAPES[4]
        assert (bits(dense_by_loops(a[4:5, :n], b[4:5, :m], metric=metric, fused=True)) != bits(cost[4:5, :n, :m])).any()
    da, db = _dev(a), _dev(b)
    for problem in ("min", "max"):
        got = auction_solve_boxes_batch(a, b, metric, problem=problem, shapes=EDGE_SHAPES, errors="status")
        assert got["layout"] == "boxes" and got["metric"] == metric and got["meta"]["gpu"]["threads"] == threads_for(EDGE_N)
        check_plain(got, cost, EDGE_SHAPES, problem)
        dev = auction_solve_boxes_batch(da, db, metric, problem=problem, shapes=_dev(EDGE_SHAPES), errors="status")
        assert dev["sol"].is_cuda and dev["layout"] == "boxes"
        _same(_host(dev), got, matching_size=True)
    raised = auction_solve_boxes_batch(da, db, metric=metric, shapes=EDGE_SHAPES)  # errors="raise": the same dict
    _same(_host(raised), auction_solve_boxes_batch(a, b, metric, shapes=EDGE_SHAPES, errors="status"), matching_size=True)
    # the dense batch on the stored stack: every output and every field of the records, also warm and cut short
    dc, ds = _dev(cost), _dev(EDGE_SHAPES)
    p0 = np.random.default_rng(5).uniform(0, 1, (len(EDGE_SHAPES), EDGE_M))
    for kw in (dict(), dict(prices=_dev(p0)), dict(eps_start=0.01), dict(fast=True), dict(max_iter=3), dict(problem="max")):
        x = _host(auction_solve_boxes_batch(da, db, metric, shapes=ds, errors="status", **kw))
        y = _host(auction_solve_batch(dc, shapes=ds, errors="status", cardinality_check=False, **kw))
        assert (x["status"] == 0).all()
        _same(x, y)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_edges_with_outside_against_the_oracle(dtype, metric):
    a, b = edge_boxes(dtype)
    cost = boxes_to_dense(a, b, EDGE_SHAPES, metric)
    rng = np.random.default_rng([72, DTYPES.index(dtype)])
    B = len(EDGE_SHAPES)
    outside = rng.uniform(0.4, 1.0 if metric == "iou" else 1.5, (B, EDGE_N))
    for p, (n, m) in enumerate(EDGE_SHAPES):
        i = np.arange(0, n, 3)
        outside[p, i] = cost[p, i, rng.integers(0, m, i.size)]  # a tie between an entry and the outside entry
        outside[p, n:] = np.nan
    got = auction_solve_boxes_batch(a, b, metric, shapes=EDGE_SHAPES, outside=outside, errors="status")
    assert (got["status"] == 0).all() and (got["matching_size"] == -1).all() and got["outside_prices"].shape == (B, EDGE_N)
    for p, (want, m, n) in enumerate(outside_expect(cost, EDGE_SHAPES, outside, "min", fast=True)):
        outside_compare(got, p, want, m, n)
    assert (got["sol"] == -1).any() and (got["sol"] >= 0).any()
    da, db, ds, do = _dev(a), _dev(b), _dev(EDGE_SHAPES), _dev(outside)
    _same(_host(auction_solve_boxes_batch(da, db, metric, shapes=ds, outside=do, errors="status")), got, matching_size=True)
    _same(_host(auction_solve_batch(_dev(cost), shapes=ds, outside=do, errors="status")), got, matching_size=True)


# ---- outside in its three forms, the virtual entry on every lane

OUT_N, OUT_M = 9, 72


@functools.lru_cache(maxsize=None)
def outside_boxes(dtype):
    """72 problems of up to 9 rows with m_b = 1 .. 72 columns: (m_b + i) & 63 takes every value; n_b > m_b at the start."""
    rng = np.random.default_rng([73, DTYPES.index(dtype)])
    B = OUT_M
    a, b = draw_boxes("uniform", (B, OUT_N, 4), dtype, rng), draw_boxes("uniform", (B, OUT_M, 4), dtype, rng)
    shapes = np.array([(OUT_N if p % 3 else 1 + (7 * p) % OUT_N, p + 1) for p in range(B)], dtype=np.int32)
    for t in (a, b, shapes):
        t.setflags(write=False)
    return a, b, shapes


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
@pytest.mark.parametrize("metric", METRICS)
def test_outside_forms_with_the_virtual_entry_on_every_lane(metric, form):
    lanes = set()
    for dtype in DTYPES:
        a, b, shapes = outside_boxes(dtype)
        B = len(shapes)
        lanes |= {(int(m) + i) & 63 for n, m in shapes for i in range(n)}
        cost = boxes_to_dense(a, b, shapes, metric)
        rng = np.random.default_rng(9)
        outside = {"scalar": 0.7, "per_problem": rng.uniform(0.3, 1.2, B), "per_row": rng.uniform(0.3, 1.2, (B, OUT_N))}[form]
        p0 = rng.uniform(0, 1, (B, OUT_M))
        da, db, dc, ds = _dev(a), _dev(b), _dev(cost), _dev(shapes)
        o = outside if form == "scalar" else _dev(outside)
        for kw in (dict(), dict(eps_start=1e-3), dict(fast=False), dict(prices=p0), dict(max_iter=5), dict(problem="max")):
            got = _host(auction_solve_boxes_batch(da, db, metric, shapes=ds, outside=o, errors="status", **kw))
            dense = _host(auction_solve_batch(dc, shapes=ds, outside=o, errors="status", **kw))
            assert (got["status"] == 0).all()
            _same(got, dense, matching_size=True)
        host = auction_solve_boxes_batch(a, b, metric, shapes=shapes, outside=outside, errors="status")
        _same(host, _host(auction_solve_batch(dc, shapes=ds, outside=o, errors="status")), matching_size=True)
        pick = [0, 1, 7, 62, 63, 64, 71]  # ... and the oracle on dense_to_augmented, as the front end resolves the call
        ob = outside if form == "scalar" else outside[pick]
        for k, (want, m, n) in enumerate(outside_expect(np.ascontiguousarray(cost[pick]), shapes[pick], ob, "min", fast=True)):
            one = {key: (v[pick] if isinstance(v, np.ndarray) else v) for key, v in host.items() if key != "meta"}
            one["meta"] = {key: v[pick] for key, v in host["meta"].items() if isinstance(v, np.ndarray)}
            outside_compare(one, k, want, m, n)
    assert lanes == set(range(64))


# ---- the workgroup sizes and the cap

def _crowd(n, m, dtype, seed):
    """n and m boxes over a field wide enough that a box overlaps a handful of the others."""
    rng = np.random.default_rng(seed)
    span = max(int(np.sqrt(max(n, m)) / 1.5), 3)
    return draw_boxes("uniform", (1, n, 4), dtype, rng, span), draw_boxes("uniform", (1, m, 4), dtype, rng, span)


@pytest.mark.parametrize("N", [256, 257, 512, 513])
def test_each_workgroup_size(N):
    for metric, dtype in (("iou", "float32"), ("giou", "float64")):
        a, b = _crowd(N, N, dtype, [41, N])
        cost = boxes_to_dense(a, b, metric=metric)
        assert 2.0 < (cost[0] < 1.0).sum(axis=1).mean() < N / 4
        got = _host(auction_solve_boxes_batch(_dev(a), _dev(b), metric, errors="status"))
        assert got["meta"]["gpu"]["threads"] == threads_for(N) and got["status"][0] == 0
        _same(got, _host(auction_solve_batch(_dev(cost), errors="status", cardinality_check=False)), matching_size=False)
        assert got["matching_size"][0] == N and got["meta"]["n_assigned"][0] == N
    a, b = _crowd(N, N, "float32", [42, N])  # ... and once against the oracle itself, with outside (few rounds)
    outside = np.random.default_rng(N).uniform(0.3, 0.9, (1, N))
    got = _host(auction_solve_boxes_batch(_dev(a), _dev(b), "iou", outside=_dev(outside), errors="status"))
    ((want, m, n),) = outside_expect(boxes_to_dense(a, b), None, outside, "min", fast=True)
    outside_compare(got, 0, want, m, n)


def test_the_cap_2048_x_2048_with_outside_giou_fast():
    a, b = _crowd(2048, 2048, "float64", 33)
    outside = np.random.default_rng(34).uniform(0.5, 1.2, (1, 2048))
    got = _host(auction_solve_boxes_batch(_dev(a), _dev(b), "giou", outside=_dev(outside), fast=True, errors="status"))
    assert got["meta"]["gpu"]["lds_bytes"] == 155648 and got["meta"]["gpu"]["threads"] == 1024 and got["status"][0] == 0
    ((want, m, n),) = outside_expect(boxes_to_dense(a, b, metric="giou"), None, outside, "min", fast=True)
    outside_compare(got, 0, want, m, n)
    assert (got["sol"][0] == -1).any() and (got["sol"][0] >= 0).sum() > 500


# ---- verdicts

@pytest.mark.parametrize("with_outside", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_verdicts_of_a_mixed_batch(dtype, metric, with_outside):
    v = verdict_batch(dtype)
    a, b, shapes, prices, kinds = v["a"], v["b"], v["shapes"], v["prices"], v["kinds"]
    outside = v["outside"] if with_outside else None
    B, N = a.shape[0], a.shape[1]
    status, size = expected_status(a, b, shapes, prices, outside, metric)
    for p, kind in enumerate(kinds):  # the table, from the definition alone
        assert status[p] == verdict_table(kind, metric, with_outside, dtype == "float64"), (p, kind, status[p])
    cost = boxes_to_dense(a, b, metric=metric)
    da, db, ds, dp = _dev(a), _dev(b), _dev(shapes), _dev(prices)
    do = None if outside is None else _dev(outside)
    res = auction_solve_boxes_batch(da, db, metric, shapes=ds, prices=dp, outside=do, errors="status")
    got = _host(res)
    assert np.array_equal(got["status"], status), (got["status"], status)
    assert np.array_equal(got["matching_size"], size), (got["matching_size"], size)
    o = None if outside is None else outside_rows(outside, B, N)
    for p in range(B):
        n, m = (int(s) for s in shapes[p])
        if status[p] == 0 and outside is None:
            want = dense_expect(cost[p, :n, :m], "min", p0=prices[p], cardinality_check=False)
            dense_compare(got, p, want, n, m, p0=prices[p])
        elif status[p] == 0:
            ((want, m_, n_),) = outside_expect(cost[p:p + 1], shapes[p:p + 1], o[p:p + 1], "min", p0=prices[p:p + 1], fast=True)
            one = {k: (t[p:p + 1] if isinstance(t, np.ndarray) else t) for k, t in got.items() if k != "meta"}
            one["meta"] = {k: t[p:p + 1] for k, t in got["meta"].items() if isinstance(t, np.ndarray)}
            outside_compare(one, 0, want, m_, n_)
        elif status[p] == 7:
            _condemned(got, p, 0, 0, 0)
        else:
            _condemned(got, p, n, m + n if with_outside else m, n * m + (n if with_outside else 0))
    first = int(np.flatnonzero(status)[0])
    with pytest.raises(ValueError, match=f"problem {first}: a box cost is not finite"):
        raise_for_status(res)
    with pytest.raises(ValueError, match=f"problem {first}: "):
        auction_solve_boxes_batch(da, db, metric, shapes=ds, prices=dp, outside=do)
    box = kinds.index("bad_box_row")
    with pytest.raises(ValueError, match="problem 0: a box has x2 < x1 or y2 < y1"):
        auction_solve_boxes_batch(da[box:box + 1], db[box:box + 1], metric, shapes=ds[box:box + 1].contiguous())
    # the problems a host call can take (host shapes are checked before the library): the same verdicts from numpy arrays
    keep = np.flatnonzero(status != 7)
    host = auction_solve_boxes_batch(np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep]), metric,
                                     shapes=shapes[keep], prices=prices[keep],
                                     outside=None if outside is None else outside[keep], errors="status")
    assert np.array_equal(host["status"], status[keep]) and np.array_equal(host["matching_size"], size[keep])
    assert np.array_equal(host["sol"], got["sol"][keep])
    for k in ("prices",) + (("outside_prices",) if with_outside else ()):
        assert np.array_equal(bits(host[k]), bits(got[k][keep])), k
    # the list route has no BAD_BOX: the builder stores the pair as +inf and the ELL call says INFINITE_VALUE
    if with_outside:
        route = auction_solve_boxes_batch(da, db, metric, shapes=ds, outside=do, candidates=8, errors="status")
        rs = route["status"].cpu().numpy()
        for p, kind in enumerate(kinds):
            if kind in ("bad_box_row", "bad_box_col", "bad_box_and_n_gt_m", "nan_coord", "overflow_width"):
                assert rs[p] == 3, (p, kind, rs[p])
            elif kind == "ok":
                assert rs[p] == 0, (p, rs[p])


# ---- views

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_outside", [False, True])
def test_views_are_read_where_they_lie(dtype, with_outside):
    import torch
    rng = np.random.default_rng([51, DTYPES.index(dtype)])
    B, N, M = 5, 70, 130
    a, b = draw_boxes("uniform", (B, N, 4), dtype, rng, 6), draw_boxes("uniform", (B, M, 4), dtype, rng, 6)
    shapes = np.array([[70, 130], [64, 65], [1, 1], [33, 129], [70, 70]], dtype=np.int32)
    outside = rng.uniform(0.3, 1.0, (B, N)) if with_outside else None
    p0 = rng.uniform(0, 1, (B, M))
    want = auction_solve_boxes_batch(a, b, "giou", shapes=shapes, prices=p0, outside=outside, errors="status")
    assert (want["status"] == 0).all()
    tdt = getattr(torch, dtype)
    # a: the first 4 columns of a (B, N, 7) track state inside a wider buffer; b: the transpose of a (B, 4, M) buffer;
    # both inside poisoned storage (NaN: a coordinate read from it would condemn the problem)
    state = torch.full((B + 2, N + 2, 7), float("nan"), dtype=tdt)
    state[1:B + 1, 1:N + 1, :4] = torch.from_numpy(a.copy())
    state = state.cuda()
    av = state[1:B + 1, 1:N + 1, :4]
    buf = torch.full((B, 5, M + 5), float("nan"), dtype=tdt)
    buf[:, :4, 2:M + 2] = torch.from_numpy(b.copy()).transpose(1, 2)
    buf = buf.cuda()
    bv = buf[:, :4, 2:M + 2].transpose(1, 2)
    assert tuple(av.shape) == (B, N, 4) and tuple(bv.shape) == (B, M, 4) and not av.is_contiguous() and bv.stride(2) != 1
    before = (_raw(state), _raw(buf))
    do = None if outside is None else _dev(outside)
    got = _host(auction_solve_boxes_batch(av, bv, "giou", shapes=_dev(shapes), prices=_dev(p0), outside=do, errors="status"))
    _same(got, want, matching_size=True)
    lists = _lists(boxes_candidates(av, bv, 8, shapes=_dev(shapes), limit=do, metric="giou"))
    assert same_bytes(lists, boxes_to_ell(a, b, 8, shapes, outside, "giou"))
    assert (_raw(state), _raw(buf)) == before
    # one box set expanded over B (batch stride 0), and one box expanded over the rows (row stride 0)
    one_b = _dev(b[:1]).expand(B, M, 4)
    one_a = _dev(a[:, :1]).expand(B, N, 4)
    assert one_b.stride(0) == 0 and one_a.stride(1) == 0
    fb = np.ascontiguousarray(np.broadcast_to(b[:1], (B, M, 4)))
    fa = np.ascontiguousarray(np.broadcast_to(a[:, :1], (B, N, 4)))
    for (xa, xb), (ha, hb) in (((av, one_b), (a, fb)), ((one_a, bv), (fa, b))):
        want_e = auction_solve_boxes_batch(ha, hb, "iou", shapes=shapes, prices=p0, outside=outside, errors="status")
        got_e = _host(auction_solve_boxes_batch(xa, xb, "iou", shapes=shapes, prices=p0, outside=do, errors="status"))
        _same(got_e, want_e, matching_size=True)
        lists = _lists(boxes_candidates(xa, xb, 8, shapes=_dev(shapes), limit=do))
        assert same_bytes(lists, boxes_to_ell(ha, hb, 8, shapes, outside))
    assert (_raw(state), _raw(buf)) == before


# ---- the builder

def check_builder(a, b, k, metric, shapes=None, limit=None):
    """boxes_candidates on device tensors is boxes_to_ell."""
    lim = _dev(limit) if isinstance(limit, np.ndarray) else limit
    got = _lists(boxes_candidates(_dev(a), _dev(b), k, shapes=shapes, limit=lim, metric=metric))
    want = boxes_to_ell(a, b, k, shapes, limit, metric)
    for key in KEYS:
        assert got[key].tobytes() == want[key].tobytes(), (key, k, np.flatnonzero(got[key].ravel() != want[key].ravel())[:8])
    return got


@pytest.mark.parametrize("M", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("N", [1, 3, 4, 5])
def test_builder_lane_and_step_edges(gpu_lib, M, N):
    rng = np.random.default_rng([2, M, N])
    for metric, dtype, kind in (("iou", "float32", "grid"), ("giou", "float64", "uniform")):
        a, b = draw_boxes(kind, (3, N, 4), dtype, rng), draw_boxes(kind, (3, M, 4), dtype, rng)
        cost = boxes_to_dense(a, b, metric=metric)
        per_row = np.sort(cost, axis=2)[:, :, min(M - 1, 2)] + np.array([0.0, 1e-3, -1.0, np.nan, np.inf])[np.arange(N) % 5]
        for k in (1, 8, 64):
            for limit in (None, per_row, 0.9, np.array([0.5, -0.0, 100.0])):
                check_builder(a, b, k, metric, limit=limit)
        shapes = np.array([[N, M], [max(N - 1, 1), max(M - 1, 1)], [0, M]], dtype=np.int32)
        check_builder(a, b, 8, metric, shapes=_dev(shapes), limit=0.9)


def counted_boxes(dtype, k, M):
    """a (1, 4, 4), b (1, M, 4) and a per-row limit: every row is the unit square and column j is the unit square
    stretched to height 1 + j, so a row's costs j / (1 + j) grow with j and the rows have 0, exactly k, k + 1 and M
    candidates (M >= k + 1)."""
    a = np.tile(np.array([0.0, 0.0, 1.0, 1.0], dtype=dtype), (1, 4, 1))
    b = np.array([[0.0, 0.0, 1.0, 1.0 + j] for j in range(M)], dtype=dtype)[None]
    cost = boxes_to_dense(a, b)[0, 0]
    assert (np.diff(cost) > 0).all() and cost[0] == 0.0
    return a, b, np.array([[-1.0, cost[k - 1], cost[k], np.inf]]), np.array([0, k, k + 1, M])


def tied_boxes(dtype, M):
    """a (1, 2, 4), b (1, M, 4): every column but the last is row 0's 2 x 2 square moved one unit in one of four
    directions (IoU 1/3 each, the same bits), the last IS row 0, so under truncation the last column comes first and
    the ties go by column; row 1 sees ties of two values."""
    moves = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [-1, 0, -1, 0], [0, -1, 0, -1]], dtype=dtype)
    square = np.array([0, 0, 2, 2], dtype=dtype)
    b = np.concatenate([square + moves[np.arange(M - 1) % 4], square[None]])[None]
    a = np.array([[[0, 0, 2, 2], [1, 1, 4, 3]]], dtype=dtype)
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 8, 64])
def test_builder_zero_k_and_k_plus_one_candidates_and_ties(gpu_lib, dtype, k):
    for M in (k + 3, 130):
        a, b, lim, counts = counted_boxes(dtype, k, M)
        got = check_builder(a, b, k, "iou", limit=lim)
        assert got["counts"][0].tolist() == counts.tolist()
        assert got["cols"][0, 1].tolist() == list(range(k)) == got["cols"][0, 2].tolist()
    for M in (11, 65, 131):
        a, b = tied_boxes(dtype, M)
        for metric in METRICS:
            got = check_builder(a, b, k, metric)
            if k < M:
                assert got["cols"][0, 0].tolist() == sorted([M - 1] + list(range(k - 1))), (M, k)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_builder_non_finite_and_bad_box_pairs(gpu_lib, dtype, metric):
    v = verdict_batch(dtype)
    for limit in (None, -1.0, 0.7, float("nan")):
        for k in (1, 3, 11):
            got = check_builder(v["a"], v["b"], k, metric, shapes=_dev(v["shapes"]), limit=limit)
            assert not np.isnan(got["vals"]).any()
    for p, kind in enumerate(v["kinds"]):
        if kind in ("nan_coord", "inf_coord", "overflow_width", "overflow_area", "bad_box_row", "bad_box_col", "nan_and_bad_box"):
            assert np.isposinf(got["vals"][p]).any(), kind
        elif kind in ("ok", "zero_size", "price_nan"):
            assert np.isfinite(got["vals"][p]).all(), kind
    hull = v["kinds"].index("overflow_hull")
    assert np.isposinf(got["vals"][hull]).any() == (metric == "giou" or dtype == "float32")


def test_builder_2048_by_2048_with_64_candidates(gpu_lib):
    a, b = _crowd(2048, 2048, "float32", 8)
    rng = np.random.default_rng(8)
    cost = boxes_to_dense(a, b, metric="giou")
    # the limit of a row is its r-th smallest cost, r = 40 .. 89: r + 1 in-gate columns, both paths at the last step
    limit = np.take_along_axis(np.sort(cost[0], axis=1), rng.integers(40, 90, (2048, 1)), axis=1)[:, 0][None]
    got = check_builder(a, b, 64, "giou", limit=np.ascontiguousarray(limit))
    assert (got["counts"] > 64).sum() > 100 and (got["counts"] < 64).sum() > 100


# ---- end to end: the keyword route

@pytest.mark.parametrize("metric", METRICS)
def test_the_keyword_route_is_the_ell_call_on_the_lists(gpu_lib, metric):
    rng = np.random.default_rng(14)
    B, N, M = 5, 9, 13
    a, b = draw_boxes("grid", (B, N, 4), "float32", rng), draw_boxes("grid", (B, M, 4), "float32", rng)
    a[4], b[4] = draw_boxes("uniform", (N, 4), "float32", rng), draw_boxes("uniform", (M, 4), "float32", rng)
    outside = rng.uniform(0.5, 1.1, (B, N))
    prices = rng.uniform(0, 1, (B, M))
    shapes = np.array([[9, 13], [4, 13], [9, 5], [1, 1], [9, 12]])
    da, db, do = _dev(a), _dev(b), _dev(outside)
    for k in (3, 13):
        for kw in (dict(), dict(shapes=shapes), dict(prices=_dev(prices), finish="reverse"), dict(finish="reverse"),
                   dict(eps_start=1e-3, prices=_dev(prices), finish="reverse")):
            res = auction_solve_boxes_batch(da, db, metric, outside=do, candidates=k, errors="status", **kw)
            ell = boxes_to_ell(a, b, k, kw.get("shapes"), outside, metric)
            ekw = {key: v for key, v in kw.items() if key != "shapes"}
            ref = auction_solve_ell_batch(_dev(ell["cols"]), _dev(ell["vals"]), rows=_dev(ell["rows"]), n_cols=M,
                                          problem="min", outside=do, errors="status", **ekw)
            _same_as_ell(res, ref, reverse="finish" in kw)
            assert same_bytes(_lists(res["candidates"]), ell)
            assert res["truncated"].cpu().numpy().tolist() == (ell["counts"] > k).sum(axis=1).tolist()
    # where nothing was truncated the objective is the full call's (at an eps that makes both optimal within 9e-4)
    res = auction_solve_boxes_batch(da, db, metric, outside=do, candidates=13, eps_start=1e-4, errors="status")
    full = _host(auction_solve_boxes_batch(da, db, metric, outside=do, eps_start=1e-4, errors="status"))
    assert (res["truncated"].cpu().numpy() == 0).all() and (full["status"] == 0).all()
    assert np.abs(res["meta"]["obj_f64"].cpu().numpy() - full["meta"]["obj_f64"]).max() <= 2 * N * 1e-4
    host = auction_solve_boxes_batch(a, b, metric, outside=outside, candidates=13, eps_start=1e-4, errors="status")
    assert isinstance(host["sol"], np.ndarray) and np.array_equal(host["sol"], res["sol"].cpu().numpy())
    assert isinstance(host["candidates"]["cols"], np.ndarray) and same_bytes(host["candidates"], _lists(res["candidates"]))
    # the builder alone, from numpy arrays
    alone = boxes_candidates(a, b, 3, limit=outside, metric=metric)
    assert isinstance(alone["cols"], np.ndarray) and same_bytes(alone, boxes_to_ell(a, b, 3, None, outside, metric))


# ---- no wait

def test_the_device_call_does_not_wait():
    import torch
    rng = np.random.default_rng(62)
    B, N, M = 96, 48, 64
    a, b = draw_boxes("uniform", (B, N, 4), "float32", rng, 5), draw_boxes("uniform", (B, M, 4), "float32", rng, 5)
    outside = rng.uniform(0.3, 1.0, (B, N))
    want = auction_solve_boxes_batch(a, b, "giou", outside=outside, errors="status")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        sa, db, do = _dev(a), _dev(b), _dev(outside)
        da = torch.full_like(sa, float("nan"))
        da.copy_(sa)
        busy = torch.randn(4096, 4096, device="cuda")
        first = auction_solve_boxes_batch(da, db, "giou", outside=do, errors="status")  # the warm-up call
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
        da.fill_(float("nan"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(busy, reps)
        da.copy_(sa, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_boxes_batch(da, db, "giou", outside=do, errors="status")
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
