"""auction_solve_points_batch(finish="reverse") on the GPU (misslap_points_batch_reverse_finish, k_points_reverse_finish
in csrc/kernels_points_finish.hpp).

The yardstick is always sslap_amd.points_reverse_finish, the numpy model, applied to the outputs of the SAME call with
finish left out (the forward solve is pinned to the dense call and the oracle elsewhere); everything is compared bit for bit
(tests/_dense_finish.py: assert_is_the_model): sol, prices, outside_prices, reverse.its, reverse.left, meta.obj_f64 /
obj_f32 / eCE, and every other meta field, status and matching_size unchanged.  Every test calls finish="reverse" on the
points call, which the parent of this kernel does not have.
"""
import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, auction_solve_points_batch, batch_meta_to_host, points_batch, points_to_dense
from tests import _dense_finish as df
from tests import _points_finish as pf

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _points(rng, B, n, m, D=2, dtype="float64", hi=10.0):
    return rng.uniform(0, hi, (B, n, D)).astype(dtype), rng.uniform(0, hi, (B, m, D)).astype(dtype)


def _same(ra, rb, keys=("sol", "prices", "outside_prices", "status", "matching_size")):
    """two finished device results, bit for bit: the outputs, reverse and every field of the records"""
    for key in keys:
        assert (key in ra) == (key in rb), key
        if key in ra:
            assert df.host(ra[key]).tobytes() == df.host(rb[key]).tobytes(), key
    for key in ("its", "left"):
        assert np.array_equal(df.host(ra["reverse"][key]), df.host(rb["reverse"][key])), key
    assert df.records(ra).tobytes() == df.records(rb).tobytes()


@pytest.mark.parametrize("outside", [None, 60.0])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 2), (63, 64), (64, 65), (65, 130)])
def test_the_edges_of_the_row_scan(gpu_lib, n, m, outside):
    rng = np.random.default_rng(1000 * n + m)
    x, y = _points(rng, 3, n, m)
    kw = dict(fast=True, prices=rng.uniform(0, 100, (3, m)))
    if outside is not None:
        kw["outside"] = outside
    _, _, want = pf.check(_dev(x), _dev(y), **kw)
    assert want["ran"].all() and (want["reverse"]["left"] == 0).all()
    if n >= 63:
        assert (want["reverse"]["its"] > 0).all(), want["reverse"]["its"]


def _few_priced(rng, B, m, count=40):
    """starting prices that are non-zero on `count` objects only"""
    p = np.zeros((B, m))
    for b in range(B):
        p[b, rng.choice(m, count, replace=False)] = rng.uniform(0.5, 1.5, count)
    return p


def test_past_the_dense_cap_the_17th_row_of_a_lane(gpu_lib):
    """1025 x 1040 without outside: the first shape with a 17th row per lane."""
    rng = np.random.default_rng(1025)
    x, y = _points(rng, 1, 1025, 1040, hi=1.0)
    _, _, want = pf.check(_dev(x), _dev(y), fast=True, prices=_few_priced(rng, 1, 1040))
    print("1025 x 1040: its", want["reverse"]["its"].tolist())
    assert want["ran"].all() and (want["reverse"]["its"] > 0).all() and (want["reverse"]["left"] == 0).all()


def test_past_the_dense_cap_the_full_carve(gpu_lib):
    """2048 x 2048 with outside at B = 1: 4096 objects and 2048 rows in LDS (73 728 bytes), the 32nd row per lane."""
    rng = np.random.default_rng(2048)
    x, y = _points(rng, 1, 2048, 2048, hi=1.0)
    _, _, want = pf.check(_dev(x), _dev(y), fast=True, outside=rng.uniform(0.0005, 0.002, (1, 2048)),
                          prices=_few_priced(rng, 1, 2048))
    print("2048 x 2048 with outside: its", want["reverse"]["its"].tolist())
    assert want["ran"].all() and (want["reverse"]["its"] > 0).all() and (want["reverse"]["left"] == 0).all()


@pytest.mark.parametrize("outside", [False, True])
def test_the_dense_route_agrees_where_both_exist(gpu_lib, outside):
    rng = np.random.default_rng(7 + outside)
    B, n, m = 4, 40, 70
    x, y = _points(rng, B, n, m, D=3)
    shapes = np.array([[40, 70], [17, 70], [40, 41], [1, 5]], dtype=np.int32)
    kw = dict(shapes=shapes, fast=True, prices=rng.uniform(0, 200, (B, m)), problem=("min", "max")[outside])
    if outside:
        kw["outside"] = rng.uniform(20, 80, (B, n))
    got = auction_solve_points_batch(_dev(x), _dev(y), errors="status", finish="reverse", **kw)
    ref = auction_solve_batch(_dev(points_to_dense(x, y, shapes)), errors="status", finish="reverse",
                              cardinality_check=False, **kw)
    _same(got, ref, keys=("sol", "prices", "outside_prices", "status"))  # (matching_size: the dense call ran no guard)
    assert (df.host(got["status"]) == 0).all() and (df.host(got["reverse"]["its"]) > 0).any()


@pytest.mark.parametrize("D", pf.DIMS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_both_coordinate_types_every_dimension_and_both_problems(gpu_lib, dtype, D):
    rng = np.random.default_rng(10 * D + (dtype == "float32"))
    x, y = _points(rng, 3, 20, 33, D=D, dtype=dtype)
    for problem in ("min", "max"):
        for kw in (dict(), dict(outside=rng.uniform(5, 40, (3, 20)))):
            _, _, want = pf.check(_dev(x), _dev(y), problem=problem, fast=True, prices=rng.uniform(0, 300, (3, 33)), **kw)
            assert want["ran"].all() and (want["reverse"]["its"] > 0).any()


@pytest.mark.parametrize("view", ["state_slice", "transposed", "expanded"])
def test_strided_views_equal_their_contiguous_copies(gpu_lib, view):
    rng = np.random.default_rng(5)
    B, n, m, D = 3, 24, 40, 2
    x, y = _dev(rng.uniform(0, 10, (B, n, D))), _dev(rng.uniform(0, 10, (B, m, D)))
    if view == "state_slice":
        x = _dev(rng.uniform(0, 10, (B, n, 7)))[..., :2]
    elif view == "transposed":
        y = _dev(rng.uniform(0, 10, (B, D, m))).transpose(1, 2)
    else:
        y = _dev(rng.uniform(0, 10, (1, m, D)))[0].expand(B, m, D)
    assert not (x.is_contiguous() and y.is_contiguous())
    for kw in (dict(), dict(outside=rng.uniform(5, 40, (B, n)))):
        kw.update(fast=True, prices=rng.uniform(0, 150, (B, m)))
        _, r1, want = pf.check(x, y, **kw)
        assert (want["reverse"]["its"] > 0).all()
        _same(r1, auction_solve_points_batch(x.contiguous(), y.contiguous(), errors="status", finish="reverse", **kw))


def _forward_of(r0):
    rec = df.records(r0)
    return dict(sol=df.host(r0["sol"]), prices=df.host(r0["prices"]), final_eps=rec["final_eps"],
                outside_prices=df.host(r0["outside_prices"]) if "outside_prices" in r0 else None)


def test_ties_the_smaller_row_wins(gpu_lib):
    case, trace = pf.ties_case(), []
    r0, _, want = pf.check(_dev(case["x"]), _dev(case["y"]), trace=trace, **case["kw"])
    assert want["ran"].all()
    fwd = _forward_of(r0)
    ties = [pf.beta_ties(case["x"], case["y"], case["kw"]["problem"], None, fwd, b, [t[1:] for t in trace if t[0] == b])
            for b in range(case["x"].shape[0])]
    print("moves whose beta two rows share:", ties)
    assert sum(ties) >= 1


def test_chains_and_drops(gpu_lib):
    case, trace = pf.chains_case(), []
    _, _, want = pf.check(_dev(case["x"]), _dev(case["y"]), trace=trace, **case["kw"])
    assert want["ran"].all() and pf.holds_chain_and_drop(trace), trace[:8]


def test_condemned_problems_between_solved_ones_are_untouched(gpu_lib):
    rng = np.random.default_rng(17)
    B, n, m = 6, 10, 16
    x, y = _points(rng, B, n, m)
    x[1, 3, 1] = np.nan
    shapes = _dev(np.array([[10, 16], [10, 16], [0, 99999], [10, 16], [10, 9], [10, 16]], dtype=np.int32))
    for kw in (dict(), dict(outside=50.0)):
        r0, r1, want = pf.check(_dev(x), _dev(y), shapes=shapes, fast=True, prices=rng.uniform(0, 150, (B, m)), **kw)
        n_gt_m = _lib.BATCH_STATUS_INFEASIBLE if not kw else 0  # (with outside n_b > m_b is solved)
        assert df.host(r1["status"]).tolist() == [0, _lib.BATCH_STATUS_INFINITE_VALUE, _lib.BATCH_STATUS_BAD_SHAPE, 0, n_gt_m, 0]
        bad = [1, 2] if kw else [1, 2, 4]
        its, left = df.host(r1["reverse"]["its"]), df.host(r1["reverse"]["left"])
        assert (its[bad] == -1).all() and (left[bad] == -1).all()
        good = [b for b in range(B) if b not in bad]
        assert (its[good] > 0).all() and (left[good] == 0).all()


def test_a_forward_solve_cut_by_max_iter_is_untouched(gpu_lib):
    rng = np.random.default_rng(19)
    x, y = _points(rng, 3, 30, 45)
    shapes = np.array([[30, 45], [1, 45], [30, 45]], dtype=np.int32)  # (problem 1: one row, solved in one round)
    r0, r1, want = pf.check(_dev(x), _dev(y), shapes=shapes, max_iter=1, prices=rng.uniform(0, 150, (3, 45)), fast=True)
    assert (df.host(r1["status"]) == 0).all()
    assert want["ran"].tolist() == [False, True, False]
    assert df.host(r1["reverse"]["its"])[[0, 2]].tolist() == [-1, -1] and df.host(r1["reverse"]["left"])[[0, 2]].tolist() == [-1, -1]


def test_the_budget_cuts_the_finish_like_the_model(gpu_lib):
    """Few rows and many objects from high prices: the forward solve takes a few rounds, the finish one iteration per
    abandoned object.  max_iter between the two cuts the finish only."""
    rng = np.random.default_rng(23)
    x, y = _points(rng, 3, 6, 150)
    xd, yd, prices = _dev(x), _dev(y), rng.uniform(100, 400, (3, 150))
    r0, _, full = pf.check(xd, yd, fast=True, prices=prices)
    forward = int(batch_meta_to_host(r0)["its"].max())
    assert (full["reverse"]["its"] > forward + 5).all(), (forward, full["reverse"]["its"])
    _, r1, cut = pf.check(xd, yd, fast=True, prices=prices, max_iter=forward + 5)
    assert cut["ran"].all() and (cut["reverse"]["its"] == forward + 5).all() and (cut["reverse"]["left"] > 0).all()
    assert np.array_equal(df.host(r1["reverse"]["left"]), cut["reverse"]["left"])


def test_the_stall_rule(gpu_lib):
    """The forward result of integer-grid problems with outside, final_eps rewritten to 2**-60 in the device records of
    both results, then the finish alone with a budget of 5 000 (a kernel without the rule still ends): some problem's
    trace ends in a stalled iteration, and its, left and eCE are the model's."""
    import torch
    case = pf.stall_case()
    xd, yd, kw = _dev(case["x"]), _dev(case["y"]), case["kw"]
    r0 = auction_solve_points_batch(xd, yd, errors="status", **kw)
    r1 = auction_solve_points_batch(xd, yd, errors="status", **kw)
    off = _lib.DenseBatchMeta.final_eps.offset
    eps = torch.from_numpy(np.frombuffer(np.float32(pf.STALL_EPS).tobytes(), dtype=np.uint8).copy()).cuda()
    for r in (r0, r1):
        with torch.cuda.stream(r["stream"]):
            r["records"][:, off:off + 4] = eps
    assert (df.records(r0)["final_eps"] == np.float32(pf.STALL_EPS)).all()
    points_batch._reverse_finish_launch(xd, yd, r1, kw["problem"], 5000)
    trace = []
    want = pf.model_of(xd, yd, r0, trace=trace, **dict(kw, max_iter=5000))
    assert want["ran"].all() and pf.holds_stall(trace), trace[-4:]
    stalled = sorted({t[0] for t in trace if t[2] >= 0 and t[3] == -1})
    print("stalled problems:", stalled, "its", want["reverse"]["its"].tolist(), "left", want["reverse"]["left"].tolist())
    assert (want["reverse"]["left"][stalled] > 0).all() and (want["reverse"]["its"][stalled] < 5000).all()
    df.assert_is_the_model(r1, r0, want)


@pytest.mark.parametrize("outside", [None, 55.0])
def test_numpy_point_sets_take_the_device_route_and_return_numpy(gpu_lib, outside):
    rng = np.random.default_rng(31)
    x, y = _points(rng, 3, 12, 20)
    kw = dict(fast=True, prices=rng.uniform(0, 100, (3, 20)))
    if outside is not None:
        kw["outside"] = outside
    dev = auction_solve_points_batch(_dev(x), _dev(y), errors="status", finish="reverse", **kw)
    for errors in ("status", "raise"):
        got = auction_solve_points_batch(x, y, errors=errors, finish="reverse", **kw)
        assert not {"records", "info", "stream", "keep"} & set(got)
        for key in ("sol", "prices", "status", "matching_size") + (() if outside is None else ("outside_prices",)):
            assert isinstance(got[key], np.ndarray) and got[key].tobytes() == df.host(dev[key]).tobytes(), key
        for key in ("its", "left"):
            assert isinstance(got["reverse"][key], np.ndarray) and np.array_equal(got["reverse"][key], df.host(dev["reverse"][key]))
        want_meta = batch_meta_to_host(dev)
        for key in set(want_meta) - {"timer", "gpu"}:
            assert got["meta"][key].tobytes() == want_meta[key].tobytes(), key
    assert (got["reverse"]["its"] > 0).any()


def test_errors_raise_names_the_first_failing_problem_behind_the_finish(gpu_lib):
    rng = np.random.default_rng(37)
    x, y = _points(rng, 3, 8, 12)
    x[1, 0, 0] = np.inf
    for xs, ys in ((_dev(x), _dev(y)), (x, y)):
        with pytest.raises(ValueError, match=r"^problem 1: a cost \|x_i - y_j\|\^2 is not finite"):
            auction_solve_points_batch(xs, ys, fast=True, prices=rng.uniform(0, 50, (3, 12)), finish="reverse")
        res = auction_solve_points_batch(xs, ys, fast=True, prices=rng.uniform(0, 50, (3, 12)), finish="reverse", errors="status")
        assert df.host(res["reverse"]["its"]).tolist()[1] == -1 and (df.host(res["reverse"]["its"])[[0, 2]] >= 0).all()
