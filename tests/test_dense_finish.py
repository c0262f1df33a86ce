"""auction_solve_batch(finish="reverse") on the GPU (misslap_dense_batch_reverse_finish, k_dense_reverse_finish in
csrc/kernels_dense_batch.hpp).

The yardstick is always sslap_amd.dense_reverse_finish, the numpy model, applied to the outputs of the SAME call with
finish=None (the forward solve is pinned to the oracle elsewhere); everything is compared bit for bit
(tests/_dense_finish.py: assert_is_the_model): sol, prices, outside_prices, reverse.its, reverse.left, meta.obj_f64 /
obj_f32 / eCE, and every other meta field, status and matching_size unchanged.
"""
import time

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, batch_meta_to_host
from tests import _dense_finish as df

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _stack(rng, B, n, m, gate=0.3, lo=0.0, hi=100.0, integer=False, hole=-1.0):
    """(B, n, m) values on [lo, hi) with a share `gate` of holes; a random injection per problem stays free of them."""
    v = rng.integers(int(lo), int(hi), (B, n, m)).astype(np.float64) if integer else rng.uniform(lo, hi, (B, n, m))
    gated = rng.random((B, n, m)) < gate
    for b in range(B):
        gated[b, np.arange(n), rng.permutation(m)[:n]] = False
    return np.where(gated, hole, v)


def _check(stack, trace=None, **kw):
    """Both calls on the device stack, the model on the first one's outputs, the comparison.  Returns (forward result,
    finished result, model)."""
    r0 = auction_solve_batch(stack, errors="status", **kw)
    r1 = auction_solve_batch(stack, errors="status", finish="reverse", **kw)
    want = df.model_of(stack, r0, trace=trace, **kw)
    df.assert_is_the_model(r1, r0, want)
    return r0, r1, want


@pytest.mark.parametrize("n,m", [(1, 1), (1, 2), (2, 2)])
def test_the_smallest_shapes_have_nothing_to_do(gpu_lib, n, m):
    rng = np.random.default_rng(n * 10 + m)
    _, r1, want = _check(_dev(_stack(rng, 3, n, m, gate=0.0)), fast=True)
    assert (want["reverse"]["its"] == 0).all() and (want["reverse"]["left"] == 0).all()
    assert df.host(r1["reverse"]["its"]).tolist() == [0, 0, 0]


@pytest.mark.parametrize("outside", [None, 60.0])
@pytest.mark.parametrize("n,m", [(63, 64), (64, 65), (65, 130)])
def test_the_wavefront_edges_of_the_row_scan(gpu_lib, n, m, outside):
    rng = np.random.default_rng(n + m)
    kw = dict(fast=True, prices=rng.uniform(0, 100, (3, m)))
    if outside is not None:
        kw["outside"] = outside
    _, _, want = _check(_dev(_stack(rng, 3, n, m)), **kw)
    assert want["ran"].all() and (want["reverse"]["its"] > 0).all()


def test_the_full_carve(gpu_lib):
    """1024 x 1024 with outside at B = 2: 2048 objects and 1024 rows in LDS, 16 rows per lane in the column scan."""
    rng = np.random.default_rng(1024)
    mats = _stack(rng, 2, 1024, 1024, gate=0.5)
    _, _, want = _check(_dev(mats), fast=True, outside=rng.uniform(40, 60, (2, 1024)), prices=rng.uniform(0, 40, (2, 1024)))
    print("full carve: its", want["reverse"]["its"].tolist())
    assert want["ran"].all() and (want["reverse"]["its"] > 0).all() and (want["reverse"]["left"] == 0).all()


@pytest.mark.parametrize("name", list(df.situations()))
def test_the_hand_built_situations(gpu_lib, name):
    case = df.situations()[name]
    trace = []
    r0, _, want = _check(_dev(case["mats"]), trace=trace, **case["kw"])
    assert df.situation_holds(case, r0, want, trace), trace[:8]


@pytest.mark.parametrize("name", ["float64", "float32", "float16", "bfloat16"])
def test_every_element_type(gpu_lib, name):
    import torch
    rng = np.random.default_rng(len(name))
    mats = _stack(rng, 3, 20, 33, integer=True, hi=200.0)  # (integers below 256: exact in every type)
    stack = _dev(mats).to(getattr(torch, name))
    for problem in ("min", "max"):
        _, _, want = _check(stack, mat_dtype=name, problem=problem, fast=True, prices=rng.uniform(0, 300, (3, 33)))
        assert (want["reverse"]["its"] > 0).all()


@pytest.mark.parametrize("view", ["transposed", "column_slice", "expanded"])
def test_strided_views(gpu_lib, view):
    rng = np.random.default_rng(5)
    B, n, m = 3, 24, 40
    if view == "transposed":
        stack = _dev(_stack(rng, B, n, m).transpose(0, 2, 1).copy()).transpose(1, 2)
    elif view == "column_slice":
        buf = _dev(rng.uniform(0, 100, (B, n + 5, m + 9)))
        stack = buf[:, 2:2 + n, 4:4 + m]
    else:
        stack = _dev(_stack(rng, 1, n, m))[0].expand(B, n, m)
    assert not stack.is_contiguous()
    for kw in (dict(), dict(outside=rng.uniform(30, 70, (B, n)))):
        _, _, want = _check(stack, fast=True, prices=rng.uniform(0, 150, (B, m)), **kw)
        assert (want["reverse"]["its"] > 0).all()


@pytest.mark.parametrize("problem", ["min", "max"])
def test_signed_values_and_a_negative_outside(gpu_lib, problem):
    rng = np.random.default_rng(9)
    mats = _stack(rng, 4, 17, 29, lo=-50.0, hi=50.0, hole=np.nan)
    _, _, want = _check(_dev(mats), entries="finite", problem=problem, fast=True, prices=rng.uniform(0, 90, (4, 29)))
    assert (want["reverse"]["its"] > 0).all()
    _, _, want = _check(_dev(mats), entries="finite", problem=problem, outside=-5.0, prices=rng.uniform(0, 90, (4, 29)))
    assert (want["reverse"]["its"] > 0).all()
    _, _, want = _check(_dev(mats), entries="finite", problem=problem, outside=-5.0, fast=False)  # the reference's eps-scaling
    assert want["ran"].all()


@pytest.mark.parametrize("outside", [None, 45.0])
def test_mixed_shapes_in_one_batch(gpu_lib, outside):
    rng = np.random.default_rng(13)
    shapes = np.array([[30, 37], [1, 37], [12, 12], [7, 20], [30, 31]], dtype=np.int32)
    mats = _stack(rng, 5, 30, 37, gate=0.0)
    kw = dict(shapes=shapes, fast=True, prices=rng.uniform(0, 120, (5, 37)))
    if outside is not None:
        kw["outside"] = outside
    _, r1, want = _check(_dev(mats), **kw)
    assert want["ran"].all()
    if outside is None:
        assert want["reverse"]["its"][2] == 0  # the square problem
    _check(_dev(mats), **dict(kw, shapes=_dev(shapes)))  # ... and from a device shapes tensor


def test_a_condemned_problem_between_solved_ones_is_untouched(gpu_lib):
    rng = np.random.default_rng(17)
    mats = _stack(rng, 4, 10, 16, gate=0.0)
    mats[1, 3, 5] = np.inf
    shapes = _dev(np.array([[10, 16], [10, 16], [0, 99999], [10, 16]], dtype=np.int32))  # problem 2: a bad device shape
    for kw in (dict(), dict(outside=50.0)):
        r0, r1, want = _check(_dev(mats), shapes=shapes, fast=True, prices=rng.uniform(0, 150, (4, 16)), **kw)
        assert df.host(r1["status"]).tolist() == [0, _lib.BATCH_STATUS_INFINITE_VALUE, _lib.BATCH_STATUS_BAD_SHAPE, 0]
        assert df.host(r1["reverse"]["its"])[[1, 2]].tolist() == [-1, -1] and df.host(r1["reverse"]["left"])[[1, 2]].tolist() == [-1, -1]
        assert (df.host(r1["reverse"]["its"])[[0, 3]] > 0).all()


def test_a_forward_solve_cut_by_max_iter_is_untouched(gpu_lib):
    rng = np.random.default_rng(19)
    mats = _stack(rng, 3, 30, 45, gate=0.0)
    mats[1, 1:, :] = -1.0  # (problem 1 is one row by its shape: solved in one round)
    shapes = np.array([[30, 45], [1, 45], [30, 45]], dtype=np.int32)
    r0, r1, want = _check(_dev(mats), shapes=shapes, max_iter=1, prices=rng.uniform(0, 150, (3, 45)), fast=True)
    assert (df.host(r1["status"]) == 0).all()
    assert want["ran"].tolist() == [False, True, False]
    assert df.host(r1["reverse"]["its"])[[0, 2]].tolist() == [-1, -1]


def test_the_budget_cuts_the_finish_like_the_model(gpu_lib):
    """Few rows and many objects from high prices: the forward solve takes a few rounds, the finish one iteration per
    abandoned object.  max_iter between the two cuts the finish only."""
    rng = np.random.default_rng(23)
    mats = _stack(rng, 3, 6, 150, gate=0.0)
    stack, prices = _dev(mats), rng.uniform(100, 400, (3, 150))
    r0, _, full = _check(stack, fast=True, prices=prices)
    forward = int(batch_meta_to_host(r0)["its"].max())
    assert (full["reverse"]["its"] > forward + 5).all(), (forward, full["reverse"]["its"])
    _, r1, cut = _check(stack, fast=True, prices=prices, max_iter=forward + 5)
    assert cut["ran"].all() and (cut["reverse"]["its"] == forward + 5).all() and (cut["reverse"]["left"] > 0).all()
    assert np.array_equal(df.host(r1["reverse"]["left"]), cut["reverse"]["left"])


def test_a_device_stack_gets_device_outputs_and_the_call_waits_for_nothing(gpu_lib):
    import torch
    rng = np.random.default_rng(29)
    host = _stack(rng, 64, 48, 60)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src, pd = _dev(host), _dev(rng.uniform(0, 100, (64, 60)))
        w = torch.randn(4096, 4096, device="cuda")
        x = torch.full_like(src, -1.0)
        x.copy_(src)
        auction_solve_batch(x, prices=pd, fast=True, errors="status", finish="reverse")  # the warm-up call
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(8):
            w = w @ w
            w = w / w.norm()
        e[1].record()
        torch.cuda.synchronize()
        reps = int(np.ceil(8 * 400.0 / e[0].elapsed_time(e[1])))  # a queue of about 400 ms
        x.fill_(-1.0)  # read before the copy below lands, no problem would have an entry
        torch.cuda.synchronize()
        for _ in range(reps):
            w = w @ w
            w = w / w.norm()
        x.copy_(src, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_batch(x, prices=pd, fast=True, errors="status", finish="reverse")
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert pending and t_call < 100.0
    for key in ("sol", "prices", "status", "matching_size"):
        assert res[key].is_cuda, key
    assert res["reverse"]["its"].is_cuda and res["reverse"]["left"].is_cuda
    assert all(v.is_cuda for v in res["meta"].values())
    with torch.cuda.stream(stream):
        r0 = auction_solve_batch(src, prices=pd, fast=True, errors="status")
        df.assert_is_the_model(res, r0, df.model_of(src, r0))
    assert (df.host(res["status"]) == 0).all() and (df.host(res["reverse"]["its"]) > 0).any()


@pytest.mark.parametrize("outside", [None, 55.0])
def test_a_numpy_stack_takes_the_device_route_and_returns_numpy(gpu_lib, outside):
    rng = np.random.default_rng(31)
    mats, prices = _stack(rng, 3, 12, 20), rng.uniform(0, 100, (3, 20))
    kw = dict(fast=True, prices=prices) if outside is None else dict(fast=True, prices=prices, outside=outside)
    dev = auction_solve_batch(_dev(mats), errors="status", finish="reverse", **kw)
    for errors in ("status", "raise"):
        got = auction_solve_batch(mats, errors=errors, finish="reverse", **kw)
        assert not {"records", "info", "stream", "keep"} & set(got)
        for key in ("sol", "prices", "status", "matching_size") + (() if outside is None else ("outside_prices",)):
            assert isinstance(got[key], np.ndarray) and got[key].tobytes() == df.host(dev[key]).tobytes(), key
        for key in ("its", "left"):
            assert isinstance(got["reverse"][key], np.ndarray) and np.array_equal(got["reverse"][key], df.host(dev["reverse"][key]))
        want_meta = batch_meta_to_host(dev)
        for key in set(want_meta) - {"timer", "gpu"}:
            assert got["meta"][key].tobytes() == want_meta[key].tobytes(), key


def test_errors_raise_names_the_first_failing_problem_behind_the_finish(gpu_lib):
    rng = np.random.default_rng(37)
    mats = _stack(rng, 3, 8, 12, gate=0.0)
    mats[1, 0, 0] = np.inf
    with pytest.raises(ValueError, match=r"^problem 1: val holds a NaN or an infinity"):
        auction_solve_batch(_dev(mats), fast=True, finish="reverse")
    with pytest.raises(ValueError, match=r"^problem 1: val holds a NaN or an infinity"):
        auction_solve_batch(mats, fast=True, finish="reverse")
