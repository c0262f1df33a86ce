"""The one-workgroup-per-problem solves at every workgroup size and lane edge of their shared round loop (batch_solve,
csrc/kernels_batch_solve.hpp), against the oracle on the same float64 slice or loc / val, `==` on every bit: sol with its
-1 tail, its, nreductions, eCE, soln_found, n_assigned, obj, obj_f64, the fp32 bits of the start and final eps, n_rows,
n_cols (and nnz for the sparse entry), the price bits up to M and the rest of the price row.

The inputs and the expectations are those of tests/_batch_shapes.py (pinned without a GPU by
tests/test_batch_launch_shapes_nogpu.py).  Every case also asserts the launch it was written for: 256 threads up to 256
rows, 512 up to 512, 1024 above (batch_solve_threads, csrc/abi_batch_common.hpp) -- by the stack's N in the dense entry,
by the largest problem in the sparse entry, by `dims` in the sparse status mode.

  1  dense ladder       auction_solve_batch on a host float64 stack: the workgroup-size steps and the staging-slot edges
  2  status, typed      the same launches through k_dense_batch_solve_status (a condemned workgroup beside live ones) and
                        through the float16 / bfloat16 row source
  3  small in large     1024 threads around problems of 1 .. 600 rows, default mode and status mode
  4  sparse ladder      auction_solve_sparse_batch at 256 / 257 / 512 / 513 rows, default mode and status mode; status mode
                        with a carve far larger than its problems
  5  stopped solves     max_iter in {0, 1, 2, 3, 10, its // 2, its - 1} at each workgroup size: the state after round r
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import auction_solve_batch, auction_solve_sparse_batch
from tests import _batch_shapes as bs
from tests.test_dense_batch_status import _to_host as _dense_to_host
from tests.test_sparse_batch_status import _device, _to_host as _sparse_to_host

pytestmark = pytest.mark.gpu

ZERO_META = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "obj_f64", "start_eps", "final_eps",
             "start_eps_f32", "final_eps_f32", "bids_made")


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _on_device(a):
    import torch
    return torch.tensor(a, device="cuda")


def _threads(res):
    return res["meta"]["gpu"]["threads"]  # (status mode: the host form of the result carries the launch as well)


# ---- 1. the dense ladder

@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("shape", bs.LADDER_SHAPES, ids=bs.shape_id)
def test_dense_ladder(shape, problem):
    N, M = shape
    mats = bs.ladder_stack(shape)
    res = auction_solve_batch(mats, problem=problem, cardinality_check=True)  # (B < 64: the guard runs on the host)
    assert _threads(res) == bs.threads_for(N)
    assert res["sol"].shape == (3, N) and res["prices"].shape == (3, M)
    for b, want in enumerate(bs.ladder_expect(shape, problem)):
        bs.dense_compare(res, b, want, N, M)


# ---- 2. the same launches through the other two dense kernels

@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("shape", bs.STATUS_SHAPES, ids=bs.shape_id)
def test_dense_status_on_a_device_stack(shape, problem):
    N, M = shape
    mats, prices = bs.status_stack(shape)
    got = auction_solve_batch(_on_device(mats), problem=problem, prices=_on_device(prices), errors="status")
    assert got["sol"].is_cuda and got["prices"].is_cuda and got["status"].is_cuda
    res = _dense_to_host(got)
    assert _threads(res) == bs.threads_for(N)
    want_status = np.zeros(len(mats), dtype=np.int32)
    want_status[bs.CONDEMNED] = bs.EMPTY_ROW_STATUS
    assert res["status"].dtype == np.int32 and np.array_equal(res["status"], want_status)
    for b, want in enumerate(bs.status_expect(shape, problem)):
        if b != bs.CONDEMNED:
            assert res["matching_size"][b] == N
            bs.dense_compare(res, b, want, N, M, p0=prices[b])
            continue
        # the condemned workgroup left the launch with the defined outputs: its starting prices are not copied through,
        # and the guard matched every row but the empty one
        assert prices[b].all() and res["matching_size"][b] == N - 1
        assert (res["sol"][b] == -1).all() and np.array_equal(bs.bits(res["prices"][b]), bs.bits(np.zeros(M))), b
        meta = res["meta"]
        assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (N, M, (N - 1) * M)
        for k in ZERO_META:
            assert meta[k][b] == 0, k


def _typed(wide, dtype):
    """The typed stack of a widened one (its values are exact in the type): float16 on the host, bfloat16 on the device."""
    if dtype == "bfloat16":
        import torch
        return _on_device(wide).to(torch.bfloat16)
    return np.ascontiguousarray(wide.astype(dtype))


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("dtype", bs.TYPED_DTYPES)
@pytest.mark.parametrize("shape", bs.TYPED_SHAPES, ids=bs.shape_id)
def test_typed_stacks(shape, dtype, problem):
    N, M = shape
    wide = bs.typed_stack(shape, dtype)
    stack = _typed(wide, dtype)
    assert str(stack.dtype).split(".")[-1] == dtype
    res = auction_solve_batch(stack, problem=problem, mat_dtype=dtype)
    assert _threads(res) == bs.threads_for(N)
    for b, want in enumerate(bs.typed_expect(shape, dtype, problem)):
        bs.dense_compare(res, b, want, N, M)


# ---- 3. a 1024-thread launch around small problems

def _compare_small(res, problem):
    assert _threads(res) == 1024  # by the stack's N = 600, whatever the problems' own row counts
    for b, ((n, m), want) in enumerate(zip(bs.SMALL_SHAPES, bs.small_expect(problem))):
        bs.dense_compare(res, b, want, int(n), int(m))


@pytest.mark.parametrize("problem", bs.PROBLEMS)
def test_small_problems_in_a_large_stack(problem):
    res = auction_solve_batch(bs.small_stack(), problem=problem, shapes=bs.SMALL_SHAPES)
    _compare_small(res, problem)


@pytest.mark.parametrize("problem", bs.PROBLEMS)
def test_small_problems_in_a_large_stack_status(problem):
    res = _dense_to_host(auction_solve_batch(_on_device(bs.small_stack()), problem=problem, shapes=bs.SMALL_SHAPES,
                                             errors="status"))
    assert (res["status"] == 0).all() and np.array_equal(res["matching_size"], bs.SMALL_SHAPES[:, 0])
    _compare_small(res, problem)


# ---- 4. the sparse ladder

def _compare_sparse(res, wants):
    for b, want in enumerate(wants):
        bs.sparse_compare(res, b, want)


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("n", bs.SPARSE_ROWS)
def test_sparse_ladder(n, problem):
    loc, val, offsets = bs.sparse_pack(bs.sparse_batch(n))
    res = auction_solve_sparse_batch(loc, val, offsets, problem=problem)
    assert _threads(res) == bs.threads_for(n)
    assert res["sol"].shape == (4, n) and res["prices"].shape == (4, int(loc[:, 1].max()) + 1)
    _compare_sparse(res, bs.sparse_expect_batch(n, problem))


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("n", bs.SPARSE_ROWS)
def test_sparse_ladder_status_on_the_device(n, problem):
    loc, val, offsets = bs.sparse_pack(bs.sparse_batch(n))
    dims = (n, int(loc[:, 1].max()) + 1)  # the batch's own maxima
    dl, dv = _device(loc, val)
    res = _sparse_to_host(auction_solve_sparse_batch(dl, dv, offsets, problem=problem, errors="status", dims=dims))
    assert _threads(res) == bs.threads_for(n)
    assert (res["status"] == 0).all() and (res["matching_size"] == n).all()
    assert res["sol"].shape == (4, dims[0]) and res["prices"].shape == (4, dims[1])
    _compare_sparse(res, bs.sparse_expect_batch(n, problem))


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("dims", bs.SPARSE_BIG_DIMS, ids=bs.shape_id)
def test_sparse_status_large_carve_small_problems(dims, problem):
    probs = bs.sparse_small_batch()
    loc, val, offsets = bs.sparse_pack(probs)
    dl, dv = _device(loc, val)
    res = _sparse_to_host(auction_solve_sparse_batch(dl, dv, offsets, problem=problem, errors="status", dims=dims))
    assert _threads(res) == bs.threads_for(dims[0])  # 512 / 1024 threads on problems of 5 .. 40 rows
    assert (res["status"] == 0).all()
    assert res["sol"].shape == (len(probs), dims[0]) and res["prices"].shape == (len(probs), dims[1])
    _compare_sparse(res, bs.sparse_small_expect(problem))


# ---- 5. stopped solves at each workgroup size

@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("stop", range(7), ids=bs.STOP_NAMES)
@pytest.mark.parametrize("shape", bs.STOP_DENSE, ids=bs.shape_id)
def test_stopped_dense(shape, stop, problem):
    N, M = shape
    max_iter, want = bs.stop_dense_expect(shape, problem)[1][stop]
    res = auction_solve_batch(bs.stop_dense_input(shape)[None], problem=problem, max_iter=max_iter)
    assert _threads(res) == bs.threads_for(N)
    bs.dense_compare(res, 0, want, N, M)
    assert (res["sol"][0] == -1).sum() == N - want["meta"]["n_assigned"] > 0


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("stop", range(7), ids=bs.STOP_NAMES)
@pytest.mark.parametrize("n", bs.STOP_SPARSE)
def test_stopped_sparse(n, stop, problem):
    loc, val = bs.stop_sparse_input(n)
    max_iter, want = bs.stop_sparse_expect(n, problem)[1][stop]
    res = auction_solve_sparse_batch(loc, val, np.array([0, len(val)]), problem=problem, max_iter=max_iter)
    assert _threads(res) == bs.threads_for(n)
    bs.sparse_compare(res, 0, want)
    assert (res["sol"][0] == -1).sum() == n - want["meta"]["n_assigned"] > 0
