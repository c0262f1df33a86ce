"""The inputs of tests/test_batch_launch_shapes.py without a GPU: the oracle alone on every input of tests/_batch_shapes.py,
and the properties the GPU comparisons rest on -- so that a changed seed cannot quietly turn a case into a trivial one.

  every problem is feasible and its full solve ends with everyone assigned;
  every `uniform` and `ints` problem goes through at least three eps reductions;
  every dense problem and every sparse problem without a repeated (i, j) entry ends with soln_found == 1 (the loop's
  eCE exit); at least one repeated-column problem of every sparse batch really repeats an entry, and at least one ends with
  soln_found == 0 (the loop's eps exit);
  the `ints` problems tie a row's best value across lanes and across the slots of one lane;
  the rows of the sparse problems have the stated lengths;
  a stopped solve leaves somebody unassigned at every stop below the full round count.
"""
import numpy as np
import pytest

from tests import _batch_shapes as bs


def _full(want, n):
    """A full solve: everyone assigned, to distinct objects."""
    assert want["meta"]["n_assigned"] == n == want["N"]
    assert (want["sol"] >= 0).all() and np.unique(want["sol"]).size == n


def _dense_properties(kind, mat, want, problem):
    n = mat.shape[0]
    _full(want, n)
    assert want["meta"]["soln_found"] == 1 and want["meta"]["eCE"] == 1
    if kind in ("uniform", "ints"):
        assert want["meta"]["nreductions"] >= 3, want["meta"]
    if kind == "ints":
        assert bs.tied_extreme(mat, problem)


def test_thread_table():
    assert [bs.threads_for(n) for n in (1, 256, 257, 512, 513, 1024, 2048)] == [256, 256, 512, 512, 1024, 1024, 1024]
    # every size is launched by the ladders, in both layouts
    assert {bs.threads_for(N) for N, _ in bs.LADDER_SHAPES} == {256, 512, 1024}
    assert {bs.threads_for(N) for N, _ in bs.STATUS_SHAPES} == {512, 1024}
    assert [bs.threads_for(n) for n in bs.SPARSE_ROWS] == [256, 512, 512, 1024]
    assert [bs.threads_for(N) for N, _ in bs.STOP_DENSE] == [bs.threads_for(n) for n in bs.STOP_SPARSE] == [256, 512, 1024]


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("shape", bs.LADDER_SHAPES, ids=bs.shape_id)
def test_dense_ladder_inputs(shape, problem):
    mats = bs.ladder_stack(shape)
    assert mats.shape == (3,) + shape
    for kind, mat, want in zip(bs.LADDER_KINDS, mats, bs.ladder_expect(shape, problem)):
        _dense_properties(kind, mat, want, problem)
    with np.errstate(invalid="ignore"):
        holes = ~(mats[2] >= 0)
    assert 0.25 < holes.mean() < 0.35 and np.isnan(mats[2]).any() and (mats[2] == -1).any()


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("shape", bs.STATUS_SHAPES, ids=bs.shape_id)
def test_dense_status_inputs(shape, problem):
    mats, prices = bs.status_stack(shape)
    wants = bs.status_expect(shape, problem)
    for b, kind in enumerate(bs.STATUS_KINDS):
        if b == bs.CONDEMNED:
            with np.errstate(invalid="ignore"):
                valid = mats[b] >= 0
            assert (~valid.any(axis=1)).sum() == 1 and wants[b] is None  # exactly one empty row
            continue
        _dense_properties(kind, mats[b], wants[b], problem)
    assert (prices[0] > 0).all() and (prices[bs.CONDEMNED] > 0).all() and not prices[[1, 3]].any()
    # the starting prices matter: without them problem 0 takes another course
    cold = bs.dense_expect(mats[0], problem)
    assert cold["meta"]["its"] != wants[0]["meta"]["its"] or not np.array_equal(cold["p"], wants[0]["p"])


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("dtype", bs.TYPED_DTYPES)
@pytest.mark.parametrize("shape", bs.TYPED_SHAPES, ids=bs.shape_id)
def test_typed_inputs(shape, dtype, problem):
    wide = bs.typed_stack(shape, dtype)
    assert np.array_equal(bs.round_to(wide, dtype), wide)  # every value is exact in the type
    assert np.unique(wide[0]).size < wide[0].size // 4  # rounded to 16 bits, `uniform` is full of equal values
    for kind, mat, want in zip(bs.TYPED_KINDS, wide, bs.typed_expect(shape, dtype, problem)):
        _dense_properties(kind, mat, want, problem)


@pytest.mark.parametrize("problem", bs.PROBLEMS)
def test_small_problems_in_a_large_stack(problem):
    mats = bs.small_stack()
    B, N, M = mats.shape
    assert (B, N, M) == bs.SMALL_STACK and bs.threads_for(N) == 1024
    assert bs.SMALL_SHAPES[:, 0].tolist() == [1, 2, 63, 64, 65, 256, 257, 512, 513, 600]
    assert (bs.SMALL_SHAPES[:, 1] >= bs.SMALL_SHAPES[:, 0]).all() and (bs.SMALL_SHAPES[:, 1] <= 64).any()
    assert (bs.SMALL_SHAPES[:, 0] <= N).all() and (bs.SMALL_SHAPES[:, 1] <= M).all()
    assert np.unique(bs.SMALL_SHAPES[:, 1]).size >= 8
    for b, ((n, m), kind, want) in enumerate(zip(bs.SMALL_SHAPES, bs.SMALL_KINDS, bs.small_expect(problem))):
        assert np.isposinf(mats[b, n:, :]).all() and np.isposinf(mats[b, :, m:]).all()
        if kind == "holes":
            _full(want, n)
            assert want["meta"]["soln_found"] == 1
        else:
            _dense_properties(kind, mats[b, :n, :m], want, problem)
    assert sorted(set(bs.SMALL_KINDS)) == ["holes", "ints", "uniform"]


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("n", bs.SPARSE_ROWS)
def test_sparse_ladder_inputs(n, problem):
    probs = bs.sparse_batch(n)
    wants = bs.sparse_expect_batch(n, problem)
    assert bs.SPARSE_K[n][2] in (128, 129)
    for b, ((loc, val), want, k) in enumerate(zip(probs, wants, bs.SPARSE_K[n])):
        assert (bs.row_lengths(loc) == k).all() and bs.row_lengths(loc).size == n
        assert int(loc[:, 1].max()) < (n + 43 if b == 3 else n)
        _full(want, n)
        assert want["meta"]["nreductions"] >= 3, (b, want["meta"])
        if b in bs.SPARSE_DISTINCT:
            assert not bs.has_repeated_entry(loc)
            assert want["meta"]["soln_found"] == 1, b
    assert np.array_equal(np.diff(probs[0][0][:63, 1]) > 0, np.ones(62, dtype=bool))  # stored in column order
    assert (np.diff(probs[1][0][:65, 1]) < 0).any()  # shuffled stored order
    assert bs.has_repeated_entry(probs[2][0]) and wants[2]["meta"]["soln_found"] == 0  # the loop's other exit
    assert int(probs[3][0][:, 1].max()) >= n  # rectangular in fact


@pytest.mark.parametrize("problem", bs.PROBLEMS)
def test_sparse_small_batch_inputs(problem):
    probs = bs.sparse_small_batch()
    rows = [int(lo[:, 0].max()) + 1 for lo, _ in probs]
    assert min(rows) == 5 and max(rows) == 40
    for dims in bs.SPARSE_BIG_DIMS:
        assert max(rows) * 10 < dims[0] and all(int(lo[:, 1].max()) < dims[1] for lo, _ in probs)
    assert [bs.threads_for(d[0]) for d in bs.SPARSE_BIG_DIMS] == [512, 1024]
    for (loc, val), want, n in zip(probs, bs.sparse_small_expect(problem), rows):
        _full(want, n)
        assert want["meta"]["nreductions"] >= 3, (n, want["meta"])
    assert any((val == np.floor(val)).all() for _, val in probs)  # (an `ints` problem is among them)


def _stops_leave_somebody_unassigned(n, full, stopped):
    its = full["meta"]["its"]
    assert its > 40  # the seven stops are distinct rounds of the solve, in ascending order
    assert [r for r, _ in stopped] == bs.stops(its) and bs.stops(its) == sorted(bs.stops(its))
    for r, want in stopped:
        assert want["meta"]["its"] == max(r, 1)  # (the loop body runs before the first test)
        assert want["meta"]["n_assigned"] < n and (want["sol"] == -1).sum() == n - want["meta"]["n_assigned"], r
    return [n - want["meta"]["n_assigned"] for _, want in stopped]


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("shape", bs.STOP_DENSE, ids=bs.shape_id)
def test_stopped_dense_inputs(shape, problem):
    full, stopped = bs.stop_dense_expect(shape, problem)
    _dense_properties("uniform", bs.stop_dense_input(shape), full, problem)
    left = _stops_leave_somebody_unassigned(shape[0], full, stopped)
    assert left[0] == left[1] > 64  # max_iter = 0 is one round; several 64-chunks of the list are still unassigned


@pytest.mark.parametrize("problem", bs.PROBLEMS)
@pytest.mark.parametrize("n", bs.STOP_SPARSE)
def test_stopped_sparse_inputs(n, problem):
    loc, val = bs.stop_sparse_input(n)
    assert (bs.row_lengths(loc) == 65).all() and not bs.has_repeated_entry(loc)
    full, stopped = bs.stop_sparse_expect(n, problem)
    _full(full, n)
    assert full["meta"]["soln_found"] == 1 and full["meta"]["nreductions"] >= 3
    left = _stops_leave_somebody_unassigned(n, full, stopped)
    assert left[0] == left[1] > 64
