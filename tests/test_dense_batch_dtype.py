"""auction_solve_batch / hopcroft_solve_batch on float32, float16 and bfloat16 stacks (misslap_options.mat_dtype): the
stack is read in place in its own type, and the result is bit for bit the float64 result on the widened stack.

Expected values come from the oracle on the widened float64 slices (the reference's _from_matrix(...).solve()): sol,
its, nreductions, eCE, soln_found, n_assigned, obj, obj_f64, the fp32 eps bits, n_cols and the price bits.  The float64
draw is rounded to the type first, so the typed stack and the widened stack hold the same values."""
import functools

import numpy as np
import pytest

from sslap_amd import auction_solve_batch, hopcroft_solve_batch
from tests._batch_shapes import (bits as _bits, dense_compare as _check_problem, dense_expect as _oracle,
                                 dense_values as _values, host as _host)

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16", "bfloat16"]


def _typed(draw, dtype, device=False):
    """A float64 draw rounded to dtype: (the typed stack, the same values widened to float64).  float32 / float16 give a
    numpy stack (device=True: a device tensor); bfloat16 is always a device tensor, numpy has none."""
    import torch
    if dtype == "bfloat16":
        t = torch.from_numpy(np.ascontiguousarray(draw)).to(torch.bfloat16)
        return t.cuda(), t.double().numpy()  # (widened on the host: exact by construction, subnormals included)
    a = np.ascontiguousarray(draw.astype(dtype))
    return (torch.from_numpy(a).cuda() if device else a), a.astype(np.float64)


def _raw_bytes(stack):
    if isinstance(stack, np.ndarray):
        return stack.tobytes()
    import torch
    return stack.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _check_all(res, wide, problem, shapes=None, **kw):
    B, N, M = wide.shape
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        _check_problem(res, b, _oracle(wide[b, :n, :m], problem, **kw), n, m)


def _error_of(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


# ---- 1. value kinds (and 8: the caller's data is not written)

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("kind", ["uniform", "ints", "holes"])
def test_value_kinds(dtype, problem, kind):
    rng = np.random.default_rng([DTYPES.index(dtype), int(problem == "max"), ["uniform", "ints", "holes"].index(kind)])
    stack, wide = _typed(_values(kind, (6, 24, 31), rng), dtype)
    if kind == "uniform" and dtype != "float32":  # (ties are what this case is about: bfloat16 has 128 values a binade)
        assert np.unique(wide).size < (wide.size // 2 if dtype == "bfloat16" else wide.size)
    before = _raw_bytes(stack)
    res = auction_solve_batch(stack, problem=problem, cardinality_check=(kind == "holes"), mat_dtype=dtype)
    assert _raw_bytes(stack) == before
    _check_all(res, wide, problem)


@pytest.mark.parametrize("dtype", DTYPES)
def test_callers_stack_is_untouched_by_a_min_call(dtype):
    rng = np.random.default_rng(31)
    for device in (False, True):
        stack, wide = _typed(_values("holes", (3, 7, 9), rng), dtype, device=device)
        before = _raw_bytes(stack)
        res = auction_solve_batch(stack, problem="min", mat_dtype=dtype)
        assert _raw_bytes(stack) == before and str(stack.dtype).split(".")[-1] == dtype
        _check_all(res, wide, "min")


# ---- 2. lane and alignment boundaries

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 127, 129])
def test_lane_and_alignment_boundaries(dtype, M):
    """Odd M and odd N * M: the rows of a 2-byte stack that start on no 4-byte boundary."""
    rng = np.random.default_rng([DTYPES.index(dtype), M])
    N = min(M, 9)
    stack, wide = _typed(_values("uniform", (3, N, M), rng), dtype)
    for problem in ("min", "max"):
        res = auction_solve_batch(stack, problem=problem, cardinality_check=False, mat_dtype=dtype)
        _check_all(res, wide, problem)


@functools.lru_cache(maxsize=None)
def _cap_case():
    """One 1024 x 1024 problem of small integers (exact in every type) and what the reference makes of it."""
    draw = _values("ints", (1, 1024, 1024), np.random.default_rng(3))
    return draw, _oracle(draw[0], "max")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cap_shape_uses_every_staging_slot(dtype):
    draw, want = _cap_case()
    stack, wide = _typed(draw, dtype)
    assert np.array_equal(wide, draw)
    res = auction_solve_batch(stack, problem="max", cardinality_check=False, mat_dtype=dtype)
    _check_problem(res, 0, want, 1024, 1024)


# ---- 3. mixed shapes

@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_shapes_never_read_the_padding(dtype):
    rng = np.random.default_rng(5)
    B, N, M = 9, 30, 40
    shapes = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1)
    shapes[:, 1] = np.maximum(shapes[:, 1], shapes[:, 0])
    draw = np.full((B, N, M), np.inf)  # +inf would be rejected if it were read
    for b, (n, m) in enumerate(shapes):
        draw[b, :n, :m] = _values("holes" if b % 3 == 0 else "uniform", (n, m), rng)
    stack, wide = _typed(draw, dtype)
    for problem in ("min", "max"):
        res = auction_solve_batch(stack, problem=problem, shapes=shapes, mat_dtype=dtype)
        _check_all(res, wide, problem, shapes=shapes)


# ---- 4. both guards

def _guard_case(shape, rng):
    """(feasible draw with holes, the same with problems 1 and shape[0] - 2 made infeasible)."""
    good = _values("holes", shape, rng)
    bad = good.copy()
    bad[1, :3, 0] = 5.0
    bad[1, :3, 1:] = -1.0  # rows 0..2 only reach column 0
    bad[shape[0] - 2, :2, :] = np.nan
    bad[shape[0] - 2, :2, 2] = 7.0  # rows 0 and 1 share their only column
    return good, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(6, 8, 11), (64, 8, 11)], ids=["host_guard", "device_guard"])
def test_both_guards_read_the_typed_stack(dtype, shape):
    rng = np.random.default_rng([DTYPES.index(dtype), shape[0]])
    good, bad = _guard_case(shape, rng)
    for device in ((True,) if dtype == "bfloat16" else (False, True)):  # a typed host stack and a typed device stack
        stack, wide = _typed(bad, dtype, device=device)
        text = _error_of(lambda: auction_solve_batch(wide, problem="max"))
        assert text.startswith("problem 1: Matrix is infeasible (Maximum matching possible only involves")
        assert _error_of(lambda: auction_solve_batch(stack, problem="max", mat_dtype=dtype)) == text
        # the later one alone: the first failing problem is the one named
        later, wide_later = _typed(bad[2:], dtype, device=device)
        text = _error_of(lambda: auction_solve_batch(wide_later, problem="max"))
        assert text.startswith(f"problem {shape[0] - 4}: ")
        assert _error_of(lambda: auction_solve_batch(later, problem="max", mat_dtype=dtype)) == text
        stack, wide = _typed(good, dtype, device=device)
        res = auction_solve_batch(stack, problem="max", mat_dtype=dtype)
        assert res["meta"]["gpu"]["matching_ms"] > 0 or shape[0] < 64
        _check_all(res, wide, "max")


# ---- 5. status mode on a device stack

@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_status_mode_on_a_device_stack(dtype):
    """Every output bit for bit that of the status-mode call on the widened float64 device stack (existing code, pinned
    by tests/test_dense_batch_status.py)."""
    import torch
    rng = np.random.default_rng(41)
    B, N, M = 12, 10, 13
    draw = _values("holes", (B, N, M), rng)
    draw[1, 4, :] = np.nan  # an empty row
    draw[3] = -1.0
    draw[3, 0, :2] = (1.0, 2.0)  # too few values
    draw[5, 2, 2] = np.inf  # a +inf entry
    draw[7, :3, 0] = 5.0
    draw[7, :3, 1:] = -1.0  # an infeasible pattern: rows 0..2 only reach column 0
    prices = np.zeros((B, M))
    prices[2] = rng.uniform(0, 20, M)
    prices[9, 1] = -3.5  # a bad starting price
    prices[10, M - 1] = np.nan
    stack, wide = _typed(draw, dtype, device=True)
    wide_d = torch.from_numpy(wide).cuda()
    pd = torch.from_numpy(prices).cuda()
    for kw in (dict(problem="max"), dict(problem="max", fast=True), dict(problem="min")):
        got = auction_solve_batch(stack, prices=pd, errors="status", mat_dtype=dtype, **kw)
        want = auction_solve_batch(wide_d, prices=pd, errors="status", **kw)
        torch.cuda.synchronize()
        for k in ("sol", "prices", "status", "matching_size", "records"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), (k, kw)
        status = got["status"].cpu().numpy()
        assert [int(status[b]) for b in (1, 3, 5, 7, 9, 10)] == [2, 1, 3, 4, 6, 5]
        assert (np.delete(status, [1, 3, 5, 7, 9, 10]) == 0).all()
    # the solved ones of the last call ('min') are the reference's, too
    res = dict(got, meta={k: _host(v) for k, v in got["meta"].items()})
    for b in np.flatnonzero(status == 0):
        want_b = _oracle(wide[b], "min", p0=prices[b])
        assert np.array_equal(_host(res["sol"])[b], want_b["sol"])
        assert res["meta"]["its"][b] == want_b["meta"]["its"] and res["meta"]["obj_f64"][b] == want_b["extra"]["obj_f64"]
        assert np.array_equal(_bits(_host(res["prices"])[b, :want_b["M"]]), _bits(want_b["p"]))


# ---- 6. the matcher on a typed stack

@pytest.mark.parametrize("dtype", DTYPES)
def test_hopcroft_solve_batch_on_a_typed_stack(dtype):
    rng = np.random.default_rng(43)
    draw = rng.uniform(0, 100, (5, 17, 23))
    holes = rng.random(draw.shape) < 0.6
    draw[holes] = np.where(rng.random(draw.shape) < 0.5, -1.0, np.nan)[holes]
    draw[0, 0, 0], draw[0, 0, 1] = -0.0, np.inf  # both are entries
    for device in ((True,) if dtype == "bfloat16" else (False, True)):
        stack, wide = _typed(draw, dtype, device=device)
        got = hopcroft_solve_batch(mats=stack, mat_dtype=dtype)
        want = hopcroft_solve_batch(mats=wide)
        assert np.array_equal(got["size"], want["size"]) and (want["size"] > 0).all()
        for k in ("left_pairings", "right_pairings"):
            assert np.array_equal(_host(got[k]), want[k]), k
        assert np.array_equal(got["n_rows"], want["n_rows"]) and np.array_equal(got["n_cols"], want["n_cols"])


# ---- 7. the smallest magnitudes

def _smallest(dtype):
    """(smallest subnormal, smallest normal, largest finite or None) of the type, as float64."""
    if dtype == "float32":
        return 2.0 ** -149, 2.0 ** -126, None
    if dtype == "float16":
        return 2.0 ** -24, 2.0 ** -14, 65504.0
    return 2.0 ** -133, 2.0 ** -126, None  # bfloat16: 7 fraction bits below 2^-126


def _tiny_problem(dtype):
    """4 x 5.  Row 0 can only take the smallest subnormal, row 1 chooses between the smallest normal and -0.0, row 2
    between 0.0 and 1.0, row 3 between 0.0 and the largest finite value (float16).  Where the chosen values are the tiny
    ones, obj_f64 is their exact sum: a widening that flushed denormals changes it (checked on the reference itself)."""
    sub, nrm, top = _smallest(dtype)
    hole = -1.0
    return np.array([[sub, hole, hole, hole, hole],
                     [hole, nrm, -0.0, hole, hole],
                     [hole, hole, hole, 0.0, 1.0],
                     [hole, 0.0, top if top else hole, hole, hole]])


@pytest.mark.parametrize("dtype", DTYPES)
def test_smallest_magnitudes_are_not_flushed(dtype):
    draw = _tiny_problem(dtype)[None]
    stack, wide = _typed(draw, dtype)
    assert np.array_equal(_bits(wide), _bits(draw))  # every value is exact in the type, the sign of -0.0 included
    sub, nrm, _ = _smallest(dtype)
    flushed = np.where(np.abs(wide[0]) < nrm, 0.0, wide[0])
    notices = []  # whether the reference's own result changes when the denormals are flushed
    for problem in ("max", "min"):
        want = _oracle(wide[0], problem)
        assert want["meta"]["soln_found"] and want["meta"]["its"] < 1000
        notices.append(want["extra"]["obj_f64"] != _oracle(flushed, problem)["extra"]["obj_f64"])
        res = auction_solve_batch(stack, problem=problem, mat_dtype=dtype)
        _check_problem(res, 0, want, 4, 5)
    assert any(notices)
    # rows 0 and 1 alone, 'max': subnormal + normal, an exact float64 sum with no 1.0 to absorb it
    shapes = np.array([[2, 5]])
    want = _oracle(wide[0, :2], "max")
    assert want["extra"]["obj_f64"] == sub + nrm and want["meta"]["soln_found"]
    res = auction_solve_batch(stack, problem="max", shapes=shapes, mat_dtype=dtype)
    _check_problem(res, 0, want, 2, 5)
