"""The batch solves' feasibility guard (cardinality_check=True) on the device: the Hopcroft-Karp kernel of
hopcroft_solve_batch runs behind the check pass.  Infeasible problems mixed with malformed and over-cap ones, host and
device input: the text raised is what from_matrix / from_sparse raises for the first failing slice.  Feasible batches
give bit-identical results with and without the guard.  The batches are large enough for the device guard (dense
B >= 64, sparse B >= 256: smaller ones keep the host guard)."""
import numpy as np
import pytest

from sslap_amd import auction_solve_batch, auction_solve_sparse_batch, from_matrix, from_sparse

pytestmark = pytest.mark.gpu

SPARSE_B = 300


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _first_error(make, items):
    """(index, text) of the first item whose single-problem constructor raises."""
    for b, it in enumerate(items):
        try:
            make(it)
        except ValueError as e:
            return b, str(e)
    return None, None


def _same_result(a, b):
    for k in ("sol", "prices"):
        x, y = a[k], b[k]
        x = x.cpu().numpy() if hasattr(x, "cpu") else x
        y = y.cpu().numpy() if hasattr(y, "cpu") else y
        if k == "prices":
            x, y = _bits(x), _bits(y)
        assert np.array_equal(x, y), k
    for k in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj_f64", "final_eps_f32"):
        assert np.array_equal(a["meta"][k], b["meta"][k]), k


# ---- dense
def _narrow(rng, n, m, reach):
    """n x m whose rows but the last reach only the first `reach` columns: a maximum matching of reach + 1 rows"""
    mat = rng.uniform(0, 10, (n, m))
    mat[: n - 1, reach:] = -1.0  # all rows but the last reach only `reach` columns
    return mat


def _to_device(x):
    import torch
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("device", [False, True])
def test_dense_infeasible_and_malformed_first_text_wins(device):
    if device:
        pytest.importorskip("torch")
    rng = np.random.default_rng(1)
    B, N = 80, 24
    good = rng.uniform(0, 10, (B, N, N))
    layouts = []
    m = good.copy()
    m[5] = _narrow(rng, N, N, 6)  # infeasible: 7 out of 24
    layouts.append((m, 5))
    m = good.copy()
    m[3] = _narrow(rng, N, N, 6)
    m[7, 4, :] = np.nan  # an empty row comes after the infeasible problem
    layouts.append((m, 3))
    m = good.copy()
    m[8] = _narrow(rng, N, N, 20)
    m[2, 1, 3] = np.inf  # +inf ahead of the infeasible problem: its own text first
    layouts.append((m, 2))
    for mats, b in layouts:
        want_b, want = _first_error(lambda x: from_matrix(x.copy()), list(mats))
        assert want_b == b
        src = _to_device(mats) if device else mats
        with pytest.raises(ValueError) as e:
            auction_solve_batch(src, cardinality_check=True)
        assert str(e.value) == f"problem {b}: {want}"


def test_dense_infeasible_with_shapes_and_many_problems():
    rng = np.random.default_rng(2)
    B, N, M = 300, 40, 50
    mats = rng.uniform(0, 10, (B, N, M))
    shapes = np.stack([rng.integers(5, N + 1, B), rng.integers(N, M + 1, B)], axis=1)
    b0 = 217
    n0, m0 = shapes[b0]
    mats[b0, : n0 - 1, 3:] = -1.0  # rows reach 3 columns: 4 out of n0
    want_b, want = _first_error(lambda i: from_matrix(mats[i, : shapes[i, 0], : shapes[i, 1]].copy()), range(B))
    assert want_b == b0 and "Maximum matching" in want
    with pytest.raises(ValueError) as e:
        auction_solve_batch(mats, shapes=shapes, cardinality_check=True)
    assert str(e.value) == f"problem {b0}: {want}"


@pytest.mark.parametrize("device", [False, True])
def test_dense_feasible_guard_changes_nothing(device):
    if device:
        pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    mats = rng.uniform(0, 100, (64, 48, 60))
    mats[rng.random(mats.shape) < 0.3] = -1.0
    mats[:, np.arange(48), np.arange(48)] = 1.0  # a perfect matching of the rows
    src = _to_device(mats) if device else mats
    a = auction_solve_batch(src, cardinality_check=True)
    b = auction_solve_batch(src, cardinality_check=False)
    _same_result(a, b)
    assert a["meta"]["gpu"]["matching_ms"] >= 0


# ---- sparse
def _problem(rng, n, m, per_row):
    cols = rng.integers(0, m, (n, per_row)).astype(np.int32)
    cols[:, 0] = rng.permutation(m)[:n]
    cols = rng.permuted(cols, axis=1)
    loc = np.ascontiguousarray(np.stack([np.repeat(np.arange(n, dtype=np.int32), per_row), cols.ravel()], axis=1))
    return loc, rng.uniform(0, 100, loc.shape[0])


def _narrow_sparse(rng, n, m, reach):
    loc, val = _problem(rng, n, m, 3)
    loc[loc[:, 0] < n - 1, 1] %= reach
    return loc, val


def _pack(probs):
    loc = np.ascontiguousarray(np.concatenate([p[0] for p in probs]), dtype=np.int32)
    val = np.ascontiguousarray(np.concatenate([p[1] for p in probs]))
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in probs])]).astype(np.int64)
    return loc, val, offsets


def _sparse_error(probs, device):
    want_b, want = _first_error(lambda p: from_sparse(p[0].copy(), p[1].copy(), cardinality_check=True), probs)
    loc, val, offsets = _pack(probs)
    before = loc.copy()
    if device:
        loc_d, val_d = _to_device(loc), _to_device(val)
        with pytest.raises(ValueError) as e:
            auction_solve_sparse_batch(loc_d, val_d, offsets, cardinality_check=True)
        assert np.array_equal(loc_d.cpu().numpy(), before)
    else:
        with pytest.raises(ValueError) as e:
            auction_solve_sparse_batch(loc, val, offsets, cardinality_check=True)
        assert np.array_equal(loc, before)
    assert want_b is not None
    assert str(e.value) == f"problem {want_b}: {want}"
    return want_b, want


def _malformed(rng, kind):
    loc, val = _problem(rng, 10, 12, 3)
    if kind == "negative":
        loc[7, 1] = -3
    elif kind == "unsorted":
        loc[[4, 20]] = loc[[20, 4]]
    elif kind == "gap":
        loc = loc[loc[:, 0] != 4].copy()
        val = val[: loc.shape[0]].copy()
    elif kind == "over_cap":
        loc[-1] = (9, 2100)
    elif kind == "over_cap_rows":
        loc = np.concatenate([loc, [[2200, 1]]]).astype(np.int32)
        val = np.concatenate([val, [1.0]])
    return loc, val


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("kind", ["negative", "unsorted", "gap", "over_cap_rows"])
def test_sparse_malformed_and_infeasible_first_text_wins(device, kind):
    if device:
        pytest.importorskip("torch")
    rng = np.random.default_rng(4)
    probs = [_problem(rng, 20, 25, 4) for _ in range(SPARSE_B)]
    # the malformed problem first, then an infeasible clean one; and the other way round
    probs[3] = _malformed(rng, kind)
    probs[6] = _narrow_sparse(rng, 20, 25, 5)
    b, _ = _sparse_error(probs, device)
    assert b == 3
    probs[1] = _narrow_sparse(rng, 20, 25, 4)
    b, text = _sparse_error(probs, device)
    assert b == 1 and "Maximum matching" in text


@pytest.mark.parametrize("device", [False, True])
def test_sparse_feasible_over_the_cap_is_reported_by_the_cap_check(device):
    """a column beyond the cap: the host guard passes (from_sparse itself has no cap), then the cap's text"""
    if device:
        pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    probs = [_problem(rng, 8, 10, 3) for _ in range(SPARSE_B)]
    probs[3] = _narrow_sparse(rng, 20, 25, 5)
    probs[2] = _malformed(rng, "over_cap")
    from_sparse(probs[2][0].copy(), probs[2][1].copy(), cardinality_check=True)  # feasible on its own
    loc, val, offsets = _pack(probs)
    src = (_to_device(loc), _to_device(val)) if device else (loc, val)
    with pytest.raises(ValueError) as e:
        auction_solve_sparse_batch(*src, offsets, cardinality_check=True)
    assert str(e.value).startswith("problem 2: 10 x 2101 exceeds MISSLAP_SPARSE_BATCH_MAX_DIM (2048)")


@pytest.mark.parametrize("device", [False, True])
def test_sparse_feasible_guard_changes_nothing(device):
    if device:
        pytest.importorskip("torch")
    rng = np.random.default_rng(6)
    probs = [_problem(rng, int(rng.integers(20, 256)), 256, 8) for _ in range(SPARSE_B)]
    loc, val, offsets = _pack(probs)
    src = (_to_device(loc), _to_device(val)) if device else (loc, val)
    a = auction_solve_sparse_batch(*src, offsets, cardinality_check=True)
    b = auction_solve_sparse_batch(*src, offsets, cardinality_check=False)
    _same_result(a, b)


def test_sparse_infeasible_at_the_cap():
    rng = np.random.default_rng(7)
    big = _narrow_sparse(rng, 2048, 2048, 1000)
    probs = [_problem(rng, 100, 120, 3), big] + [_problem(rng, 30, 40, 3) for _ in range(SPARSE_B)]
    b, text = _sparse_error(probs, False)
    assert b == 1 and "Maximum matching" in text


def _min_matching_ms(call, reps=3):
    return min(call()["meta"]["gpu"]["matching_ms"] for _ in range(reps))


def test_the_device_guard_runs_for_large_batches():
    """A timing signal that the guard ran on the device, with a wide margin.  Measured on one MI355X: dense 1024 x 100
    0.12 ms on the device against 1.8 ms for the host guard (16 threads); sparse 1024 x 64 with 8 entries per row
    0.15 ms against 0.70 ms.  The host guard cannot come under these bounds."""
    rng = np.random.default_rng(8)
    mats = rng.uniform(0, 100, (1024, 100, 100))
    auction_solve_batch(mats, cardinality_check=True)  # warm-up
    assert _min_matching_ms(lambda: auction_solve_batch(mats, cardinality_check=True)) < 0.6
    loc, val, offsets = _pack([_problem(rng, 64, 64, 8) for _ in range(1024)])
    auction_solve_sparse_batch(loc, val, offsets, cardinality_check=True)
    assert _min_matching_ms(lambda: auction_solve_sparse_batch(loc, val, offsets, cardinality_check=True)) < 0.4
