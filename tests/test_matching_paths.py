"""k_matching_batch (csrc/kernels_matching_batch.hpp) where its DFS recurses, backtracks and crosses lanes: the graphs
of _matching_shapes.py, through every call site of the kernel, against the model's result on each source's own stored
order (_matching_model.py; test_matching_paths_nogpu.py pins the model to the host matcher and to the reference's golden
vectors, and shows which steps the graphs reach).  hopcroft_solve_batch returns the pairings: they are compared bit for
bit.  The guards of the batch solves report the cardinality: the batches mix feasible graphs with graphs short by one or
two rows, and status, matching_size and the default mode's text must carry the model's numbers.  Every comparison is an
exact integer equality."""
import numpy as np
import pytest

import _matching_shapes as S
from sslap_amd import _lib, auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch, hopcroft_solve_batch

pytestmark = pytest.mark.gpu

INFEASIBLE = _lib.BATCH_STATUS_INFEASIBLE


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _check_pairings(res, names, source):
    left, right = _host(res["left_pairings"]), _host(res["right_pairings"])
    want = [S.expect(name, source) for name in names]
    assert left.shape == (len(names), max(e.n for e in want)) and right.shape == (len(names), max(e.m for e in want))
    for b, (name, e) in enumerate(zip(names, want)):
        assert res["size"][b] == e.size, name
        assert res["n_rows"][b] == e.n and res["n_cols"][b] == e.m, name
        assert np.array_equal(left[b, :e.n], e.left), name
        assert np.array_equal(right[b, :e.m], e.right), name
        assert (left[b, e.n:] == -1).all() and (right[b, e.m:] == -1).all(), name


def test_loc_every_case_in_one_call():
    """The carve is the largest graph's; most graphs are far smaller than it."""
    names = S.names("loc")
    loc, offsets = S.pack([S.loc_of(S.cases()[name]) for name in names])
    before = loc.copy()
    res = hopcroft_solve_batch(loc, offsets)
    _check_pairings(res, names, "loc")
    assert np.array_equal(loc, before)
    sizes = {name: int(res["size"][b]) - S.cases()[name].n for b, name in enumerate(names)}
    assert 0 in sizes.values() and -1 in sizes.values() and -2 in sizes.values()


def _typed_stack(dtype, device):
    """(the stack in its element type, a bit-for-bit copy to compare with afterwards, shapes)."""
    import torch
    mats, shapes = S.dense_stack64()
    t = torch.from_numpy(mats.copy()).to(getattr(torch, dtype))
    assert torch.equal(t.double().nan_to_num(nan=-7.0), torch.from_numpy(mats.copy()).nan_to_num(nan=-7.0))  # exact
    if device:
        t = t.cuda()
        return t, t.clone(), shapes
    a = t.numpy()
    return a, a.copy(), shapes


def _bits(x):
    if isinstance(x, np.ndarray):
        return x.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[x.dtype.itemsize])
    import torch
    return x.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[x.element_size()]).cpu().numpy()


# (numpy has no bfloat16: that stack is a device tensor)
@pytest.mark.parametrize("dtype,device", [(d, dev) for d in S.DENSE_DTYPES for dev in (False, True)
                                          if dev or d != "bfloat16"])
def test_dense_stack_in_every_element_type(dtype, device):
    """mats= with shapes, inside a larger carve whose padding is +inf (an entry, if it were read); entries are 1.0, -0.0
    and +inf, anything else -1.0 and NaN."""
    pytest.importorskip("torch")
    mats, before, shapes = _typed_stack(dtype, device)
    res = hopcroft_solve_batch(mats=mats, shapes=shapes, mat_dtype=dtype)
    _check_pairings(res, S.names("dense"), "dense")
    assert res["left_pairings"].shape[1] < mats.shape[1] and res["right_pairings"].shape[1] < mats.shape[2]
    assert np.array_equal(_bits(mats), _bits(before))  # read in place, never written


# ---- the guards --------------------------------------------------------------------------------------------------------------
# The status-mode calls stop the auction after a few rounds (the oracle-parity suites own its result; a stopped solve
# keeps status 0): what is looked at here is decided before the first round.
FEW_ROUNDS = 20


def _check_guard(res, want):
    """status and matching_size against the model's [(name, size, n)]: 0 where every row is matched, else INFEASIBLE
    with sol -1."""
    status, msize, sol = _host(res["status"]), _host(res["matching_size"]), _host(res["sol"])
    for b, (name, size, n) in enumerate(want):
        assert msize[b] == size, (name, msize[b], size)
        assert status[b] == (0 if size == n else INFEASIBLE), name
        if size < n:
            assert (sol[b] == -1).all(), name
    return {size - n for _, size, n in want}


def _pattern(name):
    return S.pattern_of(S.cases()[name])


@pytest.mark.parametrize("device", [False, True])
def test_dense_status_guard(device):
    mats, shapes = S.guard_dense_stack(S.GUARD_DENSE, pad=(2, 3))
    src = mats
    if device:
        torch = pytest.importorskip("torch")
        src = torch.from_numpy(mats).cuda()
    res = auction_solve_batch(src, shapes=shapes, errors="status", max_iter=FEW_ROUNDS)
    want = [(name, S.expect(name, "dense").size, S.cases()[name].n) for name in S.GUARD_DENSE]
    assert {0, -1, -2} <= _check_guard(res, want)


@pytest.mark.parametrize("device", [False, True])
def test_sparse_status_guard_with_dims_beyond_every_graph(device):
    loc, val, offsets = S.guard_sparse_batch(S.GUARD_SPARSE)
    cs = [S.cases()[name] for name in S.GUARD_SPARSE]
    dims = (max(c.n for c in cs) + 7, max(c.m for c in cs) + 9)
    src = (loc, val)
    if device:
        torch = pytest.importorskip("torch")
        src = (torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda())
    res = auction_solve_sparse_batch(*src, offsets, errors="status", dims=dims, max_iter=FEW_ROUNDS)
    want = [(c.name, S.expect(c.name, "loc").size, c.n) for c in cs]
    assert {0, -1, -2} <= _check_guard(res, want)
    assert _host(res["sol"]).shape == (len(cs), dims[0])


@pytest.mark.parametrize("wide", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("K", S.ELL_KS)
def test_ell_guard(K, wide):
    cols, vals, rows, names = S.guard_ell_stack(K, wide)
    res = auction_solve_ell_batch(cols, vals, rows=rows, errors="status", max_iter=FEW_ROUNDS)
    want = [(name, S.expect(name, "ell", K).size, S.cases()[name].n) for name in names]
    kinds = _check_guard(res, want)
    assert 0 in kinds and min(kinds) < 0  # feasible and infeasible graphs in every stack
    if K == 110:
        assert {0, -1, -2} <= kinds


def test_ell_guard_on_device_columns():
    torch = pytest.importorskip("torch")
    cols, vals, rows, names = S.guard_ell_stack(110, True)
    res = auction_solve_ell_batch(torch.from_numpy(cols).cuda(), torch.from_numpy(vals).cuda(), rows=rows, errors="status",
                                  max_iter=FEW_ROUNDS)
    want = np.array([S.expect(name, "ell", 110).size for name in names])
    ns = np.array([S.cases()[name].n for name in names])
    assert np.array_equal(_host(res["matching_size"]), want)
    assert np.array_equal(_host(res["status"]), np.where(want == ns, 0, INFEASIBLE))
    assert (want == ns).any() and (want == ns - 1).any() and (want == ns - 2).any()


def _cycle(names, B):
    return [names[b % len(names)] for b in range(B)]


def _first_infeasible_text(names, source):
    for b, name in enumerate(names):
        e = S.expect(name, source)
        if e.size < e.n:
            return (f"problem {b}: Matrix is infeasible (Maximum matching possible only involves {e.size} out of {e.n} "
                    f"rows.)")
    raise AssertionError("no infeasible graph in the batch")


def _is_permutation(sol, names):
    for b, name in enumerate(names):
        n = S.cases()[name].n
        s = sol[b, :n]
        assert (s >= 0).all() and np.unique(s).shape[0] == n and _pattern(name)[np.arange(n), s].all(), (b, name)
        assert (sol[b, n:] == -1).all(), (b, name)


def test_dense_default_guard_on_the_device_from_64_problems():
    names = _cycle(S.GUARD_DENSE, 64)
    mats, shapes = S.guard_dense_stack(names)
    with pytest.raises(ValueError) as e:
        auction_solve_batch(mats, shapes=shapes, cardinality_check=True)
    assert str(e.value) == _first_infeasible_text(names, "dense")
    good = _cycle([name for name in S.GUARD_DENSE if S.expect(name, "dense").size == S.cases()[name].n], 64)
    mats, shapes = S.guard_dense_stack(good)
    res = auction_solve_batch(mats, shapes=shapes, cardinality_check=True)
    _is_permutation(_host(res["sol"]), good)
    assert res["meta"]["gpu"]["matching_ms"] > 0


def test_sparse_default_guard_on_the_device_from_256_problems():
    """256 problems that reuse 8 distinct graphs cyclically."""
    names = _cycle(S.GUARD_EIGHT, 256)
    loc, val, offsets = S.guard_sparse_batch(names)
    with pytest.raises(ValueError) as e:
        auction_solve_sparse_batch(loc, val, offsets, cardinality_check=True)
    assert str(e.value) == _first_infeasible_text(names, "loc")
    good = _cycle([name for name in S.GUARD_EIGHT if S.expect(name, "loc").size == S.cases()[name].n], 256)
    loc, val, offsets = S.guard_sparse_batch(good)
    res = auction_solve_sparse_batch(loc, val, offsets, cardinality_check=True)
    _is_permutation(_host(res["sol"]), good)
