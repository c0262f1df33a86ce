"""auction_solve_sparse_batch / auction_solve_ell_batch(finish="reverse") on the GPU (misslap_sparse_batch_reverse_finish,
misslap_ell_batch_reverse_finish; k_list_reverse_finish in csrc/kernels_list_finish.hpp).

The yardstick is always sslap_amd.sparse_reverse_finish, the numpy model, applied to the outputs of the SAME call with
finish=None (the forward solve is pinned to the oracle elsewhere); everything is compared bit for bit
(tests/_dense_finish.py: assert_is_the_model): sol, prices, outside_prices, reverse.its, reverse.left, meta.obj_f64 /
obj_f32 / eCE, and every other meta field, status and matching_size unchanged.  B <= 8 and `outside` is on unless a case
says otherwise, so every graph is feasible.
"""
import numpy as np
import pytest

from sslap_amd import auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch, dense_to_packed
from sslap_amd import ell_batch, sparse_batch
from tests import _dense_finish as df
from tests import _dense_finish_edges as dfe
from tests import _list_finish as lf

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _model_kw(kw):
    return dict(problem=kw.get("problem", "min"), outside=kw.get("outside"), max_iter=kw.get("max_iter", 1000000))


def _check_sparse(problems, trace=None, **kw):
    """Both calls on the packed device arrays, the model on the first one's outputs, the comparison.  Returns (forward
    result, finished result, model)."""
    loc, val, off = lf.pack(problems)
    d_loc, d_val = _dev(loc), _dev(val)
    r0 = auction_solve_sparse_batch(d_loc, d_val, off, errors="status", **kw)
    r1 = auction_solve_sparse_batch(d_loc, d_val, off, errors="status", finish="reverse", **kw)
    want = lf.model_of((loc, val, off), r0, trace=trace, **_model_kw(kw))
    lf.assert_is_the_model(r1, r0, want)
    return r0, r1, want


def _check_ell(cols, vals, rows=None, trace=None, **kw):
    from sslap_amd import ell_to_packed
    d_cols, d_vals = _dev(cols), _dev(vals)
    r0 = auction_solve_ell_batch(d_cols, d_vals, rows, errors="status", **kw)
    r1 = auction_solve_ell_batch(d_cols, d_vals, rows, errors="status", finish="reverse", **kw)
    want = lf.model_of(ell_to_packed(cols, vals.astype(np.float64), rows), r0, trace=trace, **_model_kw(kw))
    lf.assert_is_the_model(r1, r0, want)
    return r0, r1, want


def _batch(seed, ns, ms, ints=False, **kw):
    """Gated problems of ns x ms, an outside value per row and starting prices that leave work for the finish."""
    rng = np.random.default_rng(seed)
    problems = [lf.gated_problem(rng, n, m, ints=ints, **kw) for n, m in zip(ns, ms)]
    B, N, M = len(ns), max(ns), max(max(ms), 1)
    return problems, dict(outside=np.floor(rng.uniform(20, 60, (B, N))), prices=np.floor(rng.uniform(0, 120, (B, M)) * 8) / 8)


# ---- the column-length ladder ---------------------------------------------------------------------------------------------
LADDER = (0, 1, 2, 63, 64, 65, 130)
LADDER_COL = 0


def ladder_case(c, problem):
    """n = max(c, 2) + 3 rows, m = n + 2 columns: row i has its own column 2 + i, and the rows below c also have column
    0, which is worth more than any own column and starts priced far above everything: after the forward solve it is
    open, holds c entries and is taken (c > 0) by a row.  Values are given as maximised values a: problem="max" stores
    a, "min" the cost 300 - a."""
    rng = np.random.default_rng([11, c, problem == "max"])
    n = max(c, 2) + 3
    own, top = 50.0 + rng.integers(0, 10, n), 100.0 + rng.integers(0, 20, n)
    loc, a = [], []
    for i in range(n):
        if i < c:
            loc.append((i, LADDER_COL))
            a.append(top[i])
        loc.append((i, 2 + i))
        a.append(own[i])
    a = np.array(a)
    val = a if problem == "max" else 300.0 - a
    prices = np.zeros((1, n + 2))
    prices[0, LADDER_COL] = 500.0
    outside = 5.0 if problem == "max" else 295.0
    return (np.array(loc, dtype=np.int32), val), dict(problem=problem, fast=True, prices=prices, outside=outside), n


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("c", LADDER)
def test_the_column_length_ladder(gpu_lib, c, problem):
    (loc, val), kw, n = ladder_case(c, problem)
    trace = []
    r0, _, want = _check_sparse([(loc, val)], trace=trace, **kw)
    # the situation: the priced column is open behind the forward solve, holds c entries and the finish processes it
    assert np.count_nonzero(loc[:, 1] == LADDER_COL) == c and lf.shapes_of(r0).tolist() == [[n, n + 2]]
    assert LADDER_COL not in df.host(r0["sol"])[0].tolist() and df.host(r0["prices"])[0, LADDER_COL] == 500.0
    first = next(t for t in trace if t[1] == LADDER_COL)
    assert (first[2] >= 0) == (c > 0) and want["reverse"]["left"][0] == 0
    cols, vals = lf.to_ell([(loc, val)], [n], 2)
    _, _, want_ell = _check_ell(cols, vals, n_cols=n + 2, **kw)
    assert want_ell["sol"].tobytes() == want["sol"].tobytes() and np.array_equal(want_ell["reverse"]["its"], want["reverse"]["its"])


# ---- row and carve edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 64, 65, 257])
def test_the_row_edges(gpu_lib, n):
    problems, kw = _batch(n, [n] * 3, [n + 7] * 3)
    _, _, want = _check_sparse(problems, fast=True, sizes=np.array([[0, n]] * 3), **kw)
    assert want["ran"].all() and (want["reverse"]["left"] == 0).all() and want["reverse"]["its"].sum() > 0
    cols, vals = lf.to_ell(problems, [n] * 3, 4, np.random.default_rng(n))
    _check_ell(cols, vals, fast=True, **kw)


def test_more_rows_than_columns(gpu_lib):
    problems, kw = _batch(3, [40, 33, 9], [7, 12, 2])
    _, _, want = _check_sparse(problems, fast=True, problem="max", sizes=np.array([[0, 40], [0, 33], [0, 9]]), **kw)
    assert want["ran"].all() and want["reverse"]["its"].sum() > 0


def test_leading_dimensions_larger_than_every_problem(gpu_lib):
    ns, ms = [20, 31, 5], [40, 28, 9]
    problems, kw = _batch(4, ns, ms)
    N, M = max(ns) + 3, max(ms) + 5
    kw = dict(outside=np.pad(kw["outside"], ((0, 0), (0, 3)), constant_values=np.nan),
              prices=np.pad(kw["prices"], ((0, 0), (0, 5)), constant_values=7.0))
    _, r1, want = _check_sparse(problems, fast=True, dims=(N, M), sizes=np.array([[0, n] for n in ns]), **kw)
    assert tuple(r1["sol"].shape) == (3, N) and tuple(r1["prices"].shape) == (3, M) and want["reverse"]["its"].sum() > 0
    cols, vals = lf.to_ell(problems, ns, 4)
    cols, vals = np.pad(cols, ((0, 0), (0, 3), (0, 0)), constant_values=5), np.pad(vals, ((0, 0), (0, 3), (0, 0)))
    _check_ell(cols, vals, rows=np.array(ns, dtype=np.int32), n_cols=M, fast=True, **kw)


def test_a_batch_of_mixed_sizes(gpu_lib):
    ns, ms = [1, 257, 40, 2, 130], [1, 300, 3, 60, 131]
    problems, kw = _batch(5, ns, ms)
    _, _, want = _check_sparse(problems, fast=True, sizes=np.array([[0, n] for n in ns]), **kw)
    assert want["ran"].all() and (want["reverse"]["its"][[1, 4]] > 0).all()


@pytest.mark.parametrize("front", ["sparse", "ell"])
def test_the_full_carve(gpu_lib, front):
    """One 2048 x 2048 problem with K = 2 and outside: 4096 objects, the carve above 64 KiB."""
    rng = np.random.default_rng(2048)
    n = 2048
    cols = np.stack([rng.permutation(n), rng.integers(0, n, n)], axis=1)
    cols[cols[:, 0] == cols[:, 1], 1] = -1
    cols[0, 0] = n - 1  # (the last column exists)
    if cols[0, 1] == n - 1:
        cols[0, 1] = -1
    vals = rng.uniform(0, 100, (n, 2))
    kw = dict(fast=True, problem="max", outside=rng.uniform(20, 50, (1, n)), prices=rng.uniform(0, 60, (1, n)))
    if front == "ell":
        _, _, want = _check_ell(cols[None].astype(np.int32), vals[None], n_cols=n, **kw)
    else:
        i, k = np.nonzero(cols >= 0)
        _, _, want = _check_sparse([(np.stack([i, cols[i, k]], axis=1).astype(np.int32), vals[i, k])], dims=(n, n), **kw)
    print("full carve:", front, "its", want["reverse"]["its"].tolist())
    assert want["ran"].all() and want["reverse"]["its"][0] > 0 and want["reverse"]["left"][0] == 0


# ---- the situations of the dense finish, packed -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(df.situations()))
def test_the_hand_built_situations_packed(gpu_lib, name):
    """Without outside: the packed problem is the dense one, so the forward state and the trace are the dense case's."""
    case = df.situations()[name]
    trace = []
    B, N, M = case["mats"].shape  # (sizes: without them from_sparse's N is the largest row INDEX, 0 for a one-row problem)
    r0, _, want = _check_sparse(dense_to_packed(case["mats"]), trace=trace, sizes=np.array([[M, N]] * B), **case["kw"])
    assert want["ran"].all() and df.situation_holds(case, r0, want, trace), trace[:8]


def test_a_row_without_any_real_entry(gpu_lib):
    """Its outside object is priced +inf by its one-entry bid and its profit is -inf: it never moves, the rest does."""
    rng = np.random.default_rng(21)
    loc, val = lf.gated_problem(rng, 12, 20, empty=0.0)
    keep = loc[:, 0] != 5
    kw = dict(fast=True, problem="max", outside=np.floor(rng.uniform(10, 40, (1, 12))), prices=np.floor(rng.uniform(0, 90, (1, 20))))
    r0, r1, want = _check_sparse([(loc[keep], val[keep])], sizes=np.array([[0, 12]]), **kw)
    assert np.isposinf(df.host(r0["outside_prices"])[0, 5]) and np.isposinf(df.host(r1["outside_prices"])[0, 5])
    assert want["sol"][0, 5] == -1 and want["reverse"]["its"][0] > 0 and want["reverse"]["left"][0] == 0


def test_an_outside_object_is_freed_and_taken_again(gpu_lib):
    """The dense case built for it, packed: a chained outside object goes back to its row, and another drops."""
    case = dfe.outside_loop_case()
    trace = []
    kw = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case["kw"].items()}
    _, _, want = _check_sparse(dense_to_packed(case["mats"]), trace=trace, **kw)
    dfe._claim_outside_loop(case, None, want, trace)


# ---- one family ---------------------------------------------------------------------------------------------------------------
def _same_bits(got, want, keys=("sol", "prices", "outside_prices", "status")):
    for key in keys:
        assert df.host(got[key]).tobytes() == df.host(want[key]).tobytes(), key
    for key in ("its", "left"):
        assert np.array_equal(df.host(got["reverse"][key]), df.host(want["reverse"][key])), key


def test_one_family_through_every_front_end(gpu_lib):
    import torch
    ns, ms = [17, 40, 3, 66], [30, 25, 9, 70]
    problems, kw = _batch(8, ns, ms, empty=0.15)  # (ascending columns; values and prices are float32-exact)
    B, N, M = len(ns), max(ns), max(ms)
    sizes = np.array([[0, n] for n in ns])
    kw.update(fast=True, problem="min")
    loc, val, off = lf.pack(problems)
    base = auction_solve_sparse_batch(_dev(loc), _dev(val), off, errors="status", finish="reverse", dims=(N, M), sizes=sizes, **kw)
    rec = lf.records(base)
    assert (df.host(base["status"]) == 0).all() and df.host(base["reverse"]["its"]).sum() > 0
    # the int64 / strided / float32 view with device offsets and sizes
    wide = torch.zeros((len(val), 3), dtype=torch.int64, device="cuda")
    wide[:, 1:] = _dev(loc.astype(np.int64))
    view = auction_solve_sparse_batch(wide[:, 1:], _dev(val.astype(np.float32)), _dev(off), errors="status", finish="reverse",
                                      dims=(N, M), sizes=_dev(sizes.astype(np.int64)), **kw)
    _same_bits(view, base)
    assert lf.records(view).tobytes() == rec.tobytes()
    # a list of pairs on the host: uploaded once, numpy arrays back
    pairs = auction_solve_sparse_batch(problems, errors="status", finish="reverse", dims=(N, M), sizes=sizes, **kw)
    assert isinstance(pairs["sol"], np.ndarray) and isinstance(pairs["reverse"]["its"], np.ndarray)
    _same_bits(pairs, base)
    assert np.array_equal(df.bits(pairs["meta"]["obj_f64"]), df.bits(rec["obj_f64"]))
    # ELL in both index and value types, the holes moved
    for k, (ct, vt) in enumerate([(np.int32, np.float64), (np.int64, np.float32), (np.int32, np.float32), (np.int64, np.float64)]):
        cols, vals = lf.to_ell(problems, ns, 5, np.random.default_rng(k), ct, vt)
        ell = auction_solve_ell_batch(_dev(cols), _dev(vals), np.array(ns, dtype=np.int32), n_cols=M, errors="status",
                                      finish="reverse", **kw)
        _same_bits(ell, base)
        r = lf.records(ell)
        for f in ("obj_f64", "obj_f32", "eCE", "n_assigned", "its"):
            assert r[f].tobytes() == rec[f].tobytes(), f
    # the densified stack through the dense batch: rows are stored in ascending column order
    mats = np.full((B, N, M), np.nan)
    shapes = lf.shapes_of(base).astype(np.int32)
    for b, (lb, vb) in enumerate(problems):
        mats[b, lb[:, 0], lb[:, 1]] = vb
    dense = auction_solve_batch(_dev(mats), errors="status", entries="finite", finish="reverse", shapes=shapes, **kw)
    _same_bits(dense, base)


def test_without_outside_rectangular_with_the_guard(gpu_lib):
    rng = np.random.default_rng(12)
    problems = []
    for n, m in [(20, 45), (64, 70), (5, 6)]:
        own = rng.permutation(m)[:n]
        cols = [np.union1d(rng.permutation(m)[:3], [own[i]]) for i in range(n)]
        loc = np.array([(i, j) for i in range(n) for j in cols[i]], dtype=np.int32)
        problems.append((loc, np.floor(rng.uniform(0, 100, len(loc)) * 8) / 8))
    prices = np.floor(rng.uniform(0, 150, (3, 70)))
    for problem in ("min", "max"):
        r0, _, want = _check_sparse(problems, problem=problem, fast=True, prices=prices, cardinality_check=True)
        assert (df.host(r0["matching_size"]) == [20, 64, 5]).all() and want["ran"].all() and want["reverse"]["its"].sum() > 0
    cols, vals = lf.to_ell(problems, [20, 64, 5], 4)
    _check_ell(cols, vals, rows=np.array([20, 64, 5], dtype=np.int32), n_cols=70, fast=True, prices=prices)


# ---- not run, budget, stall, duplicates, order ----------------------------------------------------------------------------------
def test_a_condemned_problem_and_a_cut_one_are_untouched(gpu_lib):
    """Problem 1 holds a NaN (status != 0); problem 2 is contested and max_iter = 3 cuts its forward solve; the two
    small ones finish.  assert_is_the_model compares every output of the problems that did not run byte for byte."""
    rng = np.random.default_rng(13)
    small = [(np.array([[0, 0], [0, 3], [1, 1], [1, 3]], dtype=np.int32), np.array([9.0, 30.0, 8.0, 28.0])) for _ in range(2)]
    bad = (small[0][0], np.array([9.0, np.nan, 8.0, 28.0]))
    n = 40
    big = (np.array([(i, j) for i in range(n) for j in range(4)], dtype=np.int32), rng.uniform(50, 60, 4 * n))
    problems = [small[0], bad, big, small[1]]
    prices = np.zeros((4, 4))
    prices[:, 3] = 100.0
    r0, r1, want = _check_sparse(problems, problem="max", fast=True, max_iter=3, outside=1.0, prices=prices)
    assert df.host(r0["status"]).tolist() == [0, df.host(r0["status"])[1], 0, 0] and df.host(r0["status"])[1] != 0
    assert want["ran"].tolist() == [True, False, False, True]
    assert df.host(r1["reverse"]["its"])[[1, 2]].tolist() == [-1, -1] and df.host(r1["reverse"]["left"])[[1, 2]].tolist() == [-1, -1]
    assert (want["reverse"]["its"][[0, 3]] >= 1).all()


@pytest.mark.parametrize("front", ["sparse", "ell"])
def test_the_budget(gpu_lib, front):
    """_reverse_finish_launch with a budget of its own on a forward result: 1, and the model's its - 1."""
    from sslap_amd import ell_to_packed
    ns = [30, 44]
    problems, kw = _batch(14, ns, [50, 60])
    kw.update(fast=True, problem="max")
    loc, val, off = lf.pack(problems)
    cols, vals = lf.to_ell(problems, ns, 4)
    rows = np.array(ns, dtype=np.int32)

    def forward():
        if front == "sparse":
            return auction_solve_sparse_batch(_dev(loc), _dev(val), off, errors="status", sizes=np.array([[0, n] for n in ns]), **kw)
        return auction_solve_ell_batch(_dev(cols), _dev(vals), rows, errors="status", **kw)

    packed = (loc, val, off) if front == "sparse" else ell_to_packed(cols, vals, rows)
    launch = (sparse_batch if front == "sparse" else ell_batch)._reverse_finish_launch
    full = lf.model_of(packed, forward(), problem="max", outside=kw["outside"])
    assert (full["reverse"]["its"] > 2).all()
    for budget in (1, int(full["reverse"]["its"].min()) - 1):
        r0, r1 = forward(), forward()
        its, left = launch(r1, "max", budget)
        want = lf.model_of(packed, r0, problem="max", outside=kw["outside"], max_iter=budget)
        lf.assert_is_the_model(r1, r0, want)
        assert df.host(its).tolist() == [budget, budget] and (df.host(left) > 0).all() and its is r1["reverse"]["its"]


def test_a_stall_ends_the_finish_with_objects_left(gpu_lib):
    """Values near 2^52 and eps = 1 / n, as tests/_dense_finish_edges.py builds its stall ("2_47-max", without outside):
    a move would not raise the moving row's profit, the finish ends with left > 0 and status stays 0."""
    case = dfe.value_case("2_47-max")
    trace = []
    r0, r1, want = _check_sparse(dense_to_packed(case["mats"]), trace=trace, problem="max", fast=True,
                                 prices=np.array(case["kw"]["prices"]), max_iter=dfe.FINISH_BUDGET)
    assert df.host(r1["status"]).tolist() == [0] and want["reverse"]["left"][0] > 0
    assert want["reverse"]["its"][0] < dfe.FINISH_BUDGET and trace[-1][2] >= 0 and trace[-1][3] == -1, trace[-1]


def test_duplicates(gpu_lib):
    """The CPU case on the GPU, from prices that leave object 2 open: the largest copy decides the move, the last stored
    copy is the choice of the eCE test and the objective counts every copy."""
    d = lf.duplicates_case()
    kw = dict(problem="max", eps_start=0.5, prices=np.array(d["prices"]), cardinality_check=False)
    trace = []
    r0, r1, want = _check_sparse([(d["loc"], d["val"])], trace=trace, **kw)
    assert df.host(r0["sol"]).tolist() == [[0, 1]] and [t[1:4] for t in trace] == [(2, 0, 0)]
    assert want["sol"].tolist() == [[2, 1]] and want["obj_f64"][0] == 5.0 + 9.0 + 7.0 + 4.0
    cols, vals = lf.to_ell([(d["loc"], d["val"])], [2], 5, np.random.default_rng(1))
    _, _, want_ell = _check_ell(cols, vals, **kw)
    assert want_ell["sol"].tolist() == [[2, 1]] and want_ell["obj_f64"][0] == want["obj_f64"][0]


def test_the_same_call_twice_gives_the_same_bits(gpu_lib):
    """Long columns (hundreds of entries each) scattered by atomics: the index's order may differ between two runs,
    the result may not."""
    rng = np.random.default_rng(15)
    n, m = 300, 12
    loc = np.array([(i, j) for i in range(n) for j in np.sort(rng.permutation(m)[:6])], dtype=np.int32)
    val = np.floor(rng.uniform(0, 16, len(loc)))  # (small integers: many exact ties within a column)
    loc2, val2, off = lf.pack([(loc, val)] * 2)
    kw = dict(errors="status", finish="reverse", fast=True, problem="max", outside=np.tile(np.floor(rng.uniform(0, 10, n)), (2, 1)),
              prices=np.tile(np.floor(rng.uniform(0, 40, m)), (2, 1)))
    runs = [auction_solve_sparse_batch(_dev(loc2), _dev(val2), off, **kw) for _ in range(2)]
    _same_bits(runs[1], runs[0])
    assert lf.records(runs[1]).tobytes() == lf.records(runs[0]).tobytes()
    assert (df.host(runs[0]["reverse"]["its"]) > 0).all()
    for key in ("sol", "prices", "outside_prices"):  # (two copies of one problem in one call)
        assert df.host(runs[0][key])[0].tobytes() == df.host(runs[0][key])[1].tobytes(), key
    its = df.host(runs[0]["reverse"]["its"])
    assert its[0] == its[1]
