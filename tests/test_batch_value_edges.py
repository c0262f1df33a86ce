"""The batch solves on the GPU at the edges of the value range (the cases of tests/_value_edges.py): negative entries,
rows of mixed signs, a C = max |v| that a negative entry or an outside value sets alone, -0.0; a C that is +inf, 0, a
subnormal or inexact as a float32; magnitudes of 2^52 .. 2^54, where eps falls below one ulp of the prices; an eps_start
of 0 after narrowing, of the smallest float32 subnormal, near FLT_MAX and +inf; and eps = (float)(1.0 / n) at row counts
whose reciprocal is inexact.

Every case goes through every entry point that accepts its values, for both problems, and every output is compared
with the oracle's with `==` on every bit (sparse_compare / dense_compare of tests/_batch_shapes.py, compare of the
outside tests): sol with its -1 tail, the meta fields, obj_f64, the fp32 bits of start_eps / final_eps, the price bits,
n_assigned.  The cases of one entry point travel in one batch per (rows, eps_start, stop), so a workgroup that spins at
eps == 0 or at eps == +inf until max_iter runs beside converging ones.  A solve that does not end on its own always has
an explicit max_iter (test_batch_value_edges_nogpu.py holds the oracle of every case to its stop); cardinality_check is
off throughout: the planted matching makes every graph feasible and the guard is tested elsewhere.
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch
from tests import _sparse_outside_fixture as sof
from tests import _value_edges as ve
from tests import test_dense_outside as dense_out
from tests import test_ell_outside as ell_out
from tests import test_sparse_outside as sparse_out
from tests._batch_shapes import bits, dense_compare, sparse_compare, sparse_pack, threads_for
from tests.test_dense_batch_status import _to_host as _dense_to_host
from tests.test_ell_batch import _device as _ell_device, _to_host as _ell_to_host, _typed
from tests.test_sparse_batch_status import _device as _sparse_device, _to_host as _sparse_to_host

pytestmark = pytest.mark.gpu

ELL_DTYPES = ((np.int32, np.float64), (np.int64, np.float32))


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _quiet_narrowing():
    """eps_start = 1e39 narrows to +inf as a float32, which numpy reports: that is the case."""
    with np.errstate(over="ignore"):
        yield


def _sparse_groups(f32=False):
    cases = [c for c in ve.sparse_cases().values() if not f32 or ve.has_f32(c)]
    return ve.groups(cases)


def _ok(res, B):
    assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
    assert (res["matching_size"] == -1).all()  # no guard in these calls
    assert res["sol"].shape[0] == B


# ---- the sparse entry point

@pytest.mark.parametrize("problem", ve.PROBLEMS)
def test_sparse_default_mode_from_host_arrays(problem):
    seen = 0
    for rows, opts, stop, cases in _sparse_groups():
        loc, val, off = sparse_pack([ve.sparse_problem_of(c) for c in cases])
        res = auction_solve_sparse_batch(loc, val, off, problem=problem, **ve.call_opts(opts, stop))
        assert res["sol"].shape == (len(cases), rows) and res["meta"]["gpu"]["threads"] == threads_for(rows)
        for b, c in enumerate(cases):
            sparse_compare(res, b, ve.sparse_want(c.name, problem))
            seen += 1
    assert seen == len(ve.sparse_cases())


@pytest.mark.parametrize("problem", ve.PROBLEMS)
def test_sparse_status_mode_from_device_tensors_with_dims(problem):
    seen = 0
    for rows, opts, stop, cases in _sparse_groups():
        loc, val, off = sparse_pack([ve.sparse_problem_of(c) for c in cases])
        dl, dv = _sparse_device(loc, val)
        res = _sparse_to_host(auction_solve_sparse_batch(dl, dv, off, problem=problem, errors="status",
                                                         dims=(rows, rows + 3), **ve.call_opts(opts, stop)))
        _ok(res, len(cases))
        assert res["sol"].shape == (len(cases), rows) and res["prices"].shape == (len(cases), rows + 3)
        for b, c in enumerate(cases):
            sparse_compare(res, b, ve.sparse_want(c.name, problem))
            seen += 1
        assert np.array_equal(bits(dv.cpu().numpy()), bits(val))  # never written, 'min' included
    assert seen == len(ve.sparse_cases())


# ---- the padded form

@pytest.mark.parametrize("problem", ve.PROBLEMS)
@pytest.mark.parametrize("itype,vtype", ELL_DTYPES, ids=["i32-f64", "i64-f32"])
def test_ell_for_both_value_types(itype, vtype, problem):
    """(int32, float64) from host arrays, (int64, float32) from device tensors; the oracle of a float32 call is the oracle
    of the rounded values, and a case with a value above FLT_MAX has no float32."""
    f32 = vtype is np.float32
    seen = set()
    for rows, opts, stop, cases in _sparse_groups(f32):
        probs = [ve.sparse_problem_of(c, f32) for c in cases]
        cols, vals, rws = sof.to_ell(probs, [rows] * len(cases), rows)
        cols, vals = _typed(cols, vals, itype, vtype)
        assert np.array_equal(vals[cols >= 0].astype(np.float64).view(np.uint64),
                              np.concatenate([p[1] for p in probs]).view(np.uint64))  # (-0.0 and subnormals kept)
        kw = dict(rows=rws, n_cols=rows, problem=problem, errors="status", **ve.call_opts(opts, stop))
        if f32:
            dc, dv = _ell_device(cols, vals)
            res = _ell_to_host(auction_solve_ell_batch(dc, dv, **kw))
        else:
            res = auction_solve_ell_batch(cols, vals, **kw)
        _ok(res, len(cases))
        assert res["sol"].shape == (len(cases), rows) and res["meta"]["gpu"]["threads"] == threads_for(rows)
        for b, c in enumerate(cases):
            sparse_compare(res, b, ve.sparse_want(c.name, problem, f32))
            seen.add(c.name)
    assert seen == set(ve.sparse_cases()) - ({"above_flt_max", "dbl_max"} if f32 else set())


# ---- eps = (float)(1.0 / n) per problem

@pytest.mark.parametrize("problem", ve.PROBLEMS)
def test_fast_on_problems_of_1_2_3_7_and_70_rows(problem):
    probs, sizes = ve.fast_mix()
    sizes = sizes.copy()  # (the frozen array would travel through torch, which takes no read-only one)
    want = ve.fast_want(problem)
    B, N, M = len(probs), max(ve.FAST_ROWS), int(sizes[:, 0].max())
    loc, val, off = sparse_pack(probs)
    kw = dict(problem=problem, fast=True, cardinality_check=False)
    results = [auction_solve_sparse_batch(loc, val, off, sizes=sizes, **kw)]
    dl, dv = _sparse_device(loc, val)
    results.append(_sparse_to_host(auction_solve_sparse_batch(dl, dv, off, sizes=sizes, errors="status", dims=(N, M), **kw)))
    cols, vals, rws = sof.to_ell(probs, list(ve.FAST_ROWS), N)
    results.append(auction_solve_ell_batch(cols, vals, rows=rws, n_cols=M, errors="status", **kw))
    for res in results:
        assert res["sol"].shape == (B, N)
        for b in range(B):
            sparse_compare(res, b, want[b])
            assert np.float32(res["meta"]["start_eps_f32"][b]) == np.float32(1.0 / ve.FAST_ROWS[b])


# ---- the dense entry point

def _dense_groups(f32=False):
    cases = [c for c in ve.dense_cases().values() if not f32 or ve.dense_rounded_f32(c.val) is not None]
    return ve.groups(cases)


@pytest.mark.parametrize("problem", ve.PROBLEMS)
@pytest.mark.parametrize("route", ["host-f64", "device-f64-status", "host-f32", "device-f32-status"])
def test_dense_for_both_element_types(route, problem):
    import torch
    f32, status = "f32" in route, "status" in route
    N, M = ve.DENSE_SHAPE
    seen = set()
    for _, opts, stop, cases in _dense_groups(f32):
        mats = np.stack([ve.dense_rounded_f32(c.val) if f32 else c.val for c in cases])
        kw = dict(problem=problem, mat_dtype="float32" if f32 else "float64", **ve.call_opts(opts, stop))
        if status:
            d = torch.from_numpy(mats).cuda()
            res = _dense_to_host(auction_solve_batch(d, errors="status", **kw))
            _ok(res, len(cases))
            assert d.cpu().numpy().tobytes() == mats.tobytes()  # never written
        else:
            res = auction_solve_batch(mats, **kw)
        assert res["sol"].shape == (len(cases), N) and res["prices"].shape == (len(cases), M)
        for b, c in enumerate(cases):
            dense_compare(res, b, ve.dense_want(c.name, problem, f32), N, M)
            seen.add(c.name)
    assert seen == set(ve.dense_cases()) - ({"above_flt_max", "dbl_max"} if f32 else set())


# ---- the outside modes: an outside value that sets C alone, a huge one, zero, a small one beside values above FLT_MAX

def _outside_groups(dense=False):
    """[(stop, [(name, value)])]: the outside cases of one stop in one batch."""
    out = {}
    for name, value, in_dense in ve.OUTSIDE:
        if in_dense or not dense:
            out.setdefault(ve.outside_stop(name), []).append((name, ve.outside_dense_value(name, value) if dense else value))
    return sorted(out.items())


@pytest.mark.parametrize("problem", ve.PROBLEMS)
def test_sparse_outside(problem):
    seen = 0
    for stop, group in _outside_groups():
        probs = [ve.sparse_problem_of(ve.sparse_cases()[name]) for name, _ in group]
        outside = np.array([value for _, value in group])
        N = max(ve.sparse_cases()[name].rows for name, _ in group)
        for res in sparse_out.both(probs, outside=outside, on_device=True, dims=(N, N), problem=problem, max_iter=stop,
                                   **ve.OUTSIDE_OPTS):
            _ok(res, len(group))
            assert res["sol"].shape == (len(group), N) and res["meta"]["gpu"]["threads"] == threads_for(N)
            for b, (name, _) in enumerate(group):
                ell_out.compare(res, b, *ve.outside_sparse_want(name, problem))
                seen += 1
    assert seen == 2 * len(ve.OUTSIDE)


@pytest.mark.parametrize("problem", ve.PROBLEMS)
@pytest.mark.parametrize("itype,vtype", ELL_DTYPES, ids=["i32-f64", "i64-f32"])
def test_ell_outside(itype, vtype, problem):
    f32 = vtype is np.float32
    seen = set()
    for stop, group in _outside_groups():
        group = [(name, value) for name, value in group if not f32 or ve.has_f32(ve.sparse_cases()[name])]
        if not group:
            continue
        probs = [ve.sparse_problem_of(ve.sparse_cases()[name], f32) for name, _ in group]
        ns = [ve.sparse_cases()[name].rows for name, _ in group]
        N = max(ns)
        cols, vals, rws = sof.to_ell(probs, ns, N)
        cols, vals = _typed(cols, vals, itype, vtype)
        outside = np.array([value for _, value in group])
        for res in ell_out.both(cols, vals, rows=rws, outside=outside, on_device=f32, n_cols=N, problem=problem,
                                max_iter=stop, **ve.OUTSIDE_OPTS):
            _ok(res, len(group))
            for b, (name, _) in enumerate(group):
                ell_out.compare(res, b, *ve.outside_sparse_want(name, problem, f32))
                seen.add(name)
    assert seen == {name for name, _, _ in ve.OUTSIDE} - ({"above_flt_max"} if f32 else set())


@pytest.mark.parametrize("problem", ve.PROBLEMS)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dense_outside(dtype, problem):
    """The non-negative cases only: a negative dense entry is absent.  Zero is given as -0.0, a valid entry there."""
    f32 = dtype == "float32"
    seen = set()
    for stop, group in _outside_groups(dense=True):
        group = [(name, value) for name, value in group
                 if not f32 or ve.dense_rounded_f32(ve.dense_cases()[name].val) is not None]
        if not group:
            continue
        mats = np.stack([ve.dense_rounded_f32(ve.dense_cases()[name].val) if f32 else ve.dense_cases()[name].val
                         for name, _ in group])
        outside = np.array([value for _, value in group])
        assert not f32 or mats.dtype == np.float32
        for res in dense_out.both(mats, outside=outside, on_device=f32, mat_dtype=dtype, problem=problem, max_iter=stop,
                                  **ve.OUTSIDE_OPTS):
            _ok(res, len(group))
            for b, (name, _) in enumerate(group):
                dense_out.compare(res, b, *ve.outside_dense_want(name, problem, f32))
                seen.add(name)
    assert seen == {"ulp_2_53", "c_is_zero", "above_flt_max"} - ({"above_flt_max"} if f32 else set())


# ---- cross-layout: the sparse status call and the ELL call on the same problem return identical arrays

@pytest.mark.parametrize("problem", ve.PROBLEMS)
@pytest.mark.parametrize("name", ["neg_mixed", "ulp_2_53", "c_is_zero"])
def test_sparse_and_ell_return_identical_arrays(name, problem):
    case = ve.sparse_cases()[name]
    loc, val = ve.sparse_problem_of(case)
    n = case.rows
    kw = dict(problem=problem, errors="status", **ve.call_opts(dict(case.opts), case.stop))
    sparse = auction_solve_sparse_batch(loc, val, np.array([0, len(val)]), dims=(n, n), **kw)
    cols, vals, rws = sof.to_ell([(loc, val)], [n], n)
    ell = auction_solve_ell_batch(cols, vals, rows=rws, n_cols=n, **kw)
    for k in ("sol", "status", "matching_size"):
        assert np.array_equal(sparse[k], ell[k]), k
    assert np.array_equal(bits(sparse["prices"]), bits(ell["prices"]))
    for k, v in ell["meta"].items():
        if k not in ("timer", "gpu"):
            assert np.array_equal(np.asarray(sparse["meta"][k]).view(np.uint8), np.asarray(v).view(np.uint8)), k
    sparse_compare(sparse, 0, ve.sparse_want(name, problem))
