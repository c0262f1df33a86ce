"""The sparse batch and the ELL batch walk their rows with one row source (csrc/kernels_batch_solve.hpp: ListBatchRows,
on the run accessors SparseRuns<SparsePacked>, SparseRuns<SparseView<I, V>> and EllRuns<I, V>): which accessor a call
reaches must not change the answer.

One small ragged batch of clean problems per K, at the lane edges of the row scan and of the lane `len & 63` that takes
the outside entry (K = 1, 2, 63, 64, 65, 128: the outside entry lands on lane 0 or on a lane with a slot of its own).
Its rows: one without a hole; one with holes at the first, a middle and the last slot; rows whose extreme value is a
repeated column with tied copies, and a square problem of two columns whose rows hold nothing but repeats (the
last-stored rule and the nsel > 1 re-walk: some row must choose a column it stores twice, asserted); a problem with
rows[b] < N and, in the outside mode, a row of holes only (len = 0).  Values are integers below 2^24:
exact in float32.  The batch is presented as
  (a) the packed sparse call                                           SparseRuns<SparsePacked>
  (b) the sparse view, int64 strided loc and float32 val               SparseRuns<SparseView<long long, float>>
  (c) ELL, int32 columns and float64 values                            EllRuns<int, double>
  (d) ELL, int64 columns and float32 values, the holes of every row    EllRuns<long long, float>
      moved to other slots than in (c), which keeps the order of the entries
in the status mode with the guard on and in the outside mode with a value per row, for `min` and `max`.  Every problem
is clean (asserted, so nothing passes by comparing nothing) and all four return the same bits in status, sol, prices,
outside_prices, matching_size and meta.  The other suites tie each front end to the oracle; this file ties the front
ends to each other.  The one test without a GPU asks the oracle, on the packed form, that every problem is feasible and
solves within MAX_ITER."""
import functools

import numpy as np
import pytest

from sslap_amd import auction_solve_ell_batch, auction_solve_sparse_batch, ell_to_packed
from tests import _ell_fixture as fxt
from tests._batch_shapes import sparse_expect, sparse_pack
from tests.test_dense_one_family import outputs

MAX_ITER = 200000
KS = (1, 2, 63, 64, 65, 128)
N = 7
VMAX = 60  # values 1 .. VMAX - 1 (many ties); a planted repeated column holds 0 or VMAX + 5
LEGS = ("packed", "view", "ell_i32_f64", "ell_i64_f32")


@functools.lru_cache(maxsize=None)
def batch(K, outside):
    """dict(c=(cols, vals), d=(cols, vals), rows, out, M): the two ELL layouts (int64 (B, N, K) / float64) of one batch,
    its row counts, the outside values (B, N) with NaN beyond rows[b], and the bound on the columns.  What lies beyond
    rows[b] is column INT_MAX and +inf."""
    rng = np.random.default_rng([733, K])
    m = K + N + 3
    plans = [["full", "edges", "repeat_max", "last", "some", "none" if outside else "some", "some"],
             ["some", "repeat_min", "full"], ["repeat_max"], ["repeat_min"], ["pair", "pair"]]
    B = len(plans)
    lay = {k: (np.full((B, N, K), fxt.INT_MAX, dtype=np.int64), np.full((B, N, K), np.inf)) for k in "cd"}
    for b, plan in enumerate(plans):
        pair = plan[0] == "pair"  # a square problem of two columns: whatever a row chooses, it is stored several times
        planted = rng.permutation(2 if pair else m)[:len(plan)]  # column planted[i] is in row i: a complete matching exists
        for i, kind in enumerate(plan):
            holes = {"full": [], "edges": sorted({0, K // 2, K - 1}), "last": [K - 1], "none": list(range(K))}.get(kind)
            if holes is None:  # about a quarter of the slots, anywhere
                holes = sorted(rng.choice(K, int(rng.integers(0, K // 4 + 1)), replace=False).tolist())
            if kind != "none" and len(holes) >= K:  # (K = 1, 2: a row of a clean problem keeps an entry)
                holes = holes[:K - 1]
            k = K - len(holes)
            others = np.setdiff1d(np.arange(m), planted[i])
            col = np.concatenate([[planted[i]], rng.choice(others, max(k - 1, 0), replace=pair)])
            val = rng.integers(1, VMAX, max(k, 1)).astype(np.float64)
            if pair:
                col[1:] = ([planted[i], 1 - planted[i], 1 - planted[i]] + rng.integers(0, 2, K).tolist())[:k - 1]
                val = rng.integers(1, VMAX, 2).astype(np.float64)[col]  # (every copy of a column ties: eCE reads the last one)
            elif kind.startswith("repeat") and k >= 2:  # two tied copies of one column hold the row's extreme value
                col[1] = col[0]
                val[:2] = VMAX + 5 if kind == "repeat_max" else 0
            order = rng.permutation(k)
            col, val = col[:k][order], val[:k][order]
            at_c = np.setdiff1d(np.arange(K), holes)
            at_d = np.arange(k) if not np.array_equal(at_c, np.arange(k)) else np.arange(K - k, K)
            for at, (cols, vals) in ((at_c, lay["c"]), (at_d, lay["d"])):
                cols[b, i] = rng.choice(np.array(fxt.HOLE_COLS), K)
                vals[b, i] = rng.choice(np.array(fxt.HOLE_VALS), K)
                cols[b, i, at] = col
                vals[b, i, at] = val
            assert k in (0, K) or not np.array_equal(lay["c"][0][b, i] >= 0, lay["d"][0][b, i] >= 0)
    rows = np.array([len(p) for p in plans], dtype=np.int32)
    out = rng.integers(1, VMAX, (B, N)).astype(np.float64)  # (never tied with a repeated column's 0 or VMAX + 5)
    out[np.arange(N)[None, :] >= rows[:, None]] = np.nan
    for a in lay["c"] + lay["d"] + (rows, out):
        a.setflags(write=False)
    return dict(c=lay["c"], d=lay["d"], rows=rows, out=out, M=m)


def rewalked(cols, sol):
    """How many rows of one problem chose a column that they store more than once: the objective re-walks such a row."""
    return sum(int((cols[i] == j).sum() > 1) for i, j in enumerate(sol) if j >= 0)


def packed_form(K, outside):
    """(packed [(loc_b, val_b)] of the real entries, sizes (B, 2) = m_b, n_b) -- the same from either layout."""
    fx = batch(K, outside)
    packed = ell_to_packed(*fx["c"], fx["rows"])
    with np.errstate(over="ignore"):  # (a hole's 1e300 becomes +inf: it is never interpreted)
        vals32 = fx["d"][1].astype(np.float32)
    for (lc, vc), (ld, vd) in zip(packed, ell_to_packed(fx["d"][0], vals32, fx["rows"])):
        assert np.array_equal(lc, ld) and np.array_equal(vc, vd)  # moving holes keeps the order; float32 is exact
    sizes = np.array([[int(loc[:, 1].max()) + 1, int(n)] for (loc, _), n in zip(packed, fx["rows"])], dtype=np.int64)
    return packed, sizes


@pytest.mark.parametrize("K", KS)
def test_on_the_cpu_every_problem_is_feasible_and_solves_within_max_iter(K):
    for outside in (False, True):
        fx = batch(K, outside)
        _, sizes = packed_form(K, outside)
        packed = ell_to_packed(*fx["c"], fx["rows"], outside=fx["out"] if outside else None)
        hits = {"min": 0, "max": 0}
        for b, ((loc, val), (m, n)) in enumerate(zip(packed, sizes.tolist())):
            assert np.isfinite(val).all() and (val == val.astype(np.float32)).all() and np.abs(val).max() < 2**24
            if not outside:
                adj = [loc[loc[:, 0] == i, 1].tolist() for i in range(n)]
                assert fxt.max_matching(adj, m) == n, (K, b)
            for problem in ("min", "max"):
                size, kw = ((m + n, n), dict(fast=True, cardinality_check=False)) if outside else ((m, n), {})
                want = sparse_expect(loc, val, problem, size=size, max_iter=MAX_ITER, **kw)
                assert 0 < want["meta"]["its"] < MAX_ITER and want["meta"]["soln_found"], (K, b, problem)
                assert want["meta"]["n_assigned"] == n, (K, b, problem)
                hits[problem] += rewalked(fx["c"][0][b], want["sol"])
        assert K < 2 or (hits["min"] and hits["max"]), (K, outside, hits)


def _leg(leg, K, outside):
    """(the front end, its positional arguments on the device, its keywords) for one presentation of the batch"""
    import torch
    fx = batch(K, outside)
    if leg.startswith("ell"):
        (cols, vals), itype, vtype = (fx["c"], np.int32, np.float64) if leg == "ell_i32_f64" else (fx["d"], np.int64, np.float32)
        with np.errstate(over="ignore"):  # (a hole's 1e300 becomes +inf: it is never interpreted)
            args = (torch.from_numpy(cols.astype(itype)).cuda(), torch.from_numpy(vals.astype(vtype)).cuda())
        return auction_solve_ell_batch, args, dict(rows=fx["rows"], n_cols=fx["M"])
    packed, sizes = packed_form(K, outside)
    loc, val, offsets = sparse_pack(packed)
    if leg == "view":
        idx = torch.full((loc.shape[0], 3), -7, dtype=torch.int64, device="cuda")
        idx[:, 1:] = torch.from_numpy(loc.astype(np.int64)).cuda()
        d_loc, d_val = idx[:, 1:], torch.from_numpy(val.astype(np.float32)).cuda()
        assert not d_loc.is_contiguous() and d_loc.stride() == (3, 1)
    else:
        d_loc, d_val = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda()
    return auction_solve_sparse_batch, (d_loc, d_val, offsets), dict(sizes=sizes, dims=(N, fx["M"]))


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("mode", ["status", "outside"])
def test_every_accessor_returns_the_same_bits(mode, problem, K):
    import torch
    outside = mode == "outside"
    fx = batch(K, outside)
    got = {}
    for leg in LEGS:
        solve, args, kw = _leg(leg, K, outside)
        if outside:
            kw["outside"] = torch.from_numpy(fx["out"].copy()).cuda()
        got[leg] = outputs(solve(*args, problem=problem, errors="status", cardinality_check=True, max_iter=MAX_ITER, **kw))
    first = got[LEGS[0]]
    n = fx["rows"]
    for leg in LEGS:  # every problem is clean for every front end, and solved
        assert (got[leg]["status"] == 0).all(), (leg, got[leg]["status"])
    assert np.array_equal(first["matching_size"], np.full(len(n), -1) if outside else n)  # the guard ran, or there is none
    assert ("outside_prices" in first) == outside
    assert np.array_equal(first["meta.n_rows"], n) and (first["meta.soln_found"] == 1).all()
    assert (first["meta.its"] > 0).all() and (first["meta.its"] < MAX_ITER).all()
    assert K < 2 or sum(rewalked(fx["c"][0][b], first["sol"][b]) for b in range(len(n))) > 0
    for leg in LEGS[1:]:
        assert got[leg].keys() == first.keys()
        for k, v in first.items():
            assert v.dtype == got[leg][k].dtype and np.array_equal(v, got[leg][k]), (leg, k)
