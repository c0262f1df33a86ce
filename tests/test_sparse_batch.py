"""auction_solve_sparse_batch on the GPU (misslap_solve_sparse_batch: one workgroup per problem, one solve launch) against
the real reference's golden vectors, against the oracle on every problem -- the reference's
_from_sparse(loc_b, val_b, size=...).solve(), bit for bit: sol, its, nreductions, eCE, soln_found, n_assigned, obj,
obj_f64, the fp32 start / final eps and the price bits -- and against GPU from_sparse."""
import numpy as np
import pytest

import cases
from sslap_amd import auction_solve_sparse_batch, from_sparse
from tests._batch_shapes import (bits as _bits, sparse_compare, sparse_expect, sparse_pack as _pack,
                                 sparse_problem as _problem)

pytestmark = pytest.mark.gpu

CAP = 2048


def _check_problem(res, b, loc, val, problem, size=None, p0=None, **kw):
    """Problem b of a result against the oracle on its loc / val: every field of tests/_batch_shapes.sparse_compare."""
    sparse_compare(res, b, sparse_expect(loc, val, problem, size=size, p0=p0, **kw))


def _check_all(res, probs, problem, sizes=None, prices=None, **kw):
    for b, (loc, val) in enumerate(probs):
        _check_problem(res, b, loc, val, problem, size=None if sizes is None else tuple(int(x) for x in sizes[b]),
                       p0=None if prices is None else prices[b], **kw)


def _solve(probs, **kw):
    loc, val, offsets = _pack(probs)
    before = (loc.copy(), val.copy())
    res = auction_solve_sparse_batch(loc, val, offsets, **kw)
    assert np.array_equal(loc, before[0]) and np.array_equal(_bits(val), _bits(before[1]))  # never written, 'min' too
    return res


# ---- the real reference: every loc/val, loc/val + size and coo golden case within the cap, batched by options
def _golden_batch_groups():
    groups = {}
    for name, (spec, kw, entry) in sorted(cases.SMALL_CASES.items()):
        if entry not in ("locval", "locval_size", "coo"):
            continue
        n, m = spec["n"], spec.get("m", spec["n"])
        if max(n, m) > CAP:
            continue
        groups.setdefault(tuple(sorted(kw.items())), []).append((name, spec, entry))
    return groups


@pytest.mark.parametrize("key", sorted(_golden_batch_groups(), key=repr), ids=repr)
def test_golden_cases_match_reference(key, golden_small):
    manifest, arrays = golden_small
    members = _golden_batch_groups()[key]
    kw = dict(key)
    probs, sizes = [], []
    for name, spec, entry in members:
        loc, val = cases.synth_inputs(spec)
        n, m = spec["n"], spec.get("m", spec["n"])
        probs.append((loc, val))
        # from_sparse reads size as (M, N) and N only enters the entry count and `fast`; without size, N = max row
        sizes.append((n, m) if entry != "locval" else (m, int(loc[:, 0].max())))
    res = _solve(probs, sizes=np.array(sizes), **kw)
    for b, (name, spec, entry) in enumerate(members):
        g = manifest["cases"][name]
        n = spec["n"]
        assert np.array_equal(res["sol"][b, :n], arrays[name + "/sol"]), name
        for k in cases.META_KEYS:
            assert res["meta"][k][b] == g["meta"][k], (name, k)
        assert res["meta"]["obj_f64"][b] == g["obj_f64"], name
    assert len(members) >= 1


def test_golden_over_cap_case_is_rejected(golden_small):
    spec, kw, _ = cases.SMALL_CASES["sq3000_int20"]
    big = cases.synth_inputs(spec)
    small = cases.synth_inputs(cases.SMALL_CASES["sq64_max"][0])
    with pytest.raises(ValueError) as e:
        _solve([small, big], **kw)
    assert str(e.value) == ("problem 1: 3000 x 3000 exceeds MISSLAP_SPARSE_BATCH_MAX_DIM (2048); solve it with "
                            "from_sparse / solve_batch")


# ---- value kinds, options
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("kind", ["uniform", "ints", "fp32"])
def test_value_kinds(problem, kind):
    rng = np.random.default_rng(hash((problem, kind)) % 2**32)
    probs = [_problem(rng, int(rng.integers(5, 40)), 45, 6, kind) for _ in range(8)]
    res = _solve(probs, problem=problem)
    _check_all(res, probs, problem)


@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(fast=True), dict(max_iter=0), dict(max_iter=1),
                                  dict(max_iter=7), dict(max_iter=7, problem="max")])
def test_eps_fast_and_max_iter(opts):
    rng = np.random.default_rng(7)
    probs = [_problem(rng, 40, 50, 8) for _ in range(5)]
    opts = dict(opts)
    problem = opts.pop("problem", "min")
    res = _solve(probs, problem=problem, **opts)
    _check_all(res, probs, problem, **opts)
    if opts.get("max_iter") == 1:
        assert (res["sol"] == -1).any()  # a stopped solve leaves persons unassigned


def test_fast_with_sizes():
    rng = np.random.default_rng(8)
    probs = [_problem(rng, 30, 40, 5) for _ in range(4)]
    sizes = np.array([[40, 30], [40, 17], [3, 30], [40, 12]])
    res = _solve(probs, problem="max", fast=True, sizes=sizes)
    _check_all(res, probs, "max", sizes=sizes, fast=True)


# ---- row patterns
def test_row_patterns():
    rng = np.random.default_rng(11)
    probs = []
    probs.append(_problem(rng, 30, 30, 10, shuffle=True))   # shuffled column order
    probs.append(_problem(rng, 30, 30, 10, shuffle=False))  # column-sorted rows
    loc, val = _problem(rng, 30, 30, 8, "ints")
    dup = rng.random(loc.shape[0]) < 0.3  # duplicate (i, j) entries, with other values, at the end of their row
    loc2 = np.concatenate([loc, loc[dup]])
    val2 = np.concatenate([val, val[dup] + rng.integers(-1, 2, int(dup.sum()))])
    order = np.argsort(loc2[:, 0], kind="stable")
    probs.append((np.ascontiguousarray(loc2[order]), np.ascontiguousarray(np.abs(val2[order]))))
    loc, val = _problem(rng, 20, 20, 1)  # one entry per row: +inf bids and prices
    probs.append((loc, val))
    loc, val = _problem(rng, 20, 25, 6)  # rows 5..24 of 6 entries; rows 0..4 a single entry each, in columns of their own
    single = np.stack([np.arange(5), 25 + np.arange(5)], axis=1).astype(np.int32)
    probs.append((np.ascontiguousarray(np.concatenate([single, loc + np.array([5, 0], dtype=np.int32)])),
                  np.concatenate([rng.uniform(0, 100, 5), val])))
    probs.append(_problem(rng, 12, 300, 200))    # rows longer than 64 entries
    probs.append(_problem(rng, 6, 1500, 1300))   # rows longer than 1024 entries
    probs.append(_problem(rng, 10, 90, 30))      # rectangular n < m
    for problem in ("min", "max"):
        res = _solve(probs, problem=problem)
        _check_all(res, probs, problem)
    assert np.isinf(res["prices"][3]).any()


def test_duplicates_count_in_the_objective():
    loc = np.array([[0, 0], [0, 1], [0, 0], [1, 1], [1, 0]], dtype=np.int32)
    val = np.array([5.0, 1.0, 7.0, 2.0, 1.0])
    res = _solve([(loc, val)], problem="max")
    _check_all(res, [(loc, val)], "max")
    assert res["sol"][0].tolist() == [0, 1] and res["meta"]["obj_f64"][0] == 14.0


# ---- sizes, many problems, starting prices
def test_mixed_sizes_up_to_the_cap():
    rng = np.random.default_rng(5)
    probs = [(np.array([[0, 0]], dtype=np.int32), np.array([3.0]))]
    for n, m, k in [(1, 7, 3), (3, 3, 3), (64, 64, 8), (200, 257, 12), (700, 1000, 5), (CAP, CAP, 16), (CAP - 1, CAP, 4)]:
        probs.append(_problem(rng, n, m, k))
    res = _solve(probs, problem="max", cardinality_check=False)
    _check_all(res, probs, "max")
    assert res["sol"].shape == (len(probs), CAP) and res["prices"].shape == (len(probs), CAP)


def test_more_problems_than_compute_units():
    rng = np.random.default_rng(13)
    probs = [_problem(rng, int(rng.integers(1, 17)), 16, 6, "ints") for _ in range(2048)]
    res = _solve(probs, problem="min")
    _check_all(res, probs, "min")


def test_starting_prices():
    rng = np.random.default_rng(9)
    probs = [_problem(rng, 25, 30, 7) for _ in range(6)]
    p0 = rng.uniform(0, 20, (6, 34))
    p0[1] = 0.0
    p0[2, ::3] = 0.0
    for problem in ("min", "max"):
        for eps_start in (0.0, 0.25):
            res = _solve(probs, problem=problem, prices=p0, eps_start=eps_start)
            _check_all(res, probs, problem, prices=p0, eps_start=eps_start)


def test_equal_to_gpu_from_sparse():
    rng = np.random.default_rng(19)
    probs = [_problem(rng, 50, 60, 9, "ints") for _ in range(4)]
    for problem in ("min", "max"):
        res = _solve(probs, problem=problem)
        for b, (loc, val) in enumerate(probs):
            s = from_sparse(loc, val.copy(), problem=problem)
            sol = s.solve()
            assert np.array_equal(res["sol"][b, :50], sol)
            for k in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "start_eps", "final_eps"):
                assert res["meta"][k][b] == s.meta[k], k
            assert res["meta"]["obj_f64"][b] == s.gpu["obj_f64"]
            assert np.array_equal(_bits(res["prices"][b, :s.num_cols]), _bits(s.prices))


# ---- errors: all or nothing, the first failing problem, from_sparse's text
def _from_sparse_error(loc, val, size=None, cardinality_check=True, prices=None):
    with pytest.raises(ValueError) as e:
        s = from_sparse(loc.copy(), val.copy(), size=size, cardinality_check=cardinality_check)
        if prices is not None:
            s.resolve(prices=prices[:s.num_cols])
    return str(e.value)


def _good(rng):
    return [_problem(rng, 6, 8, 3) for _ in range(5)]


def _expect_error(probs, b, want, **kw):
    loc, val, offsets = _pack(probs)
    before = (loc.copy(), val.copy())
    with pytest.raises(ValueError) as e:
        auction_solve_sparse_batch(loc, val, offsets, **kw)
    assert str(e.value) == f"problem {b}: {want}"
    assert np.array_equal(loc, before[0]) and np.array_equal(_bits(val), _bits(before[1]))


def _with(rng, b, fn):
    probs = _good(rng)
    loc, val = probs[b][0].copy(), probs[b][1].copy()
    probs[b] = fn(loc, val)
    return probs


@pytest.mark.parametrize("guard", [True, False])
def test_error_fewer_entries_than_n(guard):
    rng = np.random.default_rng(23)
    probs = _good(rng)
    sizes = np.array([[8, 6]] * 5)
    sizes[3] = (8, probs[3][0].shape[0] + 1)
    _expect_error(probs, 3, _from_sparse_error(*probs[3], size=tuple(sizes[3]), cardinality_check=guard), sizes=sizes,
                  cardinality_check=guard)


@pytest.mark.parametrize("guard", [True, False])
def test_error_negative_index(guard):
    rng = np.random.default_rng(24)

    def neg(loc, val):
        loc[4, 1] = -2
        return loc, val
    probs = _with(rng, 2, neg)
    _expect_error(probs, 2, _from_sparse_error(*probs[2], cardinality_check=guard), cardinality_check=guard)


def test_error_matching_guard():
    rng = np.random.default_rng(25)

    def narrow(loc, val):
        loc[loc[:, 0] < 4, 1] = 0  # rows 0..3 only reach column 0
        return loc, val
    probs = _with(rng, 4, narrow)
    want = _from_sparse_error(*probs[4])
    assert "Maximum matching" in want
    _expect_error(probs, 4, want)
    res = auction_solve_sparse_batch(*_pack(probs), cardinality_check=False)  # without the guard it is solved
    _check_all(res, probs, "min")


@pytest.mark.parametrize("guard", [True, False])
def test_error_row_gap(guard):
    rng = np.random.default_rng(26)

    def gap(loc, val):
        keep = loc[:, 0] != 2
        return np.ascontiguousarray(loc[keep]), np.ascontiguousarray(val[keep])
    probs = _with(rng, 1, gap)
    want = _from_sparse_error(*probs[1], cardinality_check=guard)
    assert ("Maximum matching" in want) == guard  # the guard speaks first, as in from_sparse
    _expect_error(probs, 1, want, cardinality_check=guard)


@pytest.mark.parametrize("guard", [True, False])
def test_error_rows_not_ascending(guard):
    rng = np.random.default_rng(27)

    def unsorted(loc, val):
        loc[[0, 5]] = loc[[5, 0]]
        return loc, val
    probs = _with(rng, 0, unsorted)
    _expect_error(probs, 0, _from_sparse_error(*probs[0], cardinality_check=guard), cardinality_check=guard)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_error_non_finite_value(bad):
    rng = np.random.default_rng(28)

    def nonfinite(loc, val):
        val[3] = bad
        return loc, val
    probs = _with(rng, 3, nonfinite)
    _expect_error(probs, 3, _from_sparse_error(*probs[3]))


def test_error_over_the_cap():
    rng = np.random.default_rng(29)
    probs = _good(rng)
    probs[2] = (np.array([[0, 0], [0, CAP]], dtype=np.int32), np.array([1.0, 2.0]))
    _expect_error(probs, 2, f"1 x {CAP + 1} exceeds MISSLAP_SPARSE_BATCH_MAX_DIM ({CAP}); solve it with "
                            "from_sparse / solve_batch")


@pytest.mark.parametrize("bad", [np.nan, -1.0, -0.0, np.inf])
def test_error_bad_starting_prices(bad):
    rng = np.random.default_rng(30)
    probs = _good(rng)
    p = np.zeros((5, 8))
    p[2, 1] = bad
    _expect_error(probs, 2, _from_sparse_error(*probs[2], prices=p[2]), prices=p)


def test_error_no_entries_and_first_failure_wins():
    rng = np.random.default_rng(31)
    probs = _good(rng)
    probs[3] = (np.zeros((0, 2), dtype=np.int32), np.zeros(0))
    _expect_error(probs, 3, "no entries")
    probs[1] = (probs[1][0], np.where(np.arange(probs[1][1].size) == 0, np.nan, probs[1][1]))
    _expect_error(probs, 1, "val holds a NaN or an infinity")
    good = _good(rng)
    res = _solve(good)  # the next call works
    _check_all(res, good, "min")


def test_error_fast_with_n_zero():
    rng = np.random.default_rng(32)
    probs = _good(rng)
    probs[2] = (np.array([[0, 0], [0, 1]], dtype=np.int32), np.array([1.0, 2.0]))  # one row: from_sparse's N = 0
    with pytest.raises(ZeroDivisionError):
        from_sparse(probs[2][0], probs[2][1].copy(), fast=True)
    with pytest.raises(ZeroDivisionError, match="problem 2"):
        auction_solve_sparse_batch(*_pack(probs), fast=True)


# ---- device input, list input
def test_device_tensors_written_on_a_side_stream():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(33)
    probs = [_problem(rng, int(rng.integers(10, 48)), 48, 7) for _ in range(16)]
    loc, val, offsets = _pack(probs)
    p0 = rng.uniform(0, 5, (16, 48))
    want = auction_solve_sparse_batch(loc, val, offsets, problem="min", prices=p0)
    lsrc, vsrc = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda()
    side = torch.cuda.Stream()
    lx, vx = torch.full_like(lsrc, -1), torch.full_like(vsrc, -1.0)
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)  # the copies below land long after the call was made
        lx.copy_(lsrc)
        vx.copy_(vsrc)
        pd = torch.from_numpy(p0).cuda()
        got = auction_solve_sparse_batch(lx, vx, offsets, problem="min", prices=pd)
    torch.cuda.synchronize()
    assert got["sol"].is_cuda and got["prices"].is_cuda and got["sol"].device == lx.device
    assert np.array_equal(got["sol"].cpu().numpy(), want["sol"])
    assert np.array_equal(_bits(got["prices"].cpu().numpy()), _bits(want["prices"]))
    for k in ("its", "nreductions", "obj_f64", "final_eps_f32"):
        assert np.array_equal(got["meta"][k], want["meta"][k]), k
    assert torch.equal(lx, lsrc) and torch.equal(vx, vsrc)  # read in place, not written
    _check_all(want, probs, "min", prices=p0)


def test_device_tensors_with_fast():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(34)
    probs = [_problem(rng, int(rng.integers(3, 30)), 30, 5) for _ in range(6)]
    loc, val, offsets = _pack(probs)
    want = auction_solve_sparse_batch(loc, val, offsets, problem="max", fast=True)
    got = auction_solve_sparse_batch(torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda(), offsets, problem="max",
                                     fast=True)
    assert np.array_equal(got["sol"].cpu().numpy(), want["sol"])
    assert np.array_equal(got["meta"]["start_eps_f32"], want["meta"]["start_eps_f32"])
    _check_all(want, probs, "max", fast=True)


def test_list_of_pairs_equals_packed_input():
    rng = np.random.default_rng(35)
    probs = [_problem(rng, int(rng.integers(2, 20)), 20, 4) for _ in range(7)]
    packed = auction_solve_sparse_batch(*_pack(probs), problem="max")
    listed = auction_solve_sparse_batch([(lo.astype(np.int64), v) for lo, v in probs], problem="max")
    assert np.array_equal(packed["sol"], listed["sol"])
    assert np.array_equal(_bits(packed["prices"]), _bits(listed["prices"]))
    for k in ("its", "nreductions", "obj_f64", "n_cols"):
        assert np.array_equal(packed["meta"][k], listed["meta"][k]), k
