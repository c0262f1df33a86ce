"""auction_solve_batch on the GPU (misslap_solve_dense_batch: one workgroup per problem, one solve launch) against the
oracle on every slice: the reference's _from_matrix(mats[b, :n_b, :m_b]).solve(), bit for bit -- sol, its,
nreductions, eCE, soln_found, n_assigned, obj, obj_f64, the fp32 start / final eps and the price bits."""
import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import auction_solve_batch, from_matrix
from tests._batch_shapes import bits as _bits, dense_compare, dense_expect, dense_values as _values

pytestmark = pytest.mark.gpu


def _oracle(mat, problem, eps_start=0.0, max_iter=1000000, fast=False, p0=None):
    o = orc.from_matrix(mat, problem=problem, eps_start=eps_start, max_iter=max_iter, fast=fast)
    if p0 is not None:  # the reference's solve() with self.p starting at p0 instead of zeros (auction_.pyx:220)
        np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))[:] = p0[:o.M]
    sol = o.solve()
    return sol, o


def _check_problem(res, b, mat, problem, n, m, p0=None, **kw):
    """Problem b of a result against the oracle on its slice: every field of tests/_batch_shapes.dense_compare."""
    dense_compare(res, b, dense_expect(mat, problem, p0=p0, **kw), n, m, p0=p0)


def _check_all(res, mats, problem, shapes=None, prices=None, **kw):
    B, N, M = mats.shape
    for b in range(B):
        n, m = (N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1]))
        _check_problem(res, b, mats[b, :n, :m], problem, n, m, p0=None if prices is None else prices[b], **kw)


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("kind", ["uniform", "ints", "fp32", "holes"])
def test_value_kinds(problem, kind):
    rng = np.random.default_rng(hash((problem, kind)) % 2**32)
    mats = _values(kind, (6, 24, 31), rng)
    before = mats.copy()
    res = auction_solve_batch(mats, problem=problem, cardinality_check=(kind == "holes"))
    assert np.array_equal(_bits(mats), _bits(before))  # the caller's array is never written, 'min' included
    _check_all(res, mats, problem)


@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(fast=True), dict(max_iter=1), dict(max_iter=7),
                                  dict(max_iter=7, problem="max"), dict(max_iter=0)])
def test_eps_and_max_iter(opts):
    rng = np.random.default_rng(7)
    mats = _values("uniform", (5, 40, 40), rng)
    opts = dict(opts)
    problem = opts.pop("problem", "min")
    res = auction_solve_batch(mats, problem=problem, **opts)
    _check_all(res, mats, problem, **opts)
    if opts.get("max_iter") == 1:
        assert (res["sol"] == -1).any()  # a stopped solve leaves persons unassigned


def test_trailing_invalid_columns_and_single_entry_rows():
    rng = np.random.default_rng(11)
    mats = _values("uniform", (4, 12, 20), rng)
    mats[:, :, 15:] = -1  # trailing all-invalid columns: the problem's M is 15
    mats[1, 3, :] = -1
    mats[1, 3, 7] = 5.0  # a row with one valid entry: its bid, and the price, are +inf
    mats[2, :, :] = -1
    mats[2, np.arange(12), np.arange(12)] = rng.uniform(0, 100, 12)  # every row a single entry
    for problem in ("min", "max"):
        res = auction_solve_batch(mats, problem=problem)
        _check_all(res, mats, problem)
        assert np.isinf(res["prices"][1, 7]) and res["meta"]["n_cols"][0] == 15


def test_narrow_tiny_and_cap_shapes():
    rng = np.random.default_rng(3)
    for shape in [(3, 5, 37), (4, 1, 9), (2, 1, 1), (1, 1024, 1024)]:
        mats = _values("uniform" if shape[1] < 1024 else "ints", shape, rng)
        res = auction_solve_batch(mats, problem="max", cardinality_check=False)
        _check_all(res, mats, "max")


def test_mixed_shapes_never_read_the_padding():
    rng = np.random.default_rng(5)
    B, N, M = 9, 30, 40
    shapes = np.stack([rng.integers(1, N + 1, B), rng.integers(1, M + 1, B)], axis=1)
    shapes[:, 1] = np.maximum(shapes[:, 1], shapes[:, 0])
    mats = np.full((B, N, M), np.inf)  # +inf would be rejected if it were read
    for b, (n, m) in enumerate(shapes):
        mats[b, :n, :m] = _values("holes" if b % 3 == 0 else "uniform", (n, m), rng)
    for problem in ("min", "max"):
        res = auction_solve_batch(mats, problem=problem, shapes=shapes)
        _check_all(res, mats, problem, shapes=shapes)


def test_starting_prices():
    rng = np.random.default_rng(9)
    mats = _values("uniform", (6, 25, 30), rng)
    p0 = rng.uniform(0, 20, (6, 30))
    p0[1] = 0.0
    p0[2, ::3] = 0.0
    for problem in ("min", "max"):
        for eps_start in (0.0, 0.25):
            res = auction_solve_batch(mats, problem=problem, prices=p0, eps_start=eps_start)
            _check_all(res, mats, problem, prices=p0, eps_start=eps_start)


def test_more_problems_than_compute_units():
    rng = np.random.default_rng(13)
    B = 2048
    shapes = np.stack([rng.integers(2, 17, B), np.full(B, 16)], axis=1)
    mats = np.where(rng.random((B, 16, 16)) < 0.9, rng.uniform(0, 100, (B, 16, 16)), -1.0)
    mats[:, np.arange(16), np.arange(16)] = 1.0
    res = auction_solve_batch(mats, problem="min", shapes=shapes)
    _check_all(res, mats, "min", shapes=shapes)


def test_stack_larger_than_2_31_bytes():
    rng = np.random.default_rng(17)
    one = rng.integers(0, 1000, (1024, 1024)).astype(np.float64)
    B = (1 << 31) // one.nbytes + 1
    mats = np.empty((B, 1024, 1024))
    mats[:] = one
    assert mats.nbytes > 1 << 31
    res = auction_solve_batch(mats, problem="max", cardinality_check=False)
    del mats
    sol_o, o = _oracle(one, "max")
    p_o = _bits(o.state()["p"])
    for b in range(B):
        assert np.array_equal(res["sol"][b], sol_o), b
        assert np.array_equal(_bits(res["prices"][b]), p_o), b
        assert res["meta"]["its"][b] == o.meta["its"] and res["meta"]["obj_f64"][b] == o.extra["obj_f64"], b


def test_equal_to_gpu_from_matrix():
    rng = np.random.default_rng(19)
    mats = _values("holes", (4, 50, 60), rng)
    for problem in ("min", "max"):
        res = auction_solve_batch(mats, problem=problem)
        for b in range(4):
            s = from_matrix(mats[b].copy(), problem=problem)
            sol = s.solve()
            assert np.array_equal(res["sol"][b], sol)
            for k in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "start_eps", "final_eps"):
                assert res["meta"][k][b] == s.meta[k], k
            assert res["meta"]["obj_f64"][b] == s.gpu["obj_f64"]
            assert np.array_equal(_bits(res["prices"][b, :s.num_cols]), _bits(s.prices))


def _from_matrix_error(mat, prices=None):
    with pytest.raises(ValueError) as e:
        s = from_matrix(mat.copy())
        if prices is not None:
            s.resolve(prices=prices[:s.num_cols])
    return str(e.value)


def test_errors_name_the_problem_and_solve_nothing():
    rng = np.random.default_rng(23)
    good = rng.uniform(0, 100, (5, 4, 4))
    cases = []
    m = good.copy()
    m[2] = -1
    m[2, 0, :2] = 1.0  # fewer valid values than rows
    cases.append((m, 2, None))
    m = good.copy()
    m[3, 1, :] = np.nan  # an empty row
    cases.append((m, 3, None))
    m = good.copy()
    m[1, 2, 2] = np.inf
    cases.append((m, 1, None))
    m = good.copy()
    m[4, :3, 1:] = -1  # rows 0..2 only reach column 0: a matching of 2 out of 4
    cases.append((m, 4, None))
    m = good.copy()
    m[3, 1, :] = -1
    m[4, :3, 1:] = -1  # the first failing problem is reported
    cases.append((m, 3, None))
    for bad in (np.nan, -1.0, -0.0, np.inf):
        p = np.zeros((5, 4))
        p[2, 1] = bad
        cases.append((good.copy(), 2, p))
    for mats, b, prices in cases:
        want = _from_matrix_error(mats[b], None if prices is None else prices[b])
        with pytest.raises(ValueError) as e:
            auction_solve_batch(mats, prices=prices)
        assert str(e.value) == f"problem {b}: {want}"
        res = auction_solve_batch(good)  # the next call works
        _check_all(res, good, "min")


def test_device_tensor_written_on_a_side_stream():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(29)
    host = _values("holes", (16, 48, 48), rng)
    p0 = rng.uniform(0, 5, (16, 48))
    want = auction_solve_batch(host, problem="min", prices=p0)
    src = torch.from_numpy(host).cuda()
    side = torch.cuda.Stream()
    x = torch.full_like(src, -1.0)
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)  # the copy below lands long after the call was made
        x.copy_(src)
        pd = torch.from_numpy(p0).cuda()
        got = auction_solve_batch(x, problem="min", prices=pd)
    torch.cuda.synchronize()
    assert got["sol"].is_cuda and got["prices"].is_cuda and got["sol"].device == x.device
    assert np.array_equal(got["sol"].cpu().numpy(), want["sol"])
    assert np.array_equal(_bits(got["prices"].cpu().numpy()), _bits(want["prices"]))
    for k in ("its", "nreductions", "obj_f64", "final_eps_f32"):
        assert np.array_equal(got["meta"][k], want["meta"][k]), k
    assert torch.equal(x.view(torch.int64), src.view(torch.int64))  # read in place, not written (NaNs compared by bits)
