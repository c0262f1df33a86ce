"""auction_solve_ell_batch(outside=) on the GPU (misslap_solve_ell_batch_outside): an outside option per row, so that a
row may stay unmatched.

  parity        every problem is the oracle's result bit for bit on ell_to_packed(..., outside=)'s (loc_b, val_b) with
                size=(m_b + n_b, n_b), given in the caller's terms (a column >= m_b is -1, the prices split into the real
                and the outside ones) -- at the lane edges of the virtual entry (K = 1 .. 128), with ties between an entry
                and the outside entry, rows without entries, shapes the plain call cannot take (n_b > m_b, holes only),
                at the workgroup-size steps and at the largest carve, for every form of `outside`, every pair of index
                and value type, eps_start, max_iter and starting prices -- from numpy arrays and from device tensors.
  cross-layout  the plain call on the explicitly augmented (B, N, K + 1) stack: identical outputs after the mapping.
  verdicts      a mixed batch: the statuses derived here on the CPU, healthy problems equal the oracle, condemned ones
                have exactly the defined outputs; the default mode raises.
  safety        device inputs are slices of poisoned buffers and are never written.
  no wait       with n_cols and a device `outside`, behind >= 200 ms of queued work the call returns at once.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import auction_solve_ell_batch, ell_to_packed
from tests import _ell_fixture as fxt
from tests._batch_shapes import META_KEYS, bits, sparse_expect, sparse_problem, sparse_problem_distinct, threads_for
from tests.test_ell_batch import ZERO_META, _busy, _device, _to_host, _typed

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _sizes(cols, rows):
    """[(m_b, n_b)]: the real columns (max + 1, 0 without an entry) and the rows of every problem."""
    out = []
    for b in range(cols.shape[0]):
        n = cols.shape[1] if rows is None else int(rows[b])
        c = cols[b, :n]
        out.append((int(c.max()) + 1 if (c >= 0).any() else 0, n))
    return out


def expect(cols, vals, rows, outside, problem, p0=None, **opts):
    """The oracle on the definition: [(want, m_b, n_b)].  vals: already in the call's value type."""
    packed = ell_to_packed(cols, vals, rows, outside=outside)
    out = []
    for b, ((loc, val), (m, n)) in enumerate(zip(packed, _sizes(cols, rows))):
        assert loc.shape[0] == int((cols[b, :n] >= 0).sum()) + n and np.isfinite(val).all()
        start = None if p0 is None else np.concatenate([p0[b, :m], np.zeros(n)])
        out.append((sparse_expect(loc, val, problem, size=(m + n, n), p0=start, **opts), m, n))
    return out


def compare(res, b, want, m, n):
    """Problem b of an outside result against the oracle's result on the augmented problem."""
    meta = res["meta"]
    sol, ws = res["sol"][b], want["sol"]
    assert np.array_equal(sol[:n], np.where(ws >= m, -1, ws)), b
    assert (ws[ws >= m] == np.flatnonzero(ws >= m) + m).all()  # (an outside object is its own row's)
    assert (sol[n:] == -1).all(), b
    for k in META_KEYS:
        assert meta[k][b] == want["meta"][k], (b, k, meta[k][b], want["meta"][k])
    assert meta["obj_f64"][b] == want["extra"]["obj_f64"], b
    assert meta["bids_made"][b] == want["extra"]["bids_made"], b
    for k in ("start_eps_f32", "final_eps_f32"):
        assert np.float32(meta[k][b]).view(np.uint32) == np.float32(want["extra"][k]).view(np.uint32), (b, k)
    assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (n, m + n, want["nnz"]), b
    assert want["N"] == n and want["M"] == m + n
    p, op = res["prices"][b], res["outside_prices"][b]
    assert p.dtype == np.float64 and op.dtype == np.float64
    assert np.array_equal(bits(p[:m]), bits(want["p"][:m])), b
    assert np.array_equal(bits(p[m:]), bits(np.zeros(len(p) - m))), b
    assert np.array_equal(bits(op[:n]), bits(want["p"][m:])), b
    assert np.array_equal(bits(op[n:]), bits(np.zeros(len(op) - n))), b


def _host(res):
    if isinstance(res["sol"], np.ndarray):
        return res
    assert res["outside_prices"].is_cuda and res["outside_prices"].device == res["sol"].device
    return dict(_to_host(res), outside_prices=res["outside_prices"].cpu().numpy())


def _device_outside(outside, pad=512):
    """outside on the device: an array as a slice of a larger buffer of NaN, a float as it is."""
    import torch
    if not isinstance(outside, np.ndarray):
        return outside
    buf = np.full(outside.size + 2 * pad, np.nan)
    buf[pad:pad + outside.size] = outside.ravel()
    return torch.from_numpy(buf).cuda()[pad:pad + outside.size].view(outside.shape)


def both(cols, vals, rows=None, outside=None, prices=None, on_device=False, n_cols=None, **kw):
    """The same batch from numpy arrays, and from device tensors that are slices of poisoned buffers; rows, prices and
    outside stay on the host (they travel pinned) or, with on_device, are device tensors too.  Nothing is written."""
    import torch
    before = (cols.copy(), vals.copy(), None if not isinstance(outside, np.ndarray) else outside.copy())
    yield auction_solve_ell_batch(cols, vals, rows=rows, prices=prices, n_cols=n_cols, outside=outside, errors="status", **kw)
    assert np.array_equal(cols, before[0]) and np.array_equal(vals.view(np.uint8), before[1].view(np.uint8))
    dc, dv = _device(cols, vals)
    do = _device_outside(outside) if on_device else outside
    dp = prices if prices is None or not on_device else torch.from_numpy(np.array(prices)).cuda()
    dr = rows if rows is None or not on_device else torch.from_numpy(np.array(rows)).cuda()
    res = auction_solve_ell_batch(dc, dv, rows=dr, prices=dp, n_cols=n_cols, outside=do, errors="status", **kw)
    for k in ("sol", "prices", "outside_prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == dc.device, k
    yield _host(res)
    assert np.array_equal(dc.cpu().numpy(), cols)  # never written
    assert np.array_equal(dv.cpu().numpy().view(np.uint8), vals.view(np.uint8))
    if on_device and isinstance(outside, np.ndarray):
        assert np.array_equal(bits(do.cpu().numpy()), bits(before[2]))


def check(cols64, vals64, rows, outside, problem="min", dtypes=fxt.DTYPES[:2], prices=None, n_cols=None, opts=(),
          want_cache=None):
    """Both routes for each pair of types against the oracle; returns the last host result."""
    B, N, K = cols64.shape
    opts = dict(opts)
    res = None
    for k, (itype, vtype) in enumerate(dtypes):
        cols, vals = _typed(cols64, vals64, itype, vtype)
        key = (np.dtype(vtype).name, problem)
        if want_cache is None or key not in want_cache:
            want = expect(cols64, vals, rows, outside, problem, p0=prices, **_oracle_opts(opts))
            if want_cache is not None:
                want_cache[key] = want
        else:
            want = want_cache[key]
        for res in both(cols, vals, rows=rows, outside=outside, prices=prices, on_device=bool(k % 2), n_cols=n_cols,
                        problem=problem, **opts):
            assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
            assert (res["matching_size"] == -1).all()  # no guard in this mode
            assert res["sol"].shape == (B, N) and res["outside_prices"].shape == (B, N)
            assert res["prices"].shape == (B, n_cols or min(max(int(cols64.max()) + 1, 1), fxt.CAP))
            assert res["meta"]["gpu"]["threads"] == threads_for(N)
            for b, (w, m, n) in enumerate(want):
                compare(res, b, w, m, n)
    return res, want


def _oracle_opts(opts):
    """The front end's resolution of `fast`, for the oracle: a single phase unless eps_start > 0 was given."""
    o = dict(opts)
    o.pop("cardinality_check", None)
    if o.get("fast") is None:
        o["fast"] = not o.get("eps_start", 0.0) > 0
    return o


def _some_of_each(want):
    """Whether, over the problems, some rows took a real column and some their outside option."""
    out = np.concatenate([w["sol"] >= m for w, m, _ in want])
    return out.any() and (~out).any()


# ---- the lane edges of the virtual entry

@functools.lru_cache(maxsize=None)
def _ladder(K, N=40):
    """Three problems at K slots, about a quarter of the slots holes: distinct uniform columns; `ints` values with an
    integer outside value (ties between an entry and the outside entry) and repeated columns; a short one (n = 33).
    Rows 5 of the first and 0 of the second have no entry; beyond n_b cols / vals / outside hold INT_MAX / +inf / NaN."""
    rng = np.random.default_rng([41, K])
    k = 1 if K <= 2 else K * 3 // 4
    m = max(N, K) + 7
    probs = [fxt.widen(*sparse_problem_distinct(rng, N, m, k, "uniform"), N, K, rng),
             fxt.widen(*sparse_problem(rng, N, m, k, "ints"), N, K, rng),
             fxt.widen(*sparse_problem(rng, N - 7, m + 30, k, "uniform"), N - 7, K, rng)]
    probs[0][0][5] = -1
    if K == 1:  # (a hole is then a row without an entry: every fourth row of the first problem)
        probs[0][0][1::4] = -1
    probs[1][0][0] = -2
    cols, vals, rows = fxt.stack(probs, N, K, fill_col=fxt.INT_MAX, fill_val=np.inf)
    outside = np.full((3, N), np.nan)
    outside[0] = rng.uniform(0, 100, N)
    outside[1] = rng.integers(0, 5, N)
    outside[2, :N - 7] = rng.uniform(20, 80, N - 7)
    return _frozen(cols, vals, rows, outside)


_LADDER_WANT = {}


@pytest.mark.parametrize("mode", ["single", "scaled"])
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128])
def test_parity_at_the_lane_edges(K, problem, mode):
    cols, vals, rows, outside = _ladder(K)
    assert list(rows) == [40, 40, 33] and not (cols[0, 5] >= 0).any() and not (cols[1, 0] >= 0).any()
    holes = np.mean([(cols[b, :rows[b]] < 0).mean() for b in range(3)])
    assert 0.15 < holes < 0.55 if K > 1 else (cols[0, :, 0] < 0).mean() >= 0.25, holes
    opts = dict(fast=True) if mode == "single" else dict(fast=False, eps_start=0.0)
    _, want = check(cols, vals, rows, outside, problem, opts=opts, want_cache=_LADDER_WANT.setdefault((K, mode), {}))
    if mode == "single":
        assert want[0][0]["meta"]["eCE"] == 1  # (distinct columns; with a repeated column the reference's own eCE test
        # takes the LAST stored value of the chosen column and may fail, as in the plain call)
    else:
        assert max(w["meta"]["nreductions"] for w, _, _ in want) >= 2  # several phases
    assert _some_of_each(want)
    w, m, _ = want[1]  # a tie between an entry and the outside entry, in a row that took either
    v = np.where(cols[1] >= 0, vals[1], np.nan)
    assert (v == outside[1][:, None]).any()
    assert np.isinf(w["p"][m + 0])  # the row without an entry: a one-entry row, whose bid is +inf


# ---- shapes the plain call cannot take

@functools.lru_cache(maxsize=None)
def _illegal():
    """n = 40 with m = 7, n = 3 with m = 1, and a problem of holes only with n = 1 and with n = 5, in one stack."""
    rng = np.random.default_rng(42)
    N, K = 40, 5
    cols = rng.choice(np.array(fxt.HOLE_COLS), (4, N, K)).astype(np.int64)
    vals = rng.choice(np.array(fxt.HOLE_VALS), (4, N, K))
    at = rng.random((N, K)) < 0.6
    cols[0][at] = rng.integers(0, 7, at.sum())
    cols[0, 0, 0] = 6
    vals[0][at] = rng.uniform(0, 100, at.sum())
    vals[0, 0, 0] = 50.0
    cols[1, :3, 2] = 0
    vals[1, :3, 2] = (3.0, 1.0, 2.0)
    rows = np.array([40, 3, 1, 5], dtype=np.int32)
    outside = rng.uniform(30, 70, (4, N))
    return _frozen(cols, vals, rows, outside)


@pytest.mark.parametrize("problem", ["min", "max"])
def test_shapes_that_were_illegal(problem):
    cols, vals, rows, outside = _illegal()
    assert _sizes(cols, rows) == [(7, 40), (1, 3), (0, 1), (0, 5)]
    res, want = check(cols, vals, rows, outside, problem, dtypes=fxt.DTYPES, n_cols=9)
    assert (res["sol"][2:] == -1).all() and list(res["meta"]["n_assigned"][2:]) == [1, 5]  # holes only: all outside
    assert (res["sol"][0] >= 0).sum() <= 7  # at most m rows hold a real column
    assert (res["sol"][1] >= 0).sum() == (1 if problem == "min" else 0)  # (costs 1 .. 3 against outside values 30 .. 70)
    assert _some_of_each(want[:1])
    # the plain call condemns every one of them
    plain = auction_solve_ell_batch(cols, vals, rows=rows, n_cols=9, errors="status")
    assert list(plain["status"]) == [fxt.EMPTY_ROW, fxt.INFEASIBLE, fxt.EMPTY_ROW, fxt.EMPTY_ROW]


# ---- the workgroup-size steps and the largest carve

@functools.lru_cache(maxsize=None)
def _tall(N, K=4):
    rng = np.random.default_rng([43, N])
    probs = [fxt.widen(*sparse_problem_distinct(rng, N, N, 3, "uniform"), N, K, rng),
             fxt.widen(*sparse_problem(rng, N - 1, N + 11, 3, "ints"), N - 1, K, rng)]
    cols, vals, rows = fxt.stack(probs, N, K)
    outside = np.stack([rng.uniform(0, 60, N), rng.integers(0, 5, N).astype(np.float64)])
    return _frozen(cols, vals, rows, outside)


@pytest.mark.parametrize("N", [256, 257, 513])
def test_parity_at_the_workgroup_size_steps(N):
    cols, vals, rows, outside = _tall(N)
    _, want = check(cols, vals, rows, outside, "min", dtypes=fxt.DTYPES[:1])
    check(cols, vals, rows, outside, "max", dtypes=fxt.DTYPES[1:2])
    assert _some_of_each(want)


def test_the_largest_carve():
    """B = 2 at N = 2048 and n_cols = 2048: 155 648 bytes of LDS for 2048 rows and 4096 objects."""
    rng = np.random.default_rng(44)
    N, K = fxt.CAP, 16
    cols = np.stack([np.stack([rng.choice(N, K, replace=False) for _ in range(N)]) for _ in range(2)]).astype(np.int64)
    cols[rng.random(cols.shape) < 0.25] = -1
    cols[0, 0, 0], cols[1, N - 1, K - 1] = N - 1, N - 1  # the last real column is in use
    vals = rng.uniform(0, 100, cols.shape)
    rows = np.array([N, N - 3], dtype=np.int32)
    outside = np.array([12.0, 20.0])
    res, want = check(cols, vals, rows, outside, "min", dtypes=fxt.DTYPES[1:2], n_cols=N)
    assert res["meta"]["gpu"]["lds_bytes"] == 24 * (2 * N) + 28 * N == 155648
    assert list(res["meta"]["n_cols"]) == [2 * N, 2 * N - 3] and _some_of_each(want)


# ---- the forms of `outside`

@functools.lru_cache(maxsize=None)
def _forms_stack():
    rng = np.random.default_rng(45)
    N, K = 20, 6
    probs = [fxt.widen(*sparse_problem(rng, n, 25, 4, kind), n, K, rng)
             for n, kind in ((20, "uniform"), (13, "ints"), (1, "uniform"), (17, "fp32"))]
    return _frozen(*fxt.stack(probs, N, K, fill_col=fxt.INT_MAX, fill_val=np.inf))


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
def test_forms_of_outside_for_every_pair_of_types(form):
    cols, vals, rows = _forms_stack()
    B, N, _ = cols.shape
    rng = np.random.default_rng(46)
    if form == "scalar":
        outside = 37.5
    elif form == "per_problem":
        outside = rng.uniform(10, 60, B)
        outside[1] = 2.0
    else:
        outside = rng.uniform(10, 60, (B, N))
        outside[1] = rng.permutation(N) / 4.0  # distinct
        for b in range(B):
            outside[b, rows[b]:] = np.nan  # never read
        assert np.isnan(outside).any()
    for problem in ("min", "max"):
        _, want = check(cols, vals, rows, outside, problem, dtypes=fxt.DTYPES)
    if form != "scalar":  # an array of another layout than the one meant is not accepted as it is
        with pytest.raises(ValueError, match="outside must have shape"):
            auction_solve_ell_batch(cols, vals, rows=rows, outside=outside.T if form == "per_row" else outside[:-1])


def test_device_outside_must_match_the_input():
    import torch
    cols, vals, rows = _forms_stack()
    dc, dv = _device(cols, vals)
    B, N, _ = cols.shape
    f = auction_solve_ell_batch
    with pytest.raises(TypeError, match="outside on the device"):
        f(cols, vals, rows=rows, outside=torch.zeros(B, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="float64"):
        f(dc, dv, rows=rows, outside=torch.zeros(B, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        f(dc, dv, rows=rows, outside=torch.zeros((B, N + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        f(dc, dv, rows=rows, outside=torch.zeros((N, B), dtype=torch.float64, device="cuda").T)


# ---- options

@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(eps_start=1e-3), dict(max_iter=3), dict(fast=False)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options(opts):
    cols, vals, rows, outside = _ladder(65 if "max_iter" in opts else 8)  # (K = 65: no problem is done in 3 rounds)
    res, want = check(cols, vals, rows, outside, "min", opts=opts)
    check(cols, vals, rows, outside, "max", opts=opts, dtypes=fxt.DTYPES[2:])
    if "max_iter" in opts:  # cut short: the rows left unassigned come back -1 and are not counted
        for b, (w, m, n) in enumerate(want):
            left = w["sol"] == -1
            assert left.any() and res["meta"]["n_assigned"][b] == n - left.sum() < n
            assert (res["sol"][b, :n][left] == -1).all() and res["meta"]["its"][b] == 3
    if "eps_start" in opts:
        assert all(np.float32(w["extra"]["start_eps_f32"]) == np.float32(opts["eps_start"]) for w, _, _ in want)


@pytest.mark.parametrize("problem", ["min", "max"])
def test_starting_prices(problem):
    cols, vals, rows, outside = _ladder(8)
    B = cols.shape[0]
    m = max(s[0] for s in _sizes(cols, rows))
    p0 = np.random.default_rng(47).uniform(0, 20, (B, m + 4))
    p0[0, ::3] = 0.0
    p0[:, m:] = np.nan  # beyond the real columns: not a price of the problem
    p0[2, _sizes(cols, rows)[2][0]:] = -1.0
    check(cols, vals, rows, outside, problem, prices=p0, dtypes=fxt.DTYPES[:2])
    check(cols, vals, rows, outside, problem, prices=p0, dtypes=fxt.DTYPES[2:], n_cols=m + 2, opts=dict(eps_start=0.25))


# ---- cross-layout: the plain call on the explicitly augmented stack

def _augmented(cols, vals, rows, outside):
    B, N, K = cols.shape
    o = np.broadcast_to(outside if np.ndim(outside) != 1 else np.asarray(outside)[:, None], (B, N))
    ac = np.concatenate([cols, np.full((B, N, 1), -1, dtype=cols.dtype)], axis=2)
    av = np.concatenate([vals, np.full((B, N, 1), np.nan, dtype=vals.dtype)], axis=2)
    for b, (m, n) in enumerate(_sizes(cols, rows)):
        ac[b, :n, K] = m + np.arange(n)
        av[b, :n, K] = o[b, :n]
    return ac, av


@pytest.mark.parametrize("kw", [dict(), dict(eps_start=0.5), dict(fast=False), dict(problem="max", max_iter=9)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("name", ["ladder65", "illegal", "forms"])
def test_same_outputs_as_the_plain_call_on_the_augmented_stack(name, kw):
    if name == "ladder65":
        cols64, vals64, rows, outside = _ladder(65)
    elif name == "illegal":
        cols64, vals64, rows, outside = _illegal()
    else:
        cols64, vals64, rows = _forms_stack()
        outside = np.array([30.0, 2.0, 5.0, 44.0])
    cols, vals = _typed(cols64, vals64, np.int64, np.float64)
    vals = np.where(cols >= 0, vals, np.nan)
    cols = np.where(cols >= 0, np.minimum(cols, fxt.CAP - 1), cols)  # (beyond n_b: still never read)
    sizes = _sizes(cols, rows)
    ac, av = _augmented(cols, vals, rows, outside)
    M = max(m + n for m, n in sizes)
    n_cols = max(max(m for m, _ in sizes), 1)
    resolved = dict(kw, fast=kw.get("fast", not kw.get("eps_start", 0.0) > 0))
    ref = auction_solve_ell_batch(ac, av, rows=rows, n_cols=M, cardinality_check=False, errors="status", **resolved)
    assert (ref["status"] == 0).all()
    for res in both(cols, vals, rows=rows, outside=outside, n_cols=n_cols, on_device=True, **kw):
        assert np.array_equal(res["status"], ref["status"])
        for b, (m, n) in enumerate(sizes):
            rs = ref["sol"][b]
            assert np.array_equal(res["sol"][b], np.where(rs >= m, -1, rs)), b
            assert np.array_equal(bits(res["prices"][b, :m]), bits(ref["prices"][b, :m])), b
            assert np.array_equal(bits(res["outside_prices"][b, :n]), bits(ref["prices"][b, m:m + n])), b
        for k, v in ref["meta"].items():
            if k not in ("timer", "gpu"):
                assert np.array_equal(np.asarray(res["meta"][k]).view(np.uint8), np.asarray(v).view(np.uint8)), k


# ---- verdicts

V_N, V_K, V_COLS, V_P = 16, 6, 30, 26


@functools.lru_cache(maxsize=1)
def _mixed():
    """A healthy problem at every even index, at every odd index one with a defect (kinds[b]: the first check it fails);
    two of the healthy ones are what the plain call condemns (an empty row, an infeasible graph)."""
    rng = np.random.default_rng([48, 1])
    N, K, P = V_N, V_K, V_P
    probs, rows, kinds, outs = [], [], [], []

    def healthy(n=None, kind="uniform"):
        n = int(rng.integers(3, N + 1)) if n is None else n
        return fxt.widen(*sparse_problem(rng, n, 22, 4, kind), n, K, rng)

    def add(cv, kind, n=None, o=None):
        probs.append(cv)
        rows.append(cv[0].shape[0] if n is None else n)
        kinds.append(kind)
        row = np.full(N, np.nan)
        row[:cv[0].shape[0]] = rng.uniform(10, 60, cv[0].shape[0]) if o is None else o
        outs.append(row)

    def entries(c, i):
        return np.flatnonzero(c[i] >= 0)

    def bad_outside(value, row, also_large=False):
        c, v = healthy(n=9)
        if also_large:
            c[0, entries(c, 0)[0]] = V_COLS + 3
        add((c, v), fxt.INFINITE_VALUE)
        outs[-1][row] = value

    def bad_entry():
        c, v = healthy(n=9)
        v[4, entries(c, 4)[-1]] = np.nan
        add((c, v), fxt.INFINITE_VALUE)

    def too_large(col):
        c, v = healthy(n=8)
        c[5, entries(c, 5)[1]] = col
        add((c, v), fxt.TOO_LARGE)

    def too_narrow():
        c, v = healthy(n=8)
        c[3, entries(c, 3)[0]] = P + 1  # (below V_COLS, beyond the prices)
        add((c, v), fxt.PRICES_TOO_NARROW)

    def empty_row():
        c, v = healthy(n=10)
        c[4] = -1
        add((c, v), fxt.OK)

    def infeasible():
        c, v = healthy(n=11)
        c[2], c[9] = -1, -3  # two rows whose only entry is the same column
        c[2, K - 1], c[9, 0] = 6, 6
        v[2, K - 1], v[9, 0] = 1.5, 2.5
        add((c, v), fxt.OK)

    plans = [lambda: add(healthy(), fxt.BAD_SHAPE, 0), lambda: add(healthy(), fxt.BAD_SHAPE, N + 1),
             lambda: bad_outside(np.nan, 0), lambda: bad_outside(np.inf, 8, also_large=True), lambda: bad_outside(-np.inf, 3),
             bad_entry, lambda: too_large(V_COLS), lambda: too_large(2**31 + 5), too_narrow,
             lambda: add(healthy(n=7), fxt.PRICE_NOT_FINITE), lambda: add(healthy(n=7), fxt.PRICE_NOT_FINITE),
             lambda: add(healthy(n=7), fxt.PRICE_NEGATIVE), lambda: add(healthy(n=7), fxt.PRICE_NEGATIVE),
             empty_row, infeasible]
    for k, plan in enumerate(plans):
        add(healthy(kind="ints" if k % 4 == 0 else "uniform"), fxt.OK)
        plan()
    cols, vals, _ = fxt.stack(probs, N, K, fill_col=fxt.INT_MAX, fill_val=np.inf)
    rows, kinds, outside = np.array(rows, dtype=np.int32), np.array(kinds, dtype=np.int32), np.stack(outs)
    B = len(probs)
    prices = rng.uniform(0, 5, (B, P))
    prices[::4] = 0.0
    seen = {fxt.PRICE_NOT_FINITE: 0, fxt.PRICE_NEGATIVE: 0}
    for b in np.flatnonzero(np.isin(kinds, (fxt.PRICE_NOT_FINITE, fxt.PRICE_NEGATIVE))):
        c = cols[b, :rows[b]]
        used = np.unique(c[c >= 0])
        prices[b, used[-1]] = {fxt.PRICE_NOT_FINITE: (np.nan, np.inf), fxt.PRICE_NEGATIVE: (-0.0, -3.0)}[int(kinds[b])][
            seen[int(kinds[b])] % 2]
        seen[int(kinds[b])] += 1
    for b in np.flatnonzero(kinds == fxt.OK):  # what lies beyond a problem's real columns is not its price
        c = cols[b, :rows[b]]
        prices[b, int(c.max()) + 1:] = np.nan if b % 8 == 0 else -1.0
    return dict(zip(("cols", "vals", "rows", "outside", "prices", "kinds"),
                    _frozen(cols, vals, rows, outside, prices, kinds)))


def expected_status(cols, vals, rows, outside, n_cols, prices):
    """(status, counts (B, 3) = n_rows, n_cols, nnz of the record) from the definition: the first check that fails."""
    B, N, _ = cols.shape
    status, counts = np.zeros(B, dtype=np.int32), np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        n = int(rows[b])
        if n < 1 or n > N:
            status[b] = fxt.BAD_SHAPE
            continue
        c, v = cols[b, :n], vals[b, :n]
        valid = c >= 0
        m = int(c[valid].max()) + 1 if valid.any() else 0
        counts[b] = (n, min(m + n, fxt.INT_MAX), int(valid.sum()) + n)
        if not (np.isfinite(v[valid].astype(np.float64)).all() and np.isfinite(outside[b, :n]).all()):
            status[b] = fxt.INFINITE_VALUE
        elif m > n_cols:
            status[b] = fxt.TOO_LARGE
        elif prices.shape[1] < m:
            status[b] = fxt.PRICES_TOO_NARROW
        elif not np.isfinite(prices[b, :m]).all():
            status[b] = fxt.PRICE_NOT_FINITE
        elif np.signbit(prices[b, :m]).any():
            status[b] = fxt.PRICE_NEGATIVE
    return status, counts


@functools.lru_cache(maxsize=None)
def _mixed_expect(vtype):
    fx = _mixed()
    cols, vals = _typed(fx["cols"], fx["vals"], np.int64, vtype)
    status, counts = expected_status(cols, vals, fx["rows"], fx["outside"], V_COLS, fx["prices"])
    ok = np.flatnonzero(status == 0)
    want = expect(cols[ok], vals[ok], fx["rows"][ok], fx["outside"][ok], "min", p0=fx["prices"][ok], fast=True, max_iter=200)
    return status, counts, dict(zip(ok.tolist(), want))


@pytest.mark.parametrize("dtypes", fxt.DTYPES, ids=["i32-f64", "i64-f32", "i64-f64", "i32-f32"])
def test_verdicts_on_the_mixed_batch(dtypes):
    fx = _mixed()
    rows, prices, outside = fx["rows"], fx["prices"], fx["outside"]
    cols, vals = _typed(fx["cols"], fx["vals"], *dtypes)
    status, counts, want = _mixed_expect(dtypes[1])
    assert np.array_equal(status, fx["kinds"]) and set(status) == {0, 3, 5, 6, 7, 13, 14}
    n_ok = 0
    for res in both(cols, vals, rows=rows, outside=outside, prices=prices, on_device=dtypes[0] is np.int64, n_cols=V_COLS,
                    max_iter=200, cardinality_check=dtypes[1] is np.float64):  # (ignored in this mode, either way)
        assert np.array_equal(res["status"], status), [(b, res["status"][b], status[b]) for b in range(len(status))]
        assert (res["matching_size"] == -1).all()
        for b in range(len(status)):
            if status[b] == 0:  # a healthy neighbour is intact: the oracle's result, bit for bit
                compare(res, b, *want[b])
                n_ok += 1
                continue
            assert (res["sol"][b] == -1).all(), b
            assert np.array_equal(bits(res["prices"][b]), bits(np.zeros(V_COLS))), b
            assert np.array_equal(bits(res["outside_prices"][b]), bits(np.zeros(V_N))), b
            assert (res["meta"]["n_rows"][b], res["meta"]["n_cols"][b], res["meta"]["nnz"][b]) == tuple(counts[b]), b
            for k in ZERO_META:
                assert res["meta"][k][b] == 0, (b, k)
    assert n_ok == 2 * int((status == 0).sum())
    # the default mode runs the same call and raises for the first bad problem
    for a, b in ((cols, vals), _device(cols, vals)):
        with pytest.raises(ValueError, match=r"^problem 1: rows = 0 outside 1 \.\. 16$"):
            auction_solve_ell_batch(a, b, rows=rows, outside=outside, prices=prices, n_cols=V_COLS, max_iter=200)
    texts = {fxt.INFINITE_VALUE: "val holds a NaN or an infinity", fxt.TOO_LARGE: "does not fit n_cols = 30|too large",
             fxt.PRICES_TOO_NARROW: "prices hold 26 columns, the problem has 28", fxt.PRICE_NOT_FINITE: "prices hold a NaN",
             fxt.PRICE_NEGATIVE: "prices must be >= 0"}
    for code, text in texts.items():
        b = int(np.flatnonzero(status == code)[0])
        sl = slice(b - 1, b + 1)
        with pytest.raises(ValueError, match=r"^problem 1: .*(" + text + ")"):
            auction_solve_ell_batch(cols[sl], vals[sl], rows=rows[sl], outside=outside[sl], prices=prices[sl], n_cols=V_COLS,
                                    max_iter=200)


# ---- the call does not wait

def test_the_call_does_not_wait():
    import torch
    rng = np.random.default_rng(49)
    B, N, K, M = 96, 48, 8, 48
    probs = [fxt.widen(*sparse_problem(rng, int(n), M, 5), int(n), K, rng) for n in rng.integers(10, N + 1, B)]
    cols, vals, rows = fxt.stack(probs, N, K)
    vals = np.where(cols >= 0, vals, -1.0)  # (finite everywhere: the NaN fill below is then the only source of a status 3)
    outside = rng.uniform(20, 60, (B, N))
    p0 = rng.uniform(0, 5, (B, M))
    want = expect(cols, vals, rows, outside, "min", p0=p0, fast=True)
    kw = dict(n_cols=M, errors="status")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        csrc, vsrc = torch.from_numpy(cols).cuda(), torch.from_numpy(vals).cuda()
        pd, rd, od = torch.from_numpy(p0).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(outside).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        cx, vx = csrc.clone(), vsrc.clone()
        auction_solve_ell_batch(cx, vx, rows=rd, prices=pd, outside=od, **kw)  # the warm-up call
        _busy(w, 2)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        _busy(w, 8)
        e[1].record()
        torch.cuda.synchronize()
        reps = int(np.ceil(8 * 400.0 / e[0].elapsed_time(e[1])))
        e[2].record()
        _busy(w, reps)
        e[3].record()
        torch.cuda.synchronize()
        D = e[2].elapsed_time(e[3])
        assert D >= 200.0, D
        vx.fill_(float("nan"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(w, reps)
        vx.copy_(vsrc, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_ell_batch(cx, vx, rows=rd, prices=pd, outside=od, **kw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _host(res)
    assert (got["status"] == 0).all()
    for b, (w_, m, n) in enumerate(want):
        compare(got, b, w_, m, n)
