"""auction_solve_sparse_batch(outside=) on the GPU (misslap_solve_sparse_batch_outside): an outside option per row of a
packed loc / val / offsets batch, so that a row may stay unmatched and a row may have no entry at all.

  parity        every problem is the oracle's result bit for bit on sparse_to_augmented's (loc_b, val_b) with
                size=(m_b + n_b, n_b), given in the caller's terms (a column >= m_b is -1, the prices split into the real
                and the outside ones) -- at the lane edges of the virtual entry (row lengths 0 .. 129) with ties between
                an entry and the outside entry, with rows without entries in every position, problems without entries,
                n_b > m_b, duplicate entries, at the workgroup-size steps and at the largest carve, for every form of
                `outside`, both problems, eps_start, max_iter and starting prices -- from numpy arrays and from device
                tensors that are slices of poisoned buffers.
  cross-layout  auction_solve_ell_batch(outside=) on the same problems padded with holes: identical outputs.
  verdicts      a mixed batch: the statuses derived on the CPU, healthy problems equal the oracle, condemned ones have
                exactly the defined outputs; errors="raise" and raise_for_status raise for the first bad problem.
  no wait       with dims and device inputs, behind >= 200 ms of queued work the call returns at once.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import (auction_solve_ell_batch, auction_solve_sparse_batch, batch_meta_to_host, raise_for_status,
                       sparse_to_augmented)
from tests import _sparse_outside_fixture as fxt
from tests._batch_shapes import bits, sparse_expect, sparse_problem, sparse_small_batch, threads_for
from tests.test_dense_batch_status import _busy
from tests.test_ell_outside import _device_outside, _oracle_opts, _some_of_each, compare
from tests.test_sparse_batch_status import ZERO_META, _device, _to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def expect(probs, sizes, outside, problem, p0=None, **opts):
    """The oracle on the definition: [(want, m_b, n_b)]."""
    loc, val, off = fxt.pack(probs)
    out = []
    for b, (lo, va, m, n) in enumerate(sparse_to_augmented(loc, val, off, sizes, outside)):
        assert lo.shape[0] == probs[b][0].shape[0] + n and np.isfinite(va).all()
        start = None if p0 is None else np.concatenate([p0[b, :m], np.zeros(n)])
        out.append((sparse_expect(lo, va, problem, size=(m + n, n), p0=start, **opts), m, n))
    return out


def _host(res):
    if isinstance(res["sol"], np.ndarray):
        return res
    assert res["outside_prices"].is_cuda and res["outside_prices"].device == res["sol"].device
    return dict(_to_host(res), outside_prices=res["outside_prices"].cpu().numpy())


def _strided(outside, pad=5):
    """A (B, P) outside on the device as a slice of a wider buffer of NaN: unit stride along a row, rows P + 2 pad apart."""
    import torch
    B, P = outside.shape
    buf = np.full((B + 2, P + 2 * pad), np.nan)
    buf[1:B + 1, pad:pad + P] = outside
    t = torch.from_numpy(buf).cuda()[1:B + 1, pad:pad + P]
    assert t.stride() == (P + 2 * pad, 1) and not t.is_contiguous()
    return t


def both(probs, sizes=None, outside=None, prices=None, on_device=False, dims=None, **kw):
    """The same batch from numpy arrays, and from device tensors that are slices of poisoned buffers; sizes stays on the
    host, prices and outside too (they travel pinned) or, with on_device, are device tensors.  Nothing is written."""
    import torch
    loc, val, off = fxt.pack(probs)
    before = (loc.copy(), val.copy(), None if not isinstance(outside, np.ndarray) else outside.copy())
    yield auction_solve_sparse_batch(loc, val, off, sizes=sizes, prices=prices, dims=dims, outside=outside, errors="status",
                                     **kw)
    assert np.array_equal(loc, before[0]) and np.array_equal(bits(val), bits(before[1]))
    dl, dv = _device(loc, val)
    do = outside
    if on_device and isinstance(outside, np.ndarray):
        do = _strided(outside) if outside.ndim == 2 else _device_outside(outside)
    dp = prices if prices is None or not on_device else torch.from_numpy(np.array(prices)).cuda()
    res = auction_solve_sparse_batch(dl, dv, off, sizes=sizes, prices=dp, dims=dims, outside=do, errors="status", **kw)
    for k in ("sol", "prices", "outside_prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == dl.device, k
    yield _host(res)
    assert np.array_equal(dl.cpu().numpy(), loc) and np.array_equal(bits(dv.cpu().numpy()), bits(val))  # never written
    if do is not outside:
        assert np.array_equal(bits(do.cpu().numpy()), bits(before[2]))


def check(probs, sizes, outside, problem="min", prices=None, dims=None, opts=(), want=None, on_device=(False, True)):
    """Both routes against the oracle, with outside / prices on the host and on the device; returns (last result, want)."""
    opts = dict(opts)
    if want is None:
        want = expect(probs, sizes, outside, problem, p0=prices, **_oracle_opts(opts))
    B = len(probs)
    Nmax = dims[0] if dims else min(max(n for _, _, n in want), fxt.CAP)
    Mmax = dims[1] if dims else min(max([1] + [m for _, m, _ in want]), fxt.CAP)
    res = None
    for dev in on_device:
        for res in both(probs, sizes=sizes, outside=outside, prices=prices, on_device=dev, dims=dims, problem=problem,
                        **opts):
            assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
            assert (res["matching_size"] == -1).all()  # no guard in this mode
            assert res["sol"].shape == (B, Nmax) and res["outside_prices"].shape == (B, Nmax)
            assert res["prices"].shape == (B, Mmax)
            assert res["meta"]["gpu"]["threads"] == threads_for(Nmax)
            assert res["meta"]["gpu"]["lds_bytes"] == 24 * (Mmax + Nmax) + 28 * Nmax
            for b, (w, m, n) in enumerate(want):
                compare(res, b, w, m, n)
    return res, want


# ---- the lane edges of the virtual entry

EDGE_LENS = ((0, 1, 63), (64, 65, 127, 128), (129, 0, 64, 1, 65, 128), (127, 129, 63, 0, 1))


@functools.lru_cache(maxsize=None)
def _edges():
    """Four problems of 3 .. 6 rows whose row lengths are 0, 1, 63, 64, 65, 127, 128 and 129: lane len & 63 of the virtual
    entry on both sides of the wrap, with a second and a third pass of the scan loop.  Values and outside values are small
    integers: a real entry ties with the outside entry, which must win."""
    rng = np.random.default_rng(71)
    probs = [fxt.ragged(rng, np.array(lens), 140, "ints") for lens in EDGE_LENS]
    outside = np.full((len(probs), 8), np.nan)
    for b, lens in enumerate(EDGE_LENS):
        outside[b, :len(lens)] = rng.integers(0, 3, len(lens))
    outside.setflags(write=False)
    return probs, outside


_EDGE_WANT = {}


@pytest.mark.parametrize("mode", ["single", "scaled"])
@pytest.mark.parametrize("problem", ["min", "max"])
def test_parity_at_the_lane_edges(problem, mode):
    probs, outside = _edges()
    assert sorted({k for lens in EDGE_LENS for k in lens}) == [0, 1, 63, 64, 65, 127, 128, 129]
    opts = dict(fast=True) if mode == "single" else dict(fast=False, eps_start=0.0)
    _, want = check(probs, None, outside, problem, opts=opts, want=_EDGE_WANT.get((problem, mode)))
    _EDGE_WANT[(problem, mode)] = want
    assert _some_of_each(want)
    tie = False  # a row whose best real value equals its outside value took the outside entry: the last stored one wins
    for b, ((lo, va), (w, m, n)) in enumerate(zip(probs, want)):
        for i in range(n):
            v = va[lo[:, 0] == i]
            if len(v) and (v.min() if problem == "min" else v.max()) == outside[b, i]:
                tie = True
    assert tie
    w, m, _ = want[0]
    assert np.isinf(w["p"][m + 0])  # the row without an entry: a one-entry row, whose bid is +inf


# ---- rows without entries, problems without entries, n_b > m_b

@functools.lru_cache(maxsize=None)
def _gapped():
    rng = np.random.default_rng(72)
    probs = [fxt.ragged(rng, np.array([3, 2, 4, 1, 5]), 9, "uniform"),                  # no gap
             fxt.ragged(rng, np.array([0, 3, 2, 0, 0, 0, 4, 1, 0, 2]), 8, "uniform"),  # row 0 empty, rows 3 .. 5, row 8
             (np.zeros((0, 2), dtype=np.int32), np.zeros(0)),                           # no entry at all: m_b = 0
             fxt.ragged(rng, np.array([2, 1, 3, 0, 2, 1, 3, 2, 1, 2, 0, 3]), 3, "ints"),  # n_b = 12 > m_b = 3
             fxt.ragged(rng, np.array([0, 0, 1]), 1, "uniform")]
    sizes = np.array([[0, 5], [-7, 13], [1, 4], [3, 12], [99, 6]], dtype=np.int64)  # (sizes[:, 0] is not read)
    outside = rng.uniform(20, 70, (5, 16))
    outside[3] = rng.integers(0, 4, 16)
    outside.setflags(write=False)
    return probs, sizes, outside


@pytest.mark.parametrize("problem", ["min", "max"])
def test_rows_and_problems_without_entries(problem):
    probs, sizes, outside = _gapped()
    res, want = check(probs, sizes, outside, problem)
    assert [(m, n) for _, m, n in want] == [(9, 5), (7, 13), (0, 4), (3, 12), (1, 6)]
    assert (res["sol"][2] == -1).all() and res["meta"]["n_assigned"][2] == 4 and res["meta"]["nnz"][2] == 4
    assert (res["sol"][1][[0, 3, 4, 5, 8, 10, 11, 12]] == -1).all()  # rows without entries stay unmatched
    assert (res["sol"][3] >= 0).sum() <= 3
    assert np.isinf(res["outside_prices"][1][[0, 3, 4, 5, 8, 10, 11, 12]]).all()
    # without sizes: n_b is the last stored row + 1; the problem without entries is NO_ENTRIES, its neighbours intact
    keep = [0, 1, 3, 4]
    sub = [probs[b] for b in keep]
    check(sub, None, outside[keep], problem)
    plain = auction_solve_sparse_batch(*fxt.pack(sub), sizes=sizes[keep], errors="status", cardinality_check=False)
    assert plain["status"][0] == 0 and (plain["status"][1:] != 0).all()  # the plain call condemns the gapped ones
    got = auction_solve_sparse_batch(*fxt.pack(probs), outside=outside, errors="status")
    assert list(got["status"]) == [0, 0, fxt.NO_ENTRIES, 0, 0]
    for b, (w, m, n) in zip(keep, expect(sub, None, outside[keep], "min", fast=True)):
        compare(got, b, w, m, n)


# ---- duplicate (i, j) entries

def test_duplicate_entries_and_a_chosen_duplicate():
    rng = np.random.default_rng(73)
    hand = (np.array([[0, 1], [0, 1], [0, 2], [2, 0], [2, 0], [2, 1]], dtype=np.int32), np.array([5.0, 4.0, 9.0, 1.0, 1.0, 8.0]))
    probs = [sparse_problem(rng, 12, 9 + 6, 7, "ints"), hand, sparse_problem(rng, 30, 31, 40, "uniform")]
    outside = np.array([3.0, 50.0, 60.0])
    check(probs, None, outside, "max")
    res, want = check(probs, None, outside, "min")
    w, m, n = want[1]
    assert list(w["sol"]) == [1, m + 1, 0]  # rows 0 and 2 chose a column they store twice: get_obj adds every copy
    assert res["meta"]["obj_f64"][1] == 5.0 + 4.0 + 50.0 + 1.0 + 1.0
    lo = probs[2][0]
    chosen = [(i, j) for i, j in enumerate(want[2][0]["sol"]) if j < want[2][1]]
    assert any(((lo[:, 0] == i) & (lo[:, 1] == j)).sum() > 1 for i, j in chosen)


# ---- the workgroup-size steps and the largest carve

@functools.lru_cache(maxsize=None)
def _small():
    rng = np.random.default_rng(74)
    probs = []
    for lo, va in sparse_small_batch():  # 5 .. 40 rows; a third of the rows lose their entries
        drop = np.isin(lo[:, 0], np.flatnonzero(rng.random(int(lo[:, 0].max()) + 1) < 0.3))
        drop[-1] = False
        probs.append((lo[~drop], va[~drop]))
    outside = rng.uniform(10, 60, (len(probs), 40))
    outside.setflags(write=False)
    return probs, outside


_SMALL_WANT = {}


@pytest.mark.parametrize("rows", [256, 257, 512, 513])
def test_parity_at_the_workgroup_size_steps(rows):
    probs, outside = _small()
    padded = np.full((len(probs), rows + 3), np.nan)
    padded[:, :40] = outside
    problem = "min" if rows % 2 == 0 else "max"
    _, want = check(probs, None, padded, problem, dims=(rows, 64), want=_SMALL_WANT.get(problem))
    _SMALL_WANT[problem] = want
    assert _some_of_each(want)


def test_the_largest_carve():
    """dims = (2048, 2048): 155 648 bytes of LDS for 2048 rows and 4096 objects.  One full problem of 16 distinct entries
    per row, and one whose entries sit in every eighth row only."""
    rng = np.random.default_rng(75)
    N = fxt.CAP
    full = fxt.ragged(rng, np.full(N, 16), N, "uniform")
    full[0][0, 1] = N - 1  # (the last real column is in use)
    lens = np.zeros(N, dtype=np.int64)
    lens[::8] = 16
    thin = fxt.ragged(rng, lens, N, "uniform")
    sizes = np.array([[0, N], [0, N]], dtype=np.int64)
    res, want = check([full, thin], sizes, np.array([12.0, 20.0]), "min", dims=(N, N), on_device=(True,))
    assert res["meta"]["gpu"]["lds_bytes"] == 155648 and res["meta"]["gpu"]["threads"] == 1024
    assert list(res["meta"]["n_cols"]) == [int(full[0][:, 1].max()) + 1 + N, int(thin[0][:, 1].max()) + 1 + N]
    assert _some_of_each(want[:1]) and want[1][0]["meta"]["its"] <= 3


# ---- options, starting prices, the forms of outside

@pytest.mark.parametrize("opts", [dict(eps_start=30.0), dict(eps_start=1e-3), dict(max_iter=3), dict(fast=False)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options(opts):
    probs, sizes, outside = _gapped()
    if "max_iter" in opts:  # (problems that are not done in 3 rounds)
        probs, outside = _small()
        sizes = None
    res, want = check(probs, sizes, outside, "min", opts=opts)
    check(probs, sizes, outside, "max", opts=opts, on_device=(True,))
    if "max_iter" in opts:  # cut short: the rows left unassigned come back -1 and are not counted
        left = [w["sol"] == -1 for w, _, _ in want]
        assert any(x.any() for x in left)
        for b, (w, m, n) in enumerate(want):
            assert res["meta"]["n_assigned"][b] == n - left[b].sum() and (res["sol"][b, :n][left[b]] == -1).all()
            assert res["meta"]["its"][b] <= 3
    if opts.get("eps_start") == 30.0:
        assert max(w["meta"]["nreductions"] for w, _, _ in want) >= 2  # several phases
        assert all(np.float32(w["extra"]["start_eps_f32"]) == np.float32(30.0) for w, _, _ in want)


@pytest.mark.parametrize("problem", ["min", "max"])
def test_starting_prices(problem):
    probs, sizes, outside = _gapped()
    rng = np.random.default_rng(76)
    p0 = rng.uniform(0, 20, (len(probs), 9 + 4))
    p0[0, ::3] = 0.0
    p0[:, 9:] = np.nan  # beyond the real columns: not a price of any problem
    p0[1, 8:] = -1.0
    p0[2] = np.nan  # (m_b = 0: no price of it is read)
    check(probs, sizes, outside, problem, prices=p0)
    check(probs, sizes, outside, problem, prices=p0, dims=(16, 11), opts=dict(eps_start=0.25))


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
def test_forms_of_outside(form):
    probs, sizes, _ = _gapped()
    rng = np.random.default_rng(77)
    B = len(probs)
    if form == "scalar":
        outside = -2.5  # (a negative outside value is a value like any other)
    elif form == "per_problem":
        outside = rng.uniform(-10, 60, B)
    else:
        outside = rng.uniform(-10, 60, (B, 13 + 6))  # P > Nmax; on the device a slice with a stride
        for b, s in enumerate(sizes):
            outside[b, s[1]:] = np.nan  # never read
    for problem in ("min", "max"):
        check(probs, sizes, outside, problem)
    if form == "per_row":
        with pytest.raises(ValueError, match="P >= Nmax = 13"):
            auction_solve_sparse_batch(*fxt.pack(probs), sizes=sizes, outside=np.ascontiguousarray(outside[:, :12]))


# ---- cross-layout: the ELL outside mode on the same problems padded with holes

@pytest.mark.parametrize("kw", [dict(), dict(eps_start=0.5), dict(fast=False), dict(problem="max", max_iter=9)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("name", ["edges", "gapped", "small"])
def test_same_outputs_as_the_ell_outside_mode(name, kw):
    sizes = None
    if name == "edges":
        probs, outside = _edges()
    elif name == "gapped":
        probs, sizes, outside = _gapped()
    else:
        probs, outside = _small()
    ns = fxt.rows_of(probs, sizes)
    N = max(ns)
    M = max([1] + [int(lo[:, 1].max()) + 1 for lo, _ in probs if len(lo)])
    cols, vals, rows = fxt.to_ell(probs, ns, N)
    ref = auction_solve_ell_batch(cols, vals, rows=rows, n_cols=M, outside=np.ascontiguousarray(outside[:, :N]),
                                  errors="status", **kw)
    assert (ref["status"] == 0).all()
    for res in both(probs, sizes=sizes, outside=outside, on_device=True, **kw):
        assert res["sol"].shape == ref["sol"].shape and res["prices"].shape == ref["prices"].shape
        for k in ("sol", "status", "matching_size"):
            assert np.array_equal(res[k], ref[k]), k
        for k in ("prices", "outside_prices"):
            assert np.array_equal(bits(res[k]), bits(ref[k])), k
        for k, v in ref["meta"].items():
            if k not in ("timer", "gpu"):
                assert np.array_equal(np.asarray(res["meta"][k]).view(np.uint8), np.asarray(v).view(np.uint8)), k


# ---- verdicts

@functools.lru_cache(maxsize=None)
def _mixed_expect(with_sizes):
    fx = fxt.mixed(with_sizes)
    status, counts = fxt.expected_status(fx["loc"], fx["val"], fx["offsets"], fx["sizes"], fx["outside"], fxt.V_DIMS,
                                         fx["prices"])
    ok = np.flatnonzero(status == 0)
    want = expect([fx["probs"][b] for b in ok], None if fx["sizes"] is None else fx["sizes"][ok], fx["outside"][ok], "min",
                  p0=fx["prices"][ok], fast=True, max_iter=200)
    return status, counts, dict(zip(ok.tolist(), want))


@pytest.mark.parametrize("with_sizes", [True, False], ids=["sizes", "no-sizes"])
def test_verdicts_on_the_mixed_batch(with_sizes):
    fx = fxt.mixed(with_sizes)
    status, counts, want = _mixed_expect(with_sizes)
    Nmax, Mmax = fxt.V_DIMS
    assert np.array_equal(status, fx["kinds"])
    assert set(status) == ({0, 3, 5, 6, 7, 10, 11, 13, 14} if with_sizes else {0, 3, 5, 6, 8, 10, 11, 13, 14})
    kw = dict(sizes=fx["sizes"], outside=fx["outside"], prices=fx["prices"], dims=fxt.V_DIMS, max_iter=200)
    n_ok = 0
    for dev in (False, True):
        for res in both(fx["probs"], on_device=dev, cardinality_check=dev, **kw):  # (ignored in this mode, either way)
            assert np.array_equal(res["status"], status), [(b, res["status"][b], status[b]) for b in range(len(status))]
            assert (res["matching_size"] == -1).all()
            for b in range(len(status)):
                if status[b] == 0:  # a healthy neighbour is intact: the oracle's result, bit for bit
                    compare(res, b, *want[b])
                    n_ok += 1
                    continue
                assert (res["sol"][b] == -1).all(), b
                assert np.array_equal(bits(res["prices"][b]), bits(np.zeros(Mmax))), b
                assert np.array_equal(bits(res["outside_prices"][b]), bits(np.zeros(Nmax))), b
                assert (res["meta"]["n_rows"][b], res["meta"]["n_cols"][b], res["meta"]["nnz"][b]) == tuple(counts[b]), b
                for k in ZERO_META:
                    assert res["meta"][k][b] == 0, (b, k)
            with pytest.raises(ValueError, match=r"^problem 1: loc holds a negative row or column index$"):
                raise_for_status(res)
    assert n_ok == 4 * int((status == 0).sum())
    # errors="raise" runs the same call and raises for the first bad problem, with its number
    loc, val, off = fx["loc"], fx["val"], fx["offsets"]
    for a, b in ((loc, val), _device(loc, val)):
        with pytest.raises(ValueError, match=r"^problem 1: loc holds a negative row or column index$"):
            auction_solve_sparse_batch(a, b, off, **kw)
    texts = {fxt.ROWS_UNSORTED: "rows must be sorted", fxt.INFINITE_VALUE: "NaN or an infinity .*outside value of a row",
             fxt.TOO_LARGE: r"does not fit dims = \(16, 30\)|too large",
             fxt.PRICES_TOO_NARROW: "prices hold 26 columns, the problem has 28", fxt.PRICE_NOT_FINITE: "prices hold a NaN",
             fxt.PRICE_NEGATIVE: "prices must be >= 0", fxt.BAD_SHAPE: r"sizes\[1, 1\] = ", fxt.NO_ENTRIES: "no entries"}
    for code, text in texts.items():
        if code not in status:
            continue
        b = int(np.flatnonzero(status == code)[0])
        sub = dict(kw, sizes=None if fx["sizes"] is None else fx["sizes"][b - 1:b + 1], outside=fx["outside"][b - 1:b + 1],
                   prices=fx["prices"][b - 1:b + 1])
        with pytest.raises(ValueError, match=r"^problem 1: .*(" + text + ")"):
            auction_solve_sparse_batch(*fxt.pack(fx["probs"][b - 1:b + 1]), **sub)


# ---- the call does not wait

def test_the_call_does_not_wait():
    import torch
    rng = np.random.default_rng(78)
    B, N, M = 96, 48, 48
    probs = []
    for n in rng.integers(10, N + 1, B):
        lens = rng.integers(0, 9, int(n))
        lens[-1] = 3
        probs.append(fxt.ragged(rng, lens, M, "uniform"))
    loc, val, off = fxt.pack(probs)
    outside = rng.uniform(20, 60, (B, N))
    p0 = rng.uniform(0, 5, (B, M))
    want = expect(probs, None, outside, "min", p0=p0, fast=True)
    kw = dict(dims=(N, M), errors="status")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        lsrc, vsrc = torch.from_numpy(loc).cuda(), torch.from_numpy(val).cuda()
        pd, od = torch.from_numpy(p0).cuda(), torch.from_numpy(outside).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        lx, vx = lsrc.clone(), vsrc.clone()
        auction_solve_sparse_batch(lx, vx, off, prices=pd, outside=od, **kw)  # the warm-up call
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
        res = auction_solve_sparse_batch(lx, vx, off, prices=pd, outside=od, **kw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _host(res)
    assert (got["status"] == 0).all()
    assert batch_meta_to_host(res)["n_rows"].tolist() == [n for _, _, n in want]
    for b, (w_, m, n) in enumerate(want):
        compare(got, b, w_, m, n)
