"""auction_solve_batch(outside=) on the GPU (misslap_solve_dense_batch_outside): an outside option per row of a dense
(B, N, M) stack, so that a row may stay unmatched.

  parity       every problem is the oracle's result bit for bit on dense_to_augmented's aug_b (from_matrix(aug_b).solve()),
               given in the caller's terms (a column >= m_b is -1, the prices split into the real and the outside ones)
               -- at the lane edges of the virtual entry (m = 1 .. 130 under 70 rows), with ties between an entry and
               the outside entry, fully gated rows, shapes the plain call cannot take (n_b > m_b, all gated), at the
               workgroup-size steps and at the largest carve, for every form of `outside` and every element type,
               eps_start, max_iter and starting prices -- from numpy arrays and from device tensors.
  cross-check  the plain status call on the explicitly augmented (B, N, M + N) stack: identical outputs after the mapping.
  verdicts     a mixed batch: the statuses derived here on the CPU, healthy problems equal the oracle, condemned ones
               have exactly the defined outputs; the default mode raises.
  safety       device inputs are slices of poisoned buffers and are never written.
  no wait      with a device stack and a device `outside`, behind >= 200 ms of queued work the call returns at once.
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, batch_meta_to_host, dense_to_augmented
from tests._batch_shapes import META_KEYS, bits, dense_expect, threads_for
from tests._status_fixture import expected_status as plain_status
from tests.test_dense_batch_status import _busy
from tests.test_ell_batch import ZERO_META

pytestmark = pytest.mark.gpu

OK, INFINITE_VALUE, PRICE_NOT_FINITE, PRICE_NEGATIVE, BAD_SHAPE, BAD_OUTSIDE = 0, 3, 5, 6, 7, 15


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


def _gate(rng, v, share=0.5):
    """About `share` of the entries gated, as -1 and as NaN."""
    h = rng.random(v.shape) < share
    v[h] = np.where(rng.random(v.shape) < 0.7, -1.0, np.nan)[h]
    return v


def _stack(probs, N, M, fill=np.inf):
    """Problems of their own shapes in one (B, N, M) stack; beyond a shape the stack holds `fill`."""
    mats = np.full((len(probs), N, M), fill)
    for b, p in enumerate(probs):
        mats[b, :p.shape[0], :p.shape[1]] = p
    return mats, np.array([p.shape for p in probs], dtype=np.int32)


def _outside(rows, N, shapes):
    """Per-row outside values in a (B, N) array that holds NaN beyond n_b."""
    out = np.full((len(rows), N), np.nan)
    for b, r in enumerate(rows):
        out[b, :shapes[b][0]] = r
    return out


def _typed(draw, dtype):
    """A float64 draw in the call's type: (numpy stack or, for bfloat16, a torch CPU tensor; the values widened)."""
    if dtype == "bfloat16":
        import torch
        t = torch.from_numpy(np.array(draw)).to(torch.bfloat16)
        return t, t.double().numpy()
    a = np.ascontiguousarray(draw.astype(dtype))
    return a, a.astype(np.float64)


def _sizes(mats, shapes):
    B, N, M = mats.shape
    return [(N, M) if shapes is None else (int(shapes[b][0]), int(shapes[b][1])) for b in range(B)]


def expect(wide, shapes, outside, problem, p0=None, **opts):
    """The oracle on the definition: [(want, m_b, n_b)].  wide: the stack's values as float64."""
    out = []
    for b, (aug, (n, m)) in enumerate(zip(dense_to_augmented(wide, shapes, outside=outside), _sizes(wide, shapes))):
        assert aug.shape == (n, m + n)
        start = None if p0 is None else np.concatenate([p0[b, :m], np.zeros(n)])
        want = dense_expect(aug, problem, p0=start, cardinality_check=False, **opts)
        with np.errstate(invalid="ignore"):
            want["nnz"] = int((aug >= 0).sum())
        out.append((want, m, n))
    return out


def compare(res, b, want, m, n):
    """Problem b of an outside result against the oracle's result on the augmented matrix."""
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
    """A result with numpy arrays and the host meta dict, whichever way it was computed."""
    if isinstance(res["sol"], np.ndarray):
        return res
    meta = batch_meta_to_host(res)
    for k, v in res["meta"].items():  # the device views hold the same records
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), meta[k]), k
    out = dict(res, meta=meta)
    for k in ("sol", "prices", "outside_prices", "status", "matching_size"):
        assert res[k].is_cuda and res[k].device == res["sol"].device, k
        out[k] = res[k].cpu().numpy()
    return out


def _inside(a, fill, pad=4096):
    """A host array (numpy, or a torch CPU tensor) on the device as a slice of a larger buffer that holds `fill`."""
    import torch
    t = torch.from_numpy(np.array(a)) if isinstance(a, np.ndarray) else a  # (a copy: torch takes no read-only array)
    buf = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype)
    buf[pad:pad + t.numel()] = t.reshape(-1)
    d = buf.cuda()[pad:pad + t.numel()].view(t.shape)
    assert d.is_contiguous() and d.data_ptr() != d.untyped_storage().data_ptr()
    return d


def _raw(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy().tobytes()


def both(mats, shapes=None, outside=None, prices=None, on_device=False, **kw):
    """The same batch from a numpy stack (where numpy has the type), and from a device tensor that is a slice of a
    poisoned buffer; shapes, prices and outside stay on the host (they travel pinned) or, with on_device, are device
    tensors too.  Nothing is written."""
    import torch
    if isinstance(mats, np.ndarray):
        before = (mats.copy(), None if not isinstance(outside, np.ndarray) else outside.copy())
        yield auction_solve_batch(mats, shapes=shapes, prices=prices, outside=outside, errors="status", **kw)
        assert mats.tobytes() == before[0].tobytes()
        assert before[1] is None or np.array_equal(bits(outside), bits(before[1]))
    dm = _inside(mats, np.inf)
    want_bytes = _raw(dm)
    do = _inside(outside, np.nan, 512) if on_device and isinstance(outside, np.ndarray) else outside
    dp = prices if prices is None or not on_device else _inside(prices, np.nan, 512)
    ds = shapes if shapes is None or not on_device else torch.from_numpy(np.array(shapes, dtype=np.int32)).cuda()
    res = auction_solve_batch(dm, shapes=ds, prices=dp, outside=do, errors="status", **kw)
    yield _host(res)
    assert _raw(dm) == want_bytes  # never written
    if do is not outside:
        assert np.array_equal(bits(do.cpu().numpy()), bits(outside))
    if dp is not prices:
        assert np.array_equal(bits(dp.cpu().numpy()), bits(prices))


def _oracle_opts(opts):
    """The front end's resolution of `fast`, for the oracle: a single phase unless eps_start > 0 was given."""
    o = dict(opts)
    o.pop("cardinality_check", None)
    if o.get("fast") is None:
        o["fast"] = not o.get("eps_start", 0.0) > 0
    return o


def check(draw, shapes, outside, problem="min", dtypes=("float64",), prices=None, opts=(), want_cache=None,
          on_device=None):
    """Both routes for each element type against the oracle on the widened stack; returns the last host result."""
    B, N, M = draw.shape
    opts = dict(opts)
    res = want = None
    for k, dtype in enumerate(dtypes):
        mats, wide = _typed(draw, dtype)
        key = (dtype, problem)
        if want_cache is None or key not in want_cache:
            want = expect(wide, shapes, outside, problem, p0=prices, **_oracle_opts(opts))
            if want_cache is not None:
                want_cache[key] = want
        else:
            want = want_cache[key]
        for res in both(mats, shapes=shapes, outside=outside, prices=prices, mat_dtype=dtype, problem=problem,
                        on_device=bool(k % 2) if on_device is None else on_device, **opts):
            assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
            assert (res["matching_size"] == -1).all()  # no guard in this mode
            assert res["sol"].shape == (B, N) and res["outside_prices"].shape == (B, N) and res["prices"].shape == (B, M)
            assert res["meta"]["gpu"]["threads"] == threads_for(N)
            assert res["meta"]["gpu"]["lds_bytes"] == 24 * (M + N) + 28 * N
            for b, (w, m, n) in enumerate(want):
                compare(res, b, w, m, n)
    return res, want


def _some_of_each(want):
    """Whether, over the problems, some rows took a real column and some their outside option."""
    out = np.concatenate([w["sol"] >= m for w, m, _ in want])
    return out.any() and (~out).any()


# ---- the lane edges of the virtual entry

EDGE_N = 70


@functools.lru_cache(maxsize=None)
def _ladder(m, N=EDGE_N):
    """Three problems under N = 70 rows, so that m + i passes every lane: uniform values; small integers with integer
    outside values (ties between an entry and the outside entry); a short one (n = 33) with fewer columns.  About half
    the entries are gated; row 5 of the first and row 0 of the second are fully gated.  Beyond the shapes the stack holds
    +inf and outside holds NaN."""
    rng = np.random.default_rng([51, m])
    probs = [_gate(rng, rng.uniform(0, 100, (N, m))), _gate(rng, rng.integers(0, 5, (N, m)).astype(np.float64)),
             _gate(rng, rng.uniform(0, 100, (33, max(1, m * 3 // 4))))]
    probs[0][5] = -1.0
    probs[1][0] = np.nan
    probs[1][1, 0] = 2.0  # (a valid entry that ties with row 1's outside value below, whatever the gate drew)
    mats, shapes = _stack(probs, N, m)
    out1 = rng.integers(0, 5, N).astype(np.float64)
    out1[1] = 2.0
    outside = _outside([rng.uniform(0, 100, N), out1, rng.uniform(20, 80, 33)], N, shapes)
    return _frozen(mats, shapes, outside)


_LADDER_WANT = {}


@pytest.mark.parametrize("mode", ["single", "scaled"])
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_parity_at_the_lane_edges(m, problem, mode):
    mats, shapes, outside = _ladder(m)
    assert [tuple(s) for s in shapes] == [(70, m), (70, m), (33, max(1, m * 3 // 4))]
    with np.errstate(invalid="ignore"):
        valid = [mats[b, :n, :k] >= 0 for b, (n, k) in enumerate(shapes)]
    assert not valid[0][5].any() and not valid[1][0].any()
    if m > 2:
        assert 0.35 < np.mean([v.mean() for v in valid]) < 0.65
    assert np.isinf(mats[2, 33:]).all() and np.isnan(outside[2, 33:]).all()
    opts = dict(fast=True) if mode == "single" else dict(fast=False, eps_start=0.0)
    _, want = check(mats, shapes, outside, problem, opts=opts, want_cache=_LADDER_WANT.setdefault((m, mode), {}))
    if mode == "single":
        assert all(w["meta"]["eCE"] == 1 for w, _, _ in want)
    else:
        assert max(w["meta"]["nreductions"] for w, _, _ in want) >= 2  # several phases
    assert _some_of_each(want)
    assert (mats[1, :, :m] == outside[1][:, None]).any()  # an entry ties with its row's outside entry
    assert np.isinf(want[0][0]["p"][m + 5]) and np.isinf(want[1][0]["p"][m + 0])  # a one-entry row bids +inf


# ---- shapes the plain call cannot take

@functools.lru_cache(maxsize=None)
def _illegal():
    """40 x 7, 3 x 1, and all-gated 1 x 1 and 5 x 4, in one stack."""
    rng = np.random.default_rng(52)
    tall = _gate(rng, rng.uniform(0, 100, (40, 7)))
    tall[0, 6] = 50.0
    probs = [tall, np.array([[3.0], [1.0], [2.0]]), np.array([[-1.0]]), np.where(rng.random((5, 4)) < 0.5, -1.0, np.nan)]
    mats, shapes = _stack(probs, 40, 7)
    return _frozen(mats, shapes, rng.uniform(30, 70, (4, 40)))


@pytest.mark.parametrize("problem", ["min", "max"])
def test_shapes_that_were_illegal(problem):
    mats, shapes, outside = _illegal()
    assert [tuple(s) for s in shapes] == [(40, 7), (3, 1), (1, 1), (5, 4)]
    res, want = check(mats, shapes, outside, problem, dtypes=("float64", "float32"))
    assert (res["sol"][2:] == -1).all() and list(res["meta"]["n_assigned"][2:]) == [1, 5]  # all gated: all outside
    assert (res["sol"][0] >= 0).sum() <= 7  # at most m rows hold a real column
    assert (res["sol"][1] >= 0).sum() == (1 if problem == "min" else 0)  # (costs 1 .. 3 against outside values 30 .. 70)
    assert _some_of_each(want[:1])
    assert np.isinf(res["outside_prices"][2, 0]) and np.isinf(res["outside_prices"][3, :5]).all()
    # the plain status call condemns every one of them
    status, _ = plain_status(mats, shapes)
    assert (status != 0).all() and list(status[1:]) == [4, 1, 1]  # (the guard: 3 rows on 1 column; too few values)
    plain = auction_solve_batch(np.array(mats), shapes=shapes, errors="status")
    assert np.array_equal(plain["status"], status)


# ---- the workgroup-size steps and the largest carve

@functools.lru_cache(maxsize=None)
def _tall(N, M=40):
    rng = np.random.default_rng([53, N])
    probs = [_gate(rng, rng.uniform(0, 100, (N, M)), 0.9), _gate(rng, rng.integers(0, 5, (N - 1, M - 3)).astype(np.float64), 0.9)]
    mats, shapes = _stack(probs, N, M)
    outside = _outside([rng.uniform(0, 60, N), rng.integers(0, 5, N - 1).astype(np.float64)], N, shapes)
    return _frozen(mats, shapes, outside)


@pytest.mark.parametrize("N", [256, 257, 513])
def test_parity_at_the_workgroup_size_steps(N):
    mats, shapes, outside = _tall(N)
    _, want = check(mats, shapes, outside, "min", on_device=False)
    check(mats, shapes, outside, "max", dtypes=("float32",), on_device=True)
    assert _some_of_each(want)


def test_the_largest_carve():
    """B = 2 at N = M = 1024: 77 824 bytes of LDS for 1024 rows and 2048 objects, above the 64 KB a kernel gets unasked."""
    rng = np.random.default_rng(54)
    N = _lib.DENSE_BATCH_MAX_DIM
    probs = [_gate(rng, rng.uniform(0, 100, (N, N)), 0.97), _gate(rng, rng.uniform(0, 100, (N - 3, N - 5)), 0.97)]
    probs[0][0, N - 1] = 1.0  # the last real column is in use
    mats, shapes = _stack(probs, N, N)
    outside = np.array([12.0, 20.0])
    res, want = check(mats, shapes, outside, "min", on_device=True)
    assert res["meta"]["gpu"]["lds_bytes"] == 24 * (2 * N) + 28 * N == 77824
    assert list(res["meta"]["n_cols"]) == [2 * N, 2 * N - 8] and _some_of_each(want)


# ---- the forms of `outside`, for every element type

DTYPES = ("float64", "float32", "float16", "bfloat16")


@functools.lru_cache(maxsize=None)
def _forms_stack():
    """Quarter steps below 50: exact in every one of the four types (8 significant bits)."""
    rng = np.random.default_rng(55)
    N, M = 20, 25
    probs = [_gate(rng, rng.integers(0, 200, shape) / 4.0) for shape in ((20, 25), (13, 9), (1, 25), (17, 20))]
    return _frozen(*_stack(probs, N, M))


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
def test_forms_of_outside_for_every_element_type(form):
    mats, shapes = _forms_stack()
    B, N, _ = mats.shape
    rng = np.random.default_rng(56)
    if form == "scalar":
        outside = 37.5
    elif form == "per_problem":
        outside = rng.integers(40, 240, B) / 4.0
        outside[1] = -0.0  # valid: every row of problem 1 may leave for nothing
    else:
        outside = rng.integers(40, 240, (B, N)) / 4.0
        outside[1] = rng.permutation(N) / 4.0  # distinct
        for b in range(B):
            outside[b, shapes[b][0]:] = np.nan  # never read
        assert np.isnan(outside).any()
    for dtype in DTYPES:
        _, wide = _typed(mats, dtype)
        assert np.array_equal(wide, mats, equal_nan=True)  # exactly representable
    for problem in ("min", "max"):
        for on_device in (False, True):  # outside (and shapes) on the host, and on the device
            _, want = check(mats, shapes, outside, problem, dtypes=DTYPES, on_device=on_device)
    if form != "scalar":  # an array of another layout than the one meant is not accepted as it is
        with pytest.raises(ValueError, match="outside must have shape"):
            auction_solve_batch(np.array(mats), shapes=shapes, outside=outside.T if form == "per_row" else outside[:-1])


def test_device_outside_must_match_the_input():
    import torch
    mats, shapes = _forms_stack()
    dm = torch.from_numpy(np.array(mats)).cuda()
    B, N, _ = mats.shape
    f = auction_solve_batch
    with pytest.raises(TypeError, match="outside on the device needs mats on the device"):
        f(np.array(mats), shapes=shapes, outside=torch.zeros(B, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="float64"):
        f(dm, shapes=shapes, outside=torch.zeros(B, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        f(dm, shapes=shapes, outside=torch.zeros((B, N + 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        f(dm, shapes=shapes, outside=torch.zeros((N, B), dtype=torch.float64, device="cuda").T)


# ---- options and starting prices

@pytest.mark.parametrize("opts", [dict(eps_start=0.5), dict(eps_start=1e-3), dict(max_iter=3), dict(fast=False)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options(opts):
    mats, shapes, outside = _ladder(65)
    res, want = check(mats, shapes, outside, "min", opts=opts, on_device=False)
    check(mats, shapes, outside, "max", opts=opts, dtypes=("float32",), on_device=True)
    if "max_iter" in opts:  # cut short: the rows left unassigned come back -1 and are not counted
        for b, (w, m, n) in enumerate(want):
            left = w["sol"] == -1
            assert left.any() and res["meta"]["n_assigned"][b] == n - left.sum() < n
            assert (res["sol"][b, :n][left] == -1).all() and res["meta"]["its"][b] == 3
    if "eps_start" in opts:
        assert all(np.float32(w["extra"]["start_eps_f32"]) == np.float32(opts["eps_start"]) for w, _, _ in want)


@pytest.mark.parametrize("problem", ["min", "max"])
def test_starting_prices(problem):
    mats, shapes, outside = _ladder(65)
    B, _, M = mats.shape
    p0 = np.random.default_rng(57).uniform(0, 20, (B, M))
    p0[0, ::3] = 0.0
    p0[2, shapes[2][1]:] = np.where(np.arange(M - shapes[2][1]) % 2, -1.0, np.nan)  # beyond m_b: not its prices
    check(mats, shapes, outside, problem, prices=p0, on_device=False)
    check(mats, shapes, outside, problem, prices=p0, dtypes=("float16",), on_device=True, opts=dict(eps_start=0.25))


# ---- cross-check: the plain status call on the explicitly augmented stack

def _augmented_stack(mats, shapes, outside, prices=None):
    B, N, M = mats.shape
    augs = dense_to_augmented(mats, shapes, outside=outside)
    stack = np.full((B, N, M + N), -1.0)
    p = None if prices is None else np.zeros((B, M + N))
    for b, (aug, (n, m)) in enumerate(zip(augs, _sizes(mats, shapes))):
        stack[b, :n, :m + n] = aug
        if p is not None:
            p[b, :m] = prices[b, :m]
    return stack, np.array([a.shape for a in augs], dtype=np.int32), p


@pytest.mark.parametrize("kw", [dict(), dict(eps_start=0.5), dict(fast=False), dict(problem="max", max_iter=9)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "default")
@pytest.mark.parametrize("name", ["ladder65", "illegal", "forms"])
def test_same_outputs_as_the_plain_call_on_the_augmented_stack(name, kw):
    if name == "ladder65":
        mats, shapes, outside = _ladder(65)
    elif name == "illegal":
        mats, shapes, outside = _illegal()
    else:
        mats, shapes = _forms_stack()
        outside = np.array([30.0, 2.0, 5.0, 44.0])
    sizes = _sizes(mats, shapes)
    prices = np.random.default_rng(58).uniform(0, 9, mats.shape[::2]) if name == "forms" else None
    clean = np.where(np.isinf(mats), -1.0, mats)  # (beyond the shapes; the explicit stack is gated there)
    stack, aug_shapes, aug_prices = _augmented_stack(clean, shapes, outside, prices)
    assert stack.shape[2] <= _lib.DENSE_BATCH_MAX_DIM
    resolved = dict(kw, fast=kw.get("fast", not kw.get("eps_start", 0.0) > 0))
    ref = auction_solve_batch(stack, shapes=aug_shapes, prices=aug_prices, cardinality_check=False, errors="status", **resolved)
    assert (ref["status"] == 0).all()
    for res in both(np.array(mats), shapes=shapes, outside=outside, prices=prices, on_device=True, **kw):
        assert np.array_equal(res["status"], ref["status"])
        for b, (n, m) in enumerate(sizes):
            rs = ref["sol"][b]
            assert np.array_equal(res["sol"][b], np.where(rs >= m, -1, rs)), b
            assert np.array_equal(bits(res["prices"][b, :m]), bits(ref["prices"][b, :m])), b
            assert np.array_equal(bits(res["outside_prices"][b, :n]), bits(ref["prices"][b, m:m + n])), b
        for k, v in ref["meta"].items():
            if k not in ("timer", "gpu"):
                assert np.array_equal(np.asarray(res["meta"][k]).view(np.uint8), np.asarray(v).view(np.uint8)), k


# ---- verdicts

V_N, V_M = 16, 12


@functools.lru_cache(maxsize=1)
def _mixed():
    """A healthy problem at every even index, at every odd index one with a defect (kinds[b]: the first check it fails).
    Two of the healthy ones are so only because the NaN and the negative outside values lie beyond n_b; others are what
    the plain call condemns (a fully gated row, n_b > m_b)."""
    rng = np.random.default_rng([59, 1])
    N, M = V_N, V_M
    probs, kinds, outs, shp, fix = [], [], [], [], []

    def healthy(n=None, m=None, kind="uniform"):
        n = int(rng.integers(3, N + 1)) if n is None else n
        m = int(rng.integers(2, M + 1)) if m is None else m
        v = rng.uniform(0, 100, (n, m)) if kind == "uniform" else rng.integers(0, 5, (n, m)).astype(np.float64)
        v = _gate(rng, v, 0.4)
        v[0, 0] = 7.0  # (a valid entry in the first column: the price at column 0 is one of the problem's)
        return v

    def add(v, kind, shape=None, beyond=np.nan, price=None):
        n = v.shape[0]
        probs.append(v)
        kinds.append(kind)
        shp.append(v.shape if shape is None else shape)
        row = np.full(N, beyond)
        row[:n] = rng.uniform(10, 60, n)
        outs.append(row)
        fix.append(price)

    def bad_outside(value, row, kind=BAD_OUTSIDE, also_inf_entry=False):
        v = healthy(n=9)
        if also_inf_entry:  # (BAD_OUTSIDE comes first)
            v[2, 0] = np.inf
        add(v, kind)
        outs[-1][row] = value

    def inf_entry():
        v = healthy(n=9)
        v[4, 0] = np.inf
        add(v, INFINITE_VALUE)

    def gated_row():
        v = healthy(n=10)
        v[4] = -1.0
        add(v, OK)

    plans = [lambda: add(healthy(), BAD_SHAPE, (0, 5)), lambda: add(healthy(), BAD_SHAPE, (4, M + 1)),
             lambda: bad_outside(-1.0, 0), lambda: bad_outside(-np.inf, 3, also_inf_entry=True),
             lambda: bad_outside(np.nan, 8), lambda: bad_outside(np.inf, 8, INFINITE_VALUE), inf_entry,
             lambda: add(healthy(n=7), PRICE_NOT_FINITE, price=np.nan), lambda: add(healthy(n=7), PRICE_NOT_FINITE, price=np.inf),
             lambda: add(healthy(n=7), PRICE_NEGATIVE, price=-0.0), lambda: add(healthy(n=7), PRICE_NEGATIVE, price=-3.0),
             lambda: add(healthy(n=6), OK, beyond=np.nan), lambda: add(healthy(n=6), OK, beyond=-2.0),
             gated_row, lambda: add(healthy(n=N, m=3), OK)]
    for k, plan in enumerate(plans):
        add(healthy(kind="ints" if k % 4 == 0 else "uniform"), OK)
        plan()
    mats, _ = _stack(probs, N, M)
    shapes, kinds, outside = np.array(shp, dtype=np.int32), np.array(kinds, dtype=np.int32), np.stack(outs)
    B = len(probs)
    prices = rng.uniform(0, 5, (B, M))
    prices[::4] = 0.0
    for b in range(B):
        if fix[b] is not None:
            prices[b, 0] = fix[b]
        elif kinds[b] == OK:  # what lies beyond a problem's columns is not its price
            prices[b, shapes[b][1]:] = np.nan if b % 8 == 0 else -1.0
    return dict(zip(("mats", "shapes", "outside", "prices", "kinds"), _frozen(mats, shapes, outside, prices, kinds)))


def expected_status(mats, shapes, outside, prices):
    """(status, counts (B, 3) = n_rows, n_cols, nnz of the record) from the definition: the first check that fails."""
    B, N, M = mats.shape
    status, counts = np.zeros(B, dtype=np.int32), np.zeros((B, 3), dtype=np.int64)
    for b in range(B):
        n, m = (int(x) for x in shapes[b])
        if n < 1 or n > N or m < 1 or m > M:
            status[b] = BAD_SHAPE
            continue
        a, o, p = mats[b, :n, :m], outside[b, :n], prices[b, :m]
        with np.errstate(invalid="ignore"):
            valid, o_valid = a >= 0, o >= 0
        counts[b] = (n, m + n, int(valid.sum()) + n)
        if not o_valid.all():
            status[b] = BAD_OUTSIDE
        elif np.isinf(a[valid]).any() or np.isinf(o).any():
            status[b] = INFINITE_VALUE
        elif not np.isfinite(p).all():
            status[b] = PRICE_NOT_FINITE
        elif np.signbit(p).any():
            status[b] = PRICE_NEGATIVE
    return status, counts


@functools.lru_cache(maxsize=None)
def _mixed_expect(dtype):
    fx = _mixed()
    _, wide = _typed(fx["mats"], dtype)
    status, counts = expected_status(wide, fx["shapes"], fx["outside"], fx["prices"])
    ok = np.flatnonzero(status == 0)
    want = expect(wide[ok], fx["shapes"][ok], fx["outside"][ok], "min", p0=fx["prices"][ok], fast=True, max_iter=200)
    return status, counts, dict(zip(ok.tolist(), want))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_verdicts_on_the_mixed_batch(dtype):
    import torch
    fx = _mixed()
    shapes, prices, outside = fx["shapes"], fx["prices"], fx["outside"]
    mats, _ = _typed(fx["mats"], dtype)
    status, counts, want = _mixed_expect(dtype)
    assert np.array_equal(status, fx["kinds"]) and set(status) == {0, 3, 5, 6, 7, 15}
    B = len(status)
    dm = _inside(mats, np.inf)
    dev = dict(shapes=torch.from_numpy(np.array(shapes)).cuda(), prices=_inside(prices, np.nan, 512),
               outside=_inside(outside, np.nan, 512))  # (BAD_SHAPE is a device verdict: host shapes raise)
    n_ok = 0
    for cardinality_check in (True, False):  # (ignored in this mode, either way)
        res = _host(auction_solve_batch(dm, errors="status", mat_dtype=dtype, max_iter=200,
                                        cardinality_check=cardinality_check, **dev))
        assert np.array_equal(res["status"], status), [(b, res["status"][b], status[b]) for b in range(B)]
        assert (res["matching_size"] == -1).all()
        for b in range(B):
            if status[b] == 0:  # a healthy neighbour is intact: the oracle's result, bit for bit
                compare(res, b, *want[b])
                n_ok += 1
                continue
            assert (res["sol"][b] == -1).all(), b
            assert np.array_equal(bits(res["prices"][b]), bits(np.zeros(V_M))), b
            assert np.array_equal(bits(res["outside_prices"][b]), bits(np.zeros(V_N))), b
            assert (res["meta"]["n_rows"][b], res["meta"]["n_cols"][b], res["meta"]["nnz"][b]) == tuple(counts[b]), b
            for k in ZERO_META:
                assert res["meta"][k][b] == 0, (b, k)
    assert n_ok == 2 * int((status == 0).sum())
    # the healthy and the host-checkable problems from numpy arrays: the same verdicts
    keep = np.flatnonzero(status != BAD_SHAPE)
    res = auction_solve_batch(mats[keep], shapes=shapes[keep], prices=prices[keep], outside=outside[keep], errors="status",
                              mat_dtype=dtype, max_iter=200)
    assert np.array_equal(res["status"], status[keep])
    for k, b in enumerate(keep):
        if status[b] == 0:
            compare(res, k, *want[int(b)])
    # the default mode runs the same call and raises for the first bad problem
    with pytest.raises(ValueError, match=r"^problem 1: shape \(0, 5\) outside 1 \.\. 16 x 1 \.\. 12$"):
        auction_solve_batch(dm, mat_dtype=dtype, max_iter=200, **dev)
    texts = {BAD_OUTSIDE: r"the outside value of row 0 is -1\.0: it must be >= 0", INFINITE_VALUE: "val holds a NaN or an infinity",
             PRICE_NOT_FINITE: "prices hold a NaN", PRICE_NEGATIVE: "prices must be >= 0"}
    for code, text in texts.items():
        b = int(np.flatnonzero(status == code)[0])
        sl = slice(b - 1, b + 1)
        for stack, kw in ((mats[sl], dict(shapes=shapes[sl], prices=prices[sl], outside=outside[sl])),
                          (dm[sl], {k: v[sl] for k, v in dev.items()})):
            with pytest.raises(ValueError, match=r"^problem 1: .*(" + text + ")"):
                auction_solve_batch(stack, mat_dtype=dtype, max_iter=200, **kw)
    b = int(np.flatnonzero(status == BAD_OUTSIDE)[2])  # a NaN in row 8
    with pytest.raises(ValueError, match=r"^problem 0: the outside value of row 8 is nan"):
        auction_solve_batch(mats[b:b + 1], shapes=shapes[b:b + 1], outside=outside[b:b + 1], mat_dtype=dtype)


# ---- the call does not wait

def test_the_call_does_not_wait():
    import torch
    rng = np.random.default_rng(60)
    B, N, M = 96, 48, 40
    shapes = np.stack([rng.integers(10, N + 1, B), rng.integers(5, M + 1, B)], axis=1).astype(np.int32)
    mats = _gate(rng, rng.uniform(0, 100, (B, N, M)))
    outside = rng.uniform(20, 60, (B, N))
    p0 = rng.uniform(0, 5, (B, M))
    want = expect(mats, shapes, outside, "min", p0=p0, fast=True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        src = torch.from_numpy(mats).cuda()
        pd, sd, od = torch.from_numpy(p0).cuda(), torch.from_numpy(shapes).cuda(), torch.from_numpy(outside).cuda()
        w = torch.randn(4096, 4096, device="cuda")
        x = src.clone()
        auction_solve_batch(x, shapes=sd, prices=pd, outside=od, errors="status")  # the warm-up call
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
        x.fill_(float("inf"))  # read before the copy below lands, every problem would have status 3
        torch.cuda.synchronize()
        _busy(w, reps)
        x.copy_(src, non_blocking=True)
        t0 = time.perf_counter()
        res = auction_solve_batch(x, shapes=sd, prices=pd, outside=od, errors="status")
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
