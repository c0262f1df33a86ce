"""auction_solve_sparse_batch on a view of the packed arrays, on the GPU (misslap_solve_sparse_batch_status_view /
_outside_view): int32 and int64 indices with any strides, float64 and float32 values, offsets and sizes on the device.

The reference everywhere is the existing call on the compact copy -- int32 (nnz, 2) indices, the values widened to
float64, the same offsets on the host: status, matching_size, sol, prices, outside_prices and every record field, bit for
bit -- and on healthy problems of the lane-edge batch the oracle directly.  Every device input is a slice of a larger
buffer filled with poison (huge indices, NaN values) around and between the view's elements.

  mixed batch   every status code next to healthy neighbours, through every layout, in both modes
  lane edges    rows of 1 .. 129 stored entries, ties, duplicates, the float32 edge values, against the oracle
  int64 range   indices beyond the int32 range saturate: never a valid index
  offsets       unusable slices get code 7 and reach no neighbour
  guard         INFEASIBLE through a view, with the existing call's matching_size
  recipe        nonzero / searchsorted / the call, against per-problem lists extracted on the host
  no wait       with everything on the device and dims the call returns while the stream is busy
  unchanged     contiguous int32 / float64 tensors with host offsets give what they gave
"""
import faulthandler
import functools
import time

import numpy as np
import pytest

from sslap_amd import auction_solve_sparse_batch, batch_meta_to_host, raise_for_status
from tests import _sparse_outside_fixture as ofx
from tests import _sparse_status_fixture as sfx
from tests._batch_shapes import sparse_problem
from tests.test_dense_batch_status import _busy
from tests.test_sparse_batch import _check_problem
from tests.test_sparse_batch_status import _to_host

pytestmark = pytest.mark.gpu

INT_MAX, INT_MIN = 2**31 - 1, -2**31
LAYOUTS = [("int32", "compact"), ("int64", "compact"), ("int64", "wide"), ("int64", "transposed")]
VALUES = ["float64", "float32"]
STRIDES = {"compact": lambda W: (2, 1), "wide": lambda W: (3, 1), "transposed": lambda W: (1, W)}
OUTS = ("status", "matching_size", "sol", "prices", "outside_prices")
PAD = 7


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _lay(loc, val, index, layout, values, pad=PAD):
    """loc (nnz, 2) / val (nnz,) on the device as views of poisoned buffers: the (nnz, 2) slice of a longer array, the
    [:, 1:] of an (nnz, 3) one, or the transpose of two rows of a (3, W) one; the index poison is far beyond every carve
    (and, for int64, beyond the int32 range), the value poison is NaN.  Returns (loc view, val view, the buffers)."""
    import torch
    nnz, W = len(val), len(val) + 2 * pad
    poison = INT_MAX if index == "int32" else 2**40 + 12345
    if layout == "compact":
        buf = np.full((W, 2), poison, dtype=index)
        buf[pad:pad + nnz] = loc
        t = (db := torch.from_numpy(buf).cuda())[pad:pad + nnz]
    elif layout == "wide":
        buf = np.full((W, 3), poison, dtype=index)
        buf[pad:pad + nnz, 1:] = loc
        t = (db := torch.from_numpy(buf).cuda())[pad:pad + nnz, 1:]
    else:
        buf = np.full((3, W), poison, dtype=index)
        buf[1:, pad:pad + nnz] = np.asarray(loc).T
        t = (db := torch.from_numpy(buf).cuda())[1:, pad:pad + nnz].t()
    if nnz > 1:
        assert tuple(t.stride()) == STRIDES[layout](W), (layout, t.stride())
    assert tuple(t.shape) == (nnz, 2)
    vb = np.full(W, np.nan, dtype=values)
    vb[pad:pad + nnz] = val
    v = (dvb := torch.from_numpy(vb).cuda())[pad:pad + nnz]
    return t, v, ((db, buf), (dvb, vb))


def _unwritten(buffers):
    for dev, host in buffers:
        got = dev.cpu().numpy()
        assert np.array_equal(got.view(np.uint8), host.view(np.uint8))


def _cuda(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a)).cuda()  # (a copy: fixtures are read-only)


def _flat(res):
    """The outputs and every record field of a device result as host arrays of raw bits."""
    import torch
    torch.cuda.synchronize()
    out = {k: res[k].cpu().numpy() for k in OUTS if k in res}
    out.update({"meta." + k: v.cpu().numpy() for k, v in res["meta"].items()})
    return {k: (a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a)
            for k, a in out.items()}


def _reference(loc, val, offsets, **kw):
    """The existing call on the compact copy: int32 (nnz, 2), float64, host offsets / sizes; device prices / outside."""
    assert np.asarray(loc).min(initial=0) >= INT_MIN and np.asarray(loc).max(initial=0) <= INT_MAX
    dl, dv = _cuda(np.asarray(loc).astype(np.int32).reshape(-1, 2)), _cuda(np.asarray(val).astype(np.float64))
    for k in ("prices", "outside"):
        if isinstance(kw.get(k), np.ndarray):
            kw[k] = _cuda(kw[k])
    return _flat(auction_solve_sparse_batch(dl, dv, np.asarray(offsets), errors="status", **kw))


def _same(got, want, rows=None, what=""):
    assert set(got) == set(want), (set(got) ^ set(want), what)
    for k, w in want.items():
        g = got[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, what)
        if rows is not None:
            g, w = g[rows], w[rows]
        assert np.array_equal(g, w), (k, what, np.argwhere(g != w)[:5].tolist())


def _view_call(loc, val, offsets, index, layout, values, device_offsets=True, **kw):
    """The call through a view, everything it takes on the device; nothing of the storage is written."""
    t, v, buffers = _lay(loc, val, index, layout, values)
    for k in ("sizes", "prices", "outside"):
        if isinstance(kw.get(k), np.ndarray):
            kw[k] = _cuda(kw[k])
    off = _cuda(np.asarray(offsets, dtype=np.int64)) if device_offsets else np.asarray(offsets)
    res = auction_solve_sparse_batch(t, v, off, errors="status", **kw)
    flat = _flat(res)
    _unwritten(buffers)
    return flat, res


# ---- 1. the mixed batches

@functools.lru_cache(maxsize=None)
def _status_inputs(values):
    fx = sfx.mixed_batch()
    loc, val, offsets = sfx.pack(fx["probs"])
    if values == "float32":
        val = val.astype(np.float32)  # (the fixture's values rounded; the reference gets their widening)
    return fx, loc, val, offsets


@functools.lru_cache(maxsize=None)
def _status_reference(values, fast, check):
    fx, loc, val, offsets = _status_inputs(values)
    return _reference(loc, val, offsets, sizes=fx["sizes"], prices=fx["prices"], fast=fast, cardinality_check=check,
                      max_iter=200, dims=sfx.DIMS)


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("index,layout", LAYOUTS)
def test_mixed_batch(index, layout, values):
    fx, loc, val, offsets = _status_inputs(values)
    for fast in (True, False):
        for check in (True, False):
            want = _status_reference(values, fast, check)
            # (int64 compact: host offsets, sent for the call; everything else: offsets on the device)
            got, _ = _view_call(loc, val, offsets, index, layout, values, device_offsets=(index, layout) != ("int64", "compact"),
                                sizes=fx["sizes"], prices=fx["prices"], fast=fast, cardinality_check=check, max_iter=200,
                                dims=sfx.DIMS)
            _same(got, want, what=(fast, check))
            if fast and check and values == "float64":  # the batch holds every code, as the fixture planted them
                assert np.array_equal(got["status"], fx["kinds"]) and set(got["status"]) == set(sfx.ORDER) | {0}


def _outside_forms(fx):
    full = fx["outside"]
    per_problem = np.where(np.isfinite(full[:, 0]), full[:, 0], 33.0)
    return {"float": 35.5, "per_problem": per_problem, "per_row": full}


@functools.lru_cache(maxsize=None)
def _outside_reference(values, with_sizes, form):
    fx = ofx.mixed(with_sizes)
    val = fx["val"].astype(values)
    return _reference(fx["loc"], val, fx["offsets"], sizes=fx["sizes"], prices=np.array(fx["prices"]), dims=ofx.V_DIMS,
                      outside=_outside_forms(fx)[form])


@pytest.mark.parametrize("values", VALUES)
@pytest.mark.parametrize("index,layout", LAYOUTS)
def test_mixed_batch_with_outside(index, layout, values):
    for with_sizes in (True, False):
        fx = ofx.mixed(with_sizes)
        val = fx["val"].astype(values)
        for form, outside in _outside_forms(fx).items():
            want = _outside_reference(values, with_sizes, form)
            got, _ = _view_call(fx["loc"], val, fx["offsets"], index, layout, values, sizes=fx["sizes"],
                                prices=np.array(fx["prices"]), dims=ofx.V_DIMS, outside=outside)
            _same(got, want, what=(with_sizes, form))
            if form == "per_row" and values == "float64":
                assert np.array_equal(got["status"], fx["kinds"])


# ---- 2. lane edges, against the oracle

FLT_MAX, FLT_SUBNORMAL = float(np.finfo(np.float32).max), float(np.float32(1e-45))
LENS = (1, 63, 64, 65, 128, 129)


def _lane_edge_problems():
    """Three problems of six rows of 1, 63, 64, 65, 128 and 129 stored entries over 130 columns, a perfect matching
    planted: integer values with ties and repeated maxima across the lane wrap, duplicate (i, j) entries, and float32
    values with -0.0, the largest finite float32 and a subnormal."""
    rng = np.random.default_rng(77)
    m, probs = 130, []
    for kind in ("ints", "duplicates", "edges"):
        planted = rng.permutation(m)[:len(LENS)]
        rows, cols = [], []
        for i, k in enumerate(LENS):
            c = rng.integers(0, m, k) if kind == "duplicates" else rng.choice(m, k, replace=False)
            if planted[i] not in c:
                c[int(rng.integers(0, k))] = planted[i]
            if kind == "duplicates" and k > 2:
                c[-1], c[k // 2] = c[0], c[0]  # the same (i, j) in the first, a middle and the last stored position
            rows.append(np.full(k, i))
            cols.append(c)
        loc = np.stack([np.concatenate(rows), np.concatenate(cols)], axis=1).astype(np.int32)
        val = rng.integers(0, 4, loc.shape[0]).astype(np.float64)  # ties, and repeated maxima 64 entries apart
        if kind == "edges":
            val = rng.uniform(0, 50, loc.shape[0]).astype(np.float32).astype(np.float64)
            at = np.flatnonzero(loc[:, 0] == 5)
            val[at[0]], val[at[64]], val[at[128]] = -0.0, FLT_SUBNORMAL, FLT_MAX
            val[np.flatnonzero(loc[:, 0] == 3)[64]] = -0.0  # in the wrapped lane of a 65-entry row
        assert np.array_equal(val.astype(np.float32).astype(np.float64), val)
        probs.append((np.ascontiguousarray(loc), val))
    assert [np.bincount(lo[:, 0]).tolist() for lo, _ in probs] == [list(LENS)] * 3
    assert np.unique(probs[1][0], axis=0).shape[0] < probs[1][0].shape[0]
    return probs


@pytest.mark.parametrize("problem", ["min", "max"])
def test_lane_edges_against_the_oracle(problem):
    probs = _lane_edge_problems()
    loc, val, offsets = sfx.pack(probs)
    for index, layout, values in (("int64", "wide", "float32"), ("int64", "transposed", "float64"),
                                  ("int32", "compact", "float32")):
        _, res = _view_call(loc, val, offsets, index, layout, values, problem=problem, dims=(6, 130))
        host = _to_host(res)
        assert (host["status"] == 0).all() and (host["matching_size"] == 6).all(), (layout, host["status"])
        for b, (lo, va) in enumerate(probs):
            _check_problem(host, b, lo, va, problem)


# ---- 3. indices beyond the int32 range

@pytest.mark.parametrize("outside", [None, 40.0])
@pytest.mark.parametrize("layout", ["compact", "wide", "transposed"])
def test_int64_indices_saturate(layout, outside):
    rng = np.random.default_rng(5)
    probs = [sfx.healthy(rng, int(rng.integers(5, 12)), 14) for _ in range(9)]
    probs = [(lo.astype(np.int64), va) for lo, va in probs]
    rows = [int(lo[:, 0].max()) + 1 for lo, _ in probs]
    probs[1][0][3, 1] = 2**32 + 3       # not column 3
    probs[3][0][-1, 0] = 2**31          # the last stored row
    probs[5][0][2, 1] = -(2**32) + 1    # its low word is 1
    probs[7][0][4, 0] = -(2**31) - 1    # its low word is INT_MAX
    loc = np.concatenate([lo for lo, _ in probs])
    val = np.concatenate([va for _, va in probs])
    offsets = np.concatenate([[0], np.cumsum([len(va) for _, va in probs])])
    sizes = np.array([[14, n] for n in rows])
    # (the outside mode without sizes: with them a last row beyond sizes[b, 1] is BAD_SHAPE before it is TOO_LARGE)
    kw = dict(dims=sfx.DIMS, max_iter=200, outside=outside) if outside is not None else \
        dict(dims=sfx.DIMS, max_iter=200, sizes=sizes)
    got, res = _view_call(loc, val, offsets, "int64", layout, "float64", **kw)
    status = got["status"].tolist()
    assert status[0::2] == [0] * 5
    assert status[1] == sfx.TOO_LARGE and status[5] == status[7] == sfx.NEGATIVE_INDEX
    # a last row at 2^31: beyond every carve where a row gap is legal (the outside mode); in the plain mode INT_MAX is
    # first of all a row that does not follow its predecessor, as it is in the existing call
    assert status[3] == (sfx.TOO_LARGE if outside is not None else sfx.ROW_GAP)
    assert (got["sol"][1::2] == -1).all() and not got["prices"][1::2].any()
    # the whole call is the existing call on the saturated indices ...
    _same(got, _reference(loc.clip(INT_MIN, INT_MAX), val, offsets, **kw))
    # ... and every healthy neighbour is what it is alone
    for b in range(0, 9, 2):
        solo = _reference(probs[b][0], probs[b][1], np.array([0, len(probs[b][1])]), **(dict(kw, sizes=sizes[b:b + 1]) if outside is None else kw))
        for k, w in solo.items():
            assert np.array_equal(got[k][b], w[0]), (b, k)
    with pytest.raises(ValueError, match=r"^problem 1: column index too large"):
        raise_for_status(res)


# ---- 4. offsets that nobody checked

def _offset_cases(t, nnz):
    cases = {}
    for name, edits in (("decreasing", {3: t[2] - 2}), ("beyond nnz", {4: nnz + 5}), ("negative", {2: -3}),
                        ("huge", {1: 2**40}), ("empty slice", {5: t[4]}), ("loose ends", {0: 1, 6: nnz - 1})):
        o = t.copy()
        for k, v in edits.items():
            o[k] = v
        cases[name] = o
    return cases


@pytest.mark.parametrize("outside", [None, 25.0])
def test_unusable_slices_get_code_7_and_reach_nobody(outside):
    rng = np.random.default_rng(9)
    probs = [sfx.healthy(rng, int(rng.integers(5, 12)), 14) for _ in range(6)]
    loc, val, true = sfx.pack(probs)
    nnz = len(val)
    kw = dict(dims=sfx.DIMS, max_iter=200)
    if outside is not None:
        kw["outside"] = outside
    seen = set()
    for name, off in _offset_cases(true, nnz).items():
        got, res = _view_call(loc, val, off, "int64", "wide", "float32" if outside is None else "float64", **kw)
        bad = [not (0 <= off[b] <= off[b + 1] <= nnz) for b in range(6)]
        assert any(bad) == (name not in ("empty slice", "loose ends")), name
        for b in range(6):
            if bad[b]:  # code 7, the condemned outputs, an all-zero record
                assert got["status"][b] == 7 and got["matching_size"][b] == -1, (name, b)
                assert (got["sol"][b] == -1).all() and not got["prices"][b].any(), (name, b)
                assert all(not got[k][b].any() for k in got if k.startswith("meta.") or k == "outside_prices"), (name, b)
                continue
            lo, va = loc[off[b]:off[b + 1]], val[off[b]:off[b + 1]]
            solo = _reference(lo, va.astype(np.float32 if outside is None else np.float64), np.array([0, len(va)]), **kw)
            for k, w in solo.items():
                assert np.array_equal(got[k][b], w[0]), (name, b, k)
            seen.add(int(got["status"][b]))
        if any(bad):
            first = bad.index(True)
            with pytest.raises(ValueError, match=rf"^problem {first}: offsets\[{first}\] \.\. offsets\[{first + 1}\] = "
                                                 rf"{off[first]} \.\. {off[first + 1]} is not a slice of the {nnz} packed"):
                raise_for_status(res)
    assert {0, sfx.NO_ENTRIES} <= seen  # healthy neighbours, and the empty slice is NO_ENTRIES as before


# ---- 5. the guard through a view

def test_guard_through_the_transposed_view():
    rng = np.random.default_rng(21)
    ok = sparse_problem(rng, 40, 45, 6)
    lo, va = sparse_problem(rng, 40, 45, 6)
    lo = lo.copy()
    lo[lo[:, 0] < 9, 1] = lo[lo[:, 0] < 9, 1] % 5  # nine rows share five columns: at most 36 rows can be matched
    probs = [ok, (lo, va), sparse_problem(rng, 12, 12, 3)]
    loc, val, offsets = sfx.pack(probs)
    kw = dict(cardinality_check=True, dims=(40, 45))
    want = _reference(loc, val, offsets, **kw)
    got, _ = _view_call(loc, val, offsets, "int64", "transposed", "float64", **kw)
    _same(got, want)
    assert got["status"].tolist() == [0, sfx.INFEASIBLE, 0]
    assert got["matching_size"][0] == 40 and got["matching_size"][2] == 12 and 0 < got["matching_size"][1] < 40
    off, _ = _view_call(loc, val, offsets, "int64", "transposed", "float64", cardinality_check=False, dims=(40, 45))
    assert off["status"].tolist() == [0, 0, 0] and (off["matching_size"] == -1).all()


# ---- 6. the recipe, end to end

META = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj_f64", "start_eps_f32", "final_eps_f32", "n_rows",
        "n_cols", "nnz", "bids_made")


@pytest.mark.parametrize("cost_limit", [None, 0.75])
def test_the_recipe_end_to_end(cost_limit):
    import torch
    B, N, M = 5, 6, 7
    rng = np.random.default_rng(3)
    cost_h = rng.uniform(0, 1, (B, N, M)).astype(np.float32)
    gate_h = rng.random((B, N, M)) < 0.35
    for b in range(B):
        gate_h[b, np.arange(N), rng.permutation(M)[:N]] = True  # a matching of every row
    gate_h[3] = False        # a problem gated off entirely
    gate_h[1, 2] = False     # a row gated off entirely
    cost, gate = torch.from_numpy(cost_h).cuda(), torch.from_numpy(gate_h).cuda()
    kw = dict(dims=(N, M), errors="status")
    if cost_limit is not None:
        kw["outside"] = cost_limit

    idx = gate.nonzero()  # (nnz, 3) int64: b, i, j, sorted
    off = torch.searchsorted(idx[:, 0].contiguous(), torch.arange(B + 1, device=idx.device))
    # (whatever strides nonzero() chose: torch lays a device result out column by column, so the slice is a transposed view)
    assert idx.dtype == torch.int64 and off.dtype == torch.int64 and tuple(idx.shape) == (int(gate_h.sum()), 3)
    res = auction_solve_sparse_batch(idx[:, 1:], cost[gate], off, **kw)

    pairs = []
    for b in range(B):  # the same problems, extracted on the host
        i, j = np.nonzero(gate_h[b])
        pairs.append((np.stack([i, j], axis=1).astype(np.int32), cost_h[b][gate_h[b]].astype(np.float64)))
    want = auction_solve_sparse_batch(pairs, **kw)
    torch.cuda.synchronize()
    meta = batch_meta_to_host(res)
    for k in OUTS:
        if k in want:
            g = res[k].cpu().numpy()
            assert g.dtype == want[k].dtype and np.array_equal(g.view(np.uint8), want[k].view(np.uint8)), k
    for k in META:
        assert np.array_equal(meta[k], want["meta"][k]), k
    if cost_limit is None:
        assert want["status"].tolist() == [0, sfx.ROW_GAP, 0, sfx.NO_ENTRIES, 0]
    else:
        assert want["status"].tolist() == [0, 0, 0, sfx.NO_ENTRIES, 0] and want["sol"][1, 2] == -1
        assert "outside_prices" in res


# ---- 7. no wait

def _run_behind_busy_stream(stream, outside):
    import torch
    rng = np.random.default_rng(31)
    probs = [sparse_problem(rng, int(rng.integers(10, 48)), 48, 7) for _ in range(96)]
    loc, val, offsets = sfx.pack(probs)
    sizes = np.array([[48, int(lo[:, 0].max()) + 1] for lo, _ in probs])
    p0 = rng.uniform(0, 5, (96, 48))
    kw = dict(fast=True, dims=(48, 48))
    want = _reference(loc, val.astype(np.float32), offsets, sizes=sizes, prices=p0, **dict(kw, **outside))
    with torch.cuda.stream(stream):
        idx = torch.from_numpy(np.concatenate([np.zeros((len(val), 1), dtype=np.int64), loc], axis=1)).cuda()
        vsrc = torch.from_numpy(val.astype(np.float32)).cuda()
        dkw = dict(kw, sizes=_cuda(sizes), prices=_cuda(p0), errors="status",
                   **{k: _cuda(np.full(96, v)) for k, v in outside.items()})
        d_off = _cuda(offsets)
        w = torch.randn(4096, 4096, device="cuda")
        lx, vx = idx[:, 1:], vsrc.clone()
        auction_solve_sparse_batch(lx, vx, d_off, **dkw)  # the warm-up call
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
        res = auction_solve_sparse_batch(lx, vx, d_off, **dkw)
        t_call = (time.perf_counter() - t0) * 1e3
        pending = not stream.query()
        torch.cuda.synchronize()
    print(f"queued work {D:.1f} ms, host time of the call {t_call:.3f} ms, stream busy at return: {pending}")
    assert t_call < D / 4, (t_call, D)
    assert pending  # the producer chain was still running when the call came back
    got = _flat(res)
    assert (got["status"] == 0).all()
    _same(got, want)


@pytest.mark.parametrize("outside", [{}, {"outside": 60.0}], ids=["status", "outside"])
def test_the_call_does_not_wait_on_the_null_stream(outside):
    import torch
    _run_behind_busy_stream(torch.cuda.default_stream(), outside)


@pytest.mark.parametrize("outside", [{}, {"outside": 60.0}], ids=["status", "outside"])
def test_the_call_does_not_wait_on_a_side_stream(outside):
    import torch
    _run_behind_busy_stream(torch.cuda.Stream(), outside)


# ---- 8. unchanged paths

def test_contiguous_tensors_with_host_offsets_take_the_calls_they_took(monkeypatch):
    from sslap_amd import _lib
    fx, loc, val, offsets = _status_inputs("float64")
    lib, names = _lib.load(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("misslap_solve_"):
                names.append(name)
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    kw = dict(sizes=fx["sizes"], prices=fx["prices"], fast=True, max_iter=200, dims=sfx.DIMS)
    got = _reference(loc, val, offsets, **kw)
    assert names == ["misslap_solve_sparse_batch_status"]
    assert np.array_equal(got["status"], fx["kinds"])
    _same(got, _status_reference("float64", True, True))
    _view_call(loc, val, offsets, "int32", "compact", "float64", **kw)  # device offsets alone: the view entry point
    assert names[1:] == ["misslap_solve_sparse_batch_status_view"]
    ofxx = ofx.mixed(True)
    _reference(ofxx["loc"], ofxx["val"], ofxx["offsets"], sizes=ofxx["sizes"], dims=ofx.V_DIMS, outside=30.0)
    assert names[2:] == ["misslap_solve_sparse_batch_outside"]
    # the default mode on healthy problems: its own entry point, its own result
    good = fx["probs"][0:16:2]
    gl, gv, go = sfx.pack(good)
    res = auction_solve_sparse_batch(_cuda(gl), _cuda(gv), go)
    assert names[3:] == ["misslap_solve_sparse_batch"] and set(res) == {"sol", "prices", "meta"}
    # ... which reads offsets on the host: on the device they are taken with errors="status" or outside=, and with dims
    with pytest.raises(TypeError, match=r"^offsets on the device are taken with errors='status' or with outside= \(and "
                                        r"dims=\): the default mode reads offsets on the host$"):
        auction_solve_sparse_batch(_cuda(gl), _cuda(gv), _cuda(go))
    with pytest.raises(ValueError, match=r"^offsets on the device need dims=\(Nmax, Mmax\): sizing the outputs from loc "
                                         r"would read it back, and no wait may hide in this call$"):
        auction_solve_sparse_batch(_cuda(gl), _cuda(gv), _cuda(go), errors="status")
    # a view in the default mode: the status call, then raise_for_status
    t, v, _ = _lay(gl, gv, "int64", "wide", "float32")
    res = auction_solve_sparse_batch(t, v, go)
    assert names[4:] == ["misslap_solve_sparse_batch_status_view"] and (res["status"] == 0).all()
    t, v, _ = _lay(loc, val, "int64", "wide", "float64")
    with pytest.raises(ValueError, match=r"^problem 1: no entries$"):
        auction_solve_sparse_batch(t, v, offsets, sizes=fx["sizes"])
