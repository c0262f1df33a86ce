"""Strided device stacks on the GPU: auction_solve_batch and hopcroft_solve_batch(mats=) read a transposed view, a slice
of a wider buffer or an expanded matrix where it lies (misslap_solve_dense_batch_status_strided,
misslap_solve_dense_batch_outside_strided, misslap_matching_dense_batch_strided).

One method for every case:
  1. the view is built inside a larger storage whose every element outside the view is +inf: a stray read condemns the
     problem (INFINITE_VALUE) or changes C;
  2. the call runs on the view and on view.contiguous();
  3. every output (sol, prices, outside_prices, status, matching_size, every meta field) is compared with == on the bits;
  4. float64 problems of at most 300 rows are also compared with the oracle (dense_expect / dense_compare);
  5. afterwards the bytes of the whole storage are what they were.

The shapes sit at the edges of both bid mappings of the strided row source (csrc/kernels_dense_batch.hpp: the wavefront
scan, and for a transposed view one lane per person in rounds of at least LANE_MIN_K bidders) and of the workgroup
sizes.  A 65 x 130 solve starts with 65 bidders (one lane per person) and goes on with fewer (the wavefront scan), so
both mappings and the switch between them run in one solve.
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import _lib, auction_solve_batch, batch_meta_to_host, hopcroft_solve_batch
from tests._batch_shapes import dense_compare, dense_expect, dense_values, host, shape_id

pytestmark = pytest.mark.gpu

LANE_MIN_K = 64  # kStridedLaneMinK (csrc/abi_dense_batch.hpp): 63 x 64 stays below it, 64 x 64 and 65 x 130 cross it
KINDS = ("uniform", "ints", "holes")
DTYPES = ("float64", "float32", "float16", "bfloat16")
ORACLE_ROWS = 300


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- the layouts: (storage shape, view of the storage) for a (B, N, M) stack ------------------------------------------------
LAYOUTS = {
    # persons run along the unit stride: sN = 1, sM = N + 2
    "transposed": lambda B, N, M: ((B, M + 1, N + 2), lambda s: s[:, :M, :N].transpose(1, 2)),
    # unit last stride
    "cols": lambda B, N, M: ((B, N, M + 7), lambda s: s[:, :, 3:3 + M]),
    "rows": lambda B, N, M: ((B, N + 3, M), lambda s: s[:, 1:1 + N]),
    "batch": lambda B, N, M: ((2 * B, N, M), lambda s: s[::2]),
    "padded": lambda B, N, M: ((B, N, M + 10), lambda s: s[:, :, :M]),
    # neither stride is 1
    "generic": lambda B, N, M: ((B, 2 * N, 3 * M), lambda s: s[:, ::2, ::3]),
}


def make_view(vals, layout, dtype="float64"):
    """(storage, view): vals (float64 numpy (B, N, M)) rounded to dtype, inside a storage of +inf."""
    import torch
    B, N, M = vals.shape
    shape, of = LAYOUTS[layout](B, N, M)
    storage = torch.full(shape, float("inf"), dtype=getattr(torch, dtype), device="cuda")
    view = of(storage)
    assert tuple(view.shape) == (B, N, M) and not view.is_contiguous(), (layout, view.stride())
    view.copy_(torch.from_numpy(vals).to(getattr(torch, dtype)))
    return storage, view


def storage_bytes(t):
    import torch
    flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    return flat.cpu().numpy().tobytes()


def same_bits(a, b, what):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape and a.is_cuda and b.is_cuda, what
    as_int = {torch.float64: torch.int64, torch.float32: torch.int32}
    if a.dtype in as_int:
        a, b = a.contiguous().view(as_int[a.dtype]), b.contiguous().view(as_int[b.dtype])
    assert torch.equal(a, b), what


def same_result(got, want):
    keys = ["sol", "prices", "status", "matching_size"] + (["outside_prices"] if "outside_prices" in want else [])
    assert ("outside_prices" in got) == ("outside_prices" in want)
    for k in keys:
        same_bits(got[k], want[k], k)
    assert set(got["meta"]) == set(want["meta"])
    for k in want["meta"]:
        same_bits(got["meta"][k], want["meta"][k], k)


def to_host(res):
    return dict(sol=host(res["sol"]), prices=host(res["prices"]), status=host(res["status"]),
                matching_size=host(res["matching_size"]), meta=batch_meta_to_host(res))


def solve_pair(storage, view, **kw):
    """The call on the view and on its compact copy: equal on every bit, and the storage is left as it was."""
    before = storage_bytes(storage)
    kw.setdefault("errors", "status")
    got = auction_solve_batch(view, **kw)
    want = auction_solve_batch(view.contiguous(), **kw)
    same_result(got, want)
    assert storage_bytes(storage) == before
    return got


def oracle_check(res, vals, problem, shapes=None, prices=None, **kw):
    """The float64 problems of at most ORACLE_ROWS rows against the oracle."""
    h = to_host(res)
    for b in range(vals.shape[0]):
        n, m = (vals.shape[1:] if shapes is None else (int(x) for x in shapes[b]))
        if h["status"][b] != 0 or n > ORACLE_ROWS:
            continue
        p0 = None if prices is None else prices[b]
        dense_compare(h, b, dense_expect(vals[b, :n, :m], problem, p0=p0, **kw), n, m, p0=p0)


def kinds_stack(N, M, seed):
    return np.stack([dense_values(kind, (N, M), np.random.default_rng([seed, N, M, k])) for k, kind in enumerate(KINDS)])


# ---- 1. transposed views at the edges of both bid mappings and of the workgroup sizes --------------------------------------
TRANSPOSED_SHAPES = [(1, 1), (1, 65), (2, 64), (63, 64), (64, 64), (65, 130), (257, 300), (513, 520)]
assert any(n < LANE_MIN_K for n, _ in TRANSPOSED_SHAPES) and any(n > LANE_MIN_K for n, _ in TRANSPOSED_SHAPES)


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("shape", TRANSPOSED_SHAPES, ids=shape_id)
def test_transposed_view(shape, problem):
    vals = kinds_stack(*shape, seed=11)
    storage, view = make_view(vals, "transposed")
    assert view.stride(1) == 1
    res = solve_pair(storage, view, problem=problem)
    assert (host(res["status"]) == 0).all()
    oracle_check(res, vals, problem)


def test_transposed_view_at_the_cap():
    vals = dense_values("uniform", (1, 1024, 1024), np.random.default_rng(12))
    storage, view = make_view(vals, "transposed")
    res = solve_pair(storage, view, problem="max", cardinality_check=False)
    assert host(res["status"])[0] == 0 and batch_meta_to_host(res)["n_assigned"][0] == 1024


RAGGED = np.array([[65, 130], [1, 1], [30, 64], [64, 65], [2, 129]], dtype=np.int32)


@pytest.mark.parametrize("device_shapes", [False, True], ids=["host_shapes", "device_shapes"])
def test_transposed_view_with_ragged_shapes(device_shapes):
    import torch
    rng = np.random.default_rng(13)
    shapes = RAGGED.copy()
    vals = np.full((len(shapes), 65, 130), np.inf)  # the rest of the view is not the problem's either
    for b, (n, m) in enumerate(shapes):
        vals[b, :n, :m] = dense_values(KINDS[b % 3], (int(n), int(m)), rng)
    if device_shapes:  # only a device shapes array can hold a bad entry: the host's is checked before the call
        shapes[2] = (66, 10)
    storage, view = make_view(vals, "transposed")
    arg = torch.from_numpy(shapes).cuda() if device_shapes else shapes
    res = solve_pair(storage, view, shapes=arg)
    want = np.zeros(len(shapes), dtype=np.int32)
    if device_shapes:
        want[2] = _lib.BATCH_STATUS_BAD_SHAPE
    assert np.array_equal(host(res["status"]), want)
    oracle_check(res, vals, "min", shapes=shapes)


# ---- 2. a unit last stride, and no unit stride at all ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_slice_in_every_element_type(dtype):
    vals = kinds_stack(65, 130, seed=21)
    storage, view = make_view(vals, "cols", dtype)  # 3 elements into a row: aligned to the element only
    assert view.storage_offset() == 3 and view.stride(2) == 1
    res = solve_pair(storage, view, mat_dtype=dtype, problem="max")
    assert (host(res["status"]) == 0).all()
    oracle_check(res, view.double().cpu().numpy(), "max")


@pytest.mark.parametrize("layout", ["rows", "batch", "padded", "generic"])
def test_slices_of_a_wider_buffer(layout):
    vals = kinds_stack(65, 130, seed=22)
    storage, view = make_view(vals, layout)
    res = solve_pair(storage, view)
    assert (host(res["status"]) == 0).all()
    oracle_check(res, vals, "min")


def test_expanded_matrix_from_four_starting_prices():
    import torch
    rng = np.random.default_rng(23)
    N, M = 65, 130
    one = torch.from_numpy(dense_values("uniform", (N, M), rng)).cuda()
    prices = rng.uniform(0, 30, (4, M))
    prices[0] = 0.0
    view = one.expand(4, N, M)
    assert view.stride(0) == 0
    before = storage_bytes(one)
    res = auction_solve_batch(view, prices=prices, errors="status", eps_start=0.5)
    assert storage_bytes(one) == before
    sols = set()
    for b in range(4):
        want = auction_solve_batch(one[None], prices=prices[b:b + 1], errors="status", eps_start=0.5)
        for k in ("sol", "prices", "status", "matching_size"):
            same_bits(res[k][b:b + 1], want[k], (b, k))
        for k in want["meta"]:
            same_bits(res["meta"][k][b:b + 1], want["meta"][k], (b, k))
        sols.add(host(res["prices"])[b].tobytes())
    assert len(sols) == 4  # four different results
    oracle_check(res, one.cpu().numpy()[None].repeat(4, axis=0), "min", prices=prices, eps_start=0.5)


# ---- 3. the modes, on the transposed stack and on a column slice ------------------------------------------------------------
MODE_LAYOUTS = ["transposed", "cols"]


@pytest.mark.parametrize("layout", MODE_LAYOUTS)
def test_guard_reads_the_strided_stack(layout):
    vals = kinds_stack(65, 130, seed=31)
    vals[1, :, :] = -1.0  # rows 0 and 1 can only take column 7, every other row its own column: 64 of 65 rows match
    vals[1, np.arange(2, 65), np.arange(2, 65) + 10] = 5.0
    vals[1, :2, 7] = 3.0
    storage, view = make_view(vals, layout)
    res = solve_pair(storage, view, cardinality_check=True)
    assert host(res["status"]).tolist() == [0, _lib.BATCH_STATUS_INFEASIBLE, 0]
    assert host(res["matching_size"]).tolist() == [65, 64, 65]
    oracle_check(res, vals, "min")


@pytest.mark.parametrize("layout", MODE_LAYOUTS)
def test_outside_option(layout):
    rng = np.random.default_rng(32)
    vals = kinds_stack(65, 130, seed=32)
    vals[rng.random(vals.shape) < 0.5] = -1.0  # half the entries gated
    vals[0, 5, :] = -1.0                        # a fully gated row
    shapes = np.array([[65, 130], [65, 20], [40, 130]], dtype=np.int32)  # problem 1: n_b > m_b
    outside = rng.uniform(20, 60, (3, 65))
    storage, view = make_view(vals, layout)
    for kw in (dict(), dict(problem="max", prices=rng.uniform(0, 5, (3, 130)))):
        res = solve_pair(storage, view, shapes=shapes, outside=outside, **kw)
        assert (host(res["status"]) == 0).all()
        sol = host(res["sol"])
        assert sol[0, 5] == -1 and (sol[1, :65] == -1).sum() >= 45  # the gated row and the rows without a column stay out


@pytest.mark.parametrize("layout", MODE_LAYOUTS)
def test_errors_raise_is_the_contiguous_message(layout):
    vals = kinds_stack(65, 130, seed=33)
    storage, view = make_view(vals, layout)
    res = auction_solve_batch(view)  # nothing to raise: the status-mode result
    same_result(res, auction_solve_batch(view.contiguous(), errors="status"))
    vals[2, 17, :] = np.nan  # an empty row in problem 2
    storage, view = make_view(vals, layout)
    before = storage_bytes(storage)
    with pytest.raises(ValueError) as strided:
        auction_solve_batch(view)
    with pytest.raises(ValueError) as compact:
        auction_solve_batch(view.contiguous())
    assert str(strided.value) == str(compact.value) and str(compact.value).startswith("problem 2: every row must have")
    with pytest.raises(ValueError) as outside:
        auction_solve_batch(view, outside=np.array([1.0, -2.0, 1.0]))
    with pytest.raises(ValueError) as outside_compact:
        auction_solve_batch(view.contiguous(), outside=np.array([1.0, -2.0, 1.0]))
    assert str(outside.value) == str(outside_compact.value) and str(outside.value).startswith("problem 1: the outside")
    assert storage_bytes(storage) == before


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_view_in_every_element_type(dtype):
    vals = kinds_stack(65, 130, seed=34)
    storage, view = make_view(vals, "transposed", dtype)
    res = solve_pair(storage, view, mat_dtype=dtype)
    assert (host(res["status"]) == 0).all()
    oracle_check(res, view.double().cpu().numpy(), "min")


@pytest.mark.parametrize("layout", MODE_LAYOUTS)
@pytest.mark.parametrize("opts", [dict(fast=True), dict(eps_start=0.5), dict(max_iter=3)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options(layout, opts):
    vals = kinds_stack(65, 130, seed=35)
    storage, view = make_view(vals, layout)
    res = solve_pair(storage, view, problem="max", **opts)
    oracle_check(res, vals, "max", **opts)


@pytest.mark.parametrize("layout", MODE_LAYOUTS + ["generic"])
def test_hopcroft_solve_batch_reads_the_view(layout):
    import torch
    vals = kinds_stack(65, 130, seed=36)
    vals[np.random.default_rng(36).random(vals.shape) < 0.9] = -1.0  # sparse graphs: the DFS recurses and backtracks
    shapes = np.array([[65, 130], [40, 9], [1, 1]])
    storage, view = make_view(vals, layout)
    before = storage_bytes(storage)
    for shp in (None, shapes):
        got = hopcroft_solve_batch(mats=view, shapes=shp)
        want = hopcroft_solve_batch(mats=view.contiguous(), shapes=shp)
        assert np.array_equal(got["size"], want["size"]) and got["size"][0] > 0
        for k in ("left_pairings", "right_pairings"):
            assert torch.equal(got[k], want[k]), k
        for k in ("n_rows", "n_cols"):
            assert np.array_equal(got[k], want[k]), k
    assert storage_bytes(storage) == before
