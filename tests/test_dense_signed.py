"""Signed dense stacks on the GPU: auction_solve_batch(entries="finite") and hopcroft_solve_batch(mats=,
entries="finite"), where an element is an entry iff it is not a NaN (MISSLAP_DENSE_ENTRIES_FINITE; the finite-mode
instances of the strided kernel family, csrc/kernels_dense_batch.hpp).

Every problem with status 0 is compared with `==` on every bit with the oracle on dense_to_packed's (loc_b, val_b)
(tests/_dense_signed.py: packed_expect); every condemned problem has exactly its status, its matching_size and the
zeroed outputs.  The verdicts are derived on the CPU from the packed problems and the host matcher alone.  All cases
travel in a handful of batches with errors="status" and an explicit max_iter.  Whatever lies outside a problem's slice
or outside a view is -inf (an entry under this rule: a stray read condemns the problem) unless a case says otherwise.
"""
import faulthandler
import functools

import numpy as np
import pytest

from sslap_amd import (_lib, auction_solve_batch, batch_meta_to_host, dense_to_packed, hopcroft_solve, hopcroft_solve_batch,
                       sparse_to_augmented)
from tests import test_ell_outside as ell_out
from tests._batch_shapes import bits, dense_compare, dense_expect, host, sparse_expect
from tests._dense_signed import (BAD_OUTSIDE, BAD_SHAPE, EMPTY_ROW, INFEASIBLE, INFINITE_VALUE, OK, PRICE_NEGATIVE,
                                 PRICE_NOT_FINITE, TOO_FEW_VALUES, expected_status, packed_expect, signed_ints,
                                 signed_uniform)
from tests.test_ell_batch import ZERO_META

pytestmark = pytest.mark.gpu

LANE_MIN_K = 64  # kStridedLaneMinK (csrc/abi_dense_batch.hpp), as tests/test_dense_strided.py takes it
MAX_ITER = 200000
PROBLEMS = ("min", "max")
DTYPES = ("float64", "float32", "float16", "bfloat16")
POISON = -np.inf


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- layouts of a (B, N, M) stack on the device: (storage, view) ------------------------------------------------------------
LAYOUTS = {
    "contiguous": lambda B, N, M: ((B, N, M), lambda s: s),
    "transposed": lambda B, N, M: ((B, M + 1, N + 2), lambda s: s[:, :M, :N].transpose(1, 2)),  # sN = 1
    "cols": lambda B, N, M: ((B, N, M + 7), lambda s: s[:, :, 3:3 + M]),                         # sM = 1
    "generic": lambda B, N, M: ((B, 2 * N, 3 * M), lambda s: s[:, ::2, ::3]),                    # neither stride is 1
}


def on_device(vals, layout="contiguous", dtype="float64", poison=POISON):
    """(storage, view): vals (float64 numpy (B, N, M)) in dtype on the device, inside a storage of `poison`."""
    import torch
    shape, of = LAYOUTS[layout](*vals.shape)
    storage = torch.full(shape, poison, dtype=getattr(torch, dtype), device="cuda")
    view = of(storage)
    assert tuple(view.shape) == vals.shape and view.is_contiguous() == (layout == "contiguous")
    view.copy_(torch.from_numpy(np.array(vals)).to(getattr(torch, dtype)))  # (a copy: torch takes no read-only array)
    return storage, view


def storage_bytes(t):
    import torch
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).cpu().numpy().tobytes()


def to_host(res):
    if isinstance(res["sol"], np.ndarray):
        return res
    out = dict(res, meta=batch_meta_to_host(res))
    for k in ("sol", "prices", "status", "matching_size") + (("outside_prices",) if "outside_prices" in res else ()):
        assert res[k].is_cuda, k
        out[k] = host(res[k])
    return out


def stack_of(probs, N, M, fill=POISON):
    mats = np.full((len(probs), N, M), fill)
    for b, p in enumerate(probs):
        mats[b, :p.shape[0], :p.shape[1]] = p
    return mats, np.array([p.shape for p in probs], dtype=np.int32)


def condemned(h, b, n_rows, n_cols, nnz):
    """The defined outputs of a problem that was not solved."""
    assert (h["sol"][b] == -1).all() and (bits(h["prices"][b]) == 0).all(), b
    if "outside_prices" in h:
        assert (bits(h["outside_prices"][b]) == 0).all(), b
    meta = h["meta"]
    assert (meta["n_rows"][b], meta["n_cols"][b], meta["nnz"][b]) == (n_rows, n_cols, nnz), b
    for k in ZERO_META:
        assert meta[k][b] == 0, (b, k)


def check(res, wide, shapes, problem, prices=None, guard=True, want=None, **opts):
    """A finite-mode result against the definition.  wide: the stack's values widened to float64 (numpy); want: cached
    packed_expect values per problem (None where condemned).  Returns the statuses."""
    h = to_host(res)
    B, N, M = wide.shape
    shp = np.tile([N, M], (B, 1)) if shapes is None else np.asarray(shapes)
    safe = np.where((shp[:, :1] >= 1) & (shp[:, :1] <= N) & (shp[:, 1:] >= 1) & (shp[:, 1:] <= M), shp, 0)
    packed = dense_to_packed(wide, safe, entries="finite")
    status, size = expected_status(packed, shp, (N, M), prices, guard)
    assert h["status"].dtype == np.int32 and h["status"].tolist() == status.tolist()
    assert h["matching_size"].tolist() == size.tolist()
    for b, (loc, val) in enumerate(packed):
        n, m = (int(x) for x in safe[b])
        if status[b] != OK:
            condemned(h, b, n, int(loc[:, 1].max()) + 1 if len(loc) else 0, len(loc))
            continue
        p0 = None if prices is None else prices[b]
        w = want[b] if want is not None else packed_expect(loc, val, problem, n, p0=p0, **opts)
        dense_compare(h, b, w, n, m, p0=p0)
        assert h["meta"]["nnz"][b] == len(loc) and h["meta"]["bids_made"][b] == w["extra"]["bids_made"], b
    return status


# ---- 1. the lane edges of the column map and both halves of the strided scan ---------------------------------------------------
EDGE_M = (1, 2, 63, 64, 65, 127, 128, 129, 513)
EDGE_N = (1, 2, 63, 64, 65, 70, 33, 70, 70)  # n <= min(m, 70); 65 and 70 rows bid one lane per person when transposed
assert all(n <= min(m, 70) for n, m in zip(EDGE_N, EDGE_M)) and max(EDGE_N) > LANE_MIN_K


@functools.lru_cache(maxsize=None)
def edge_stack():
    probs = [signed_uniform(np.random.default_rng([51, m]), n, m) for n, m in zip(EDGE_N, EDGE_M)]
    probs[4][:, 64] = np.linspace(-40, 40, 65)   # column 64: lane 0's second slot holds an entry in every row
    probs[8][:, 512] = np.linspace(45, -45, 70)  # column 512: the first slot of the scan's second half
    mats, shapes = stack_of(probs, 70, 513)
    mats.setflags(write=False)
    return mats, shapes


@functools.lru_cache(maxsize=None)
def edge_want(problem):
    mats, shapes = edge_stack()
    packed = dense_to_packed(mats, shapes, entries="finite")
    return [packed_expect(loc, val, problem, int(n), max_iter=MAX_ITER) for (loc, val), (n, _) in zip(packed, shapes)]


@pytest.mark.parametrize("problem", PROBLEMS)
@pytest.mark.parametrize("layout", ["contiguous", "generic", "transposed"])
def test_lane_edges_in_one_batch(layout, problem):
    """contiguous: the contiguous-lane scan with the stack's natural strides; generic: the two-half strided scan;
    transposed: one lane per person in the rounds of at least LANE_MIN_K bidders, the strided scan in the others."""
    mats, shapes = edge_stack()
    storage, view = on_device(mats, layout)
    before = storage_bytes(storage)
    res = auction_solve_batch(view, problem=problem, shapes=shapes, errors="status", entries="finite", max_iter=MAX_ITER)
    status = check(res, mats, shapes, problem, want=edge_want(problem))
    assert (status == OK).all() and storage_bytes(storage) == before


# ---- 2. value mixes ----------------------------------------------------------------------------------------------------------
MIX = ("mixed", "all_negative", "all_positive", "ties", "zeros", "lone_negative_sets_C")


@functools.lru_cache(maxsize=None)
def mix_stack():
    n, m = 20, 33
    out = []
    for k, kind in enumerate(MIX):
        rng = np.random.default_rng([52, k])
        if kind == "mixed":
            v = signed_uniform(rng, n, m)
        elif kind == "all_negative":
            v = rng.uniform(-100, -1, (n, m))
        elif kind == "all_positive":
            v = rng.uniform(1, 100, (n, m))
        elif kind == "ties":
            v = signed_ints(rng, n, m, -2, 3)
        elif kind == "zeros":  # -0.0 next to +0.0, among -1 and 1
            v = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0]), (n, m))
            v[0, :4] = (-0.0, 0.0, -0.0, 0.0)
        else:
            v = rng.uniform(0, 10, (n, m))
            v[7, 11] = -1000.0
        out.append(v)
    assert np.signbit(out[4][out[4] == 0]).any() and not np.signbit(out[4][out[4] == 0]).all()
    assert np.nanmax(np.abs(out[5])) == 1000.0 and np.nanmax(out[5]) < 10
    mats = np.stack(out)
    mats.setflags(write=False)
    return mats


@pytest.mark.parametrize("fast", [False, True], ids=["eps_scaling", "fast"])
@pytest.mark.parametrize("problem", PROBLEMS)
def test_value_mixes(problem, fast):
    mats = mix_stack()
    _, view = on_device(mats)
    res = auction_solve_batch(view, problem=problem, fast=fast, errors="status", entries="finite", max_iter=MAX_ITER)
    status = check(res, mats, None, problem, fast=fast, max_iter=MAX_ITER)
    assert (status == OK).all()
    h = to_host(res)
    assert (h["meta"]["n_assigned"] == 20).all() and (h["matching_size"] == 20).all()


# ---- 3. the four element types, with the bit patterns at the edge of the rule ------------------------------------------------------
# (negative subnormals: entries; NaNs with the sign bit set or clear: absent), as integers of the element's width
EDGE_BITS = {
    "float64": ((0x8000000000000001, 0x800fffffffffffff), (0xfff8000000000000, 0xfff0000000000001, 0x7ff8000000000000)),
    "float32": ((0x80000001, 0x807fffff), (0xffc00000, 0xff800001, 0x7fc00000)),
    "float16": ((0x8001, 0x83ff), (0xfe00, 0xfc01, 0x7e00)),
    "bfloat16": ((0x8001, 0x807f), (0xffc0, 0xff81, 0x7fc0)),
}


def typed_stack(dtype):
    """(device tensor of dtype (2, 12, 70), its values widened to float64 on the host)."""
    import torch
    rng = np.random.default_rng([53, DTYPES.index(dtype)])
    vals = np.stack([signed_uniform(rng, 12, 70), signed_ints(rng, 12, 70, -3, 4)])
    t = torch.from_numpy(vals).to(getattr(torch, dtype)).cuda()
    ints = {8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]
    raw = t.view(ints)
    subnormal, nans = EDGE_BITS[dtype]
    width = 8 * t.element_size()
    signed = lambda x: x - (1 << width) if x >> (width - 1) else x  # noqa: E731
    for b in range(2):
        for k, x in enumerate(subnormal):
            raw[b, 1 + k, 5 + 64 * k] = signed(x)
        for k, x in enumerate(nans):
            raw[b, 4 + k, 3 + 30 * k] = signed(x)
    wide = t.double().cpu().numpy()
    assert (wide[:, 1, 5] < 0).all() and (wide[:, 1, 5] > -1e-4).all() and np.isnan(wide[:, 4:7, [3, 33, 63]][:, [0, 1, 2], [0, 1, 2]]).all()
    return t, wide


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_type(dtype):
    t, wide = typed_stack(dtype)
    raw = storage_bytes(t)
    for layout_of in (lambda x: x, lambda x: x.transpose(1, 2).contiguous().transpose(1, 2)):
        view = layout_of(t)
        res = auction_solve_batch(view, problem="max", mat_dtype=dtype, errors="status", entries="finite", max_iter=MAX_ITER)
        status = check(res, wide, None, "max", max_iter=MAX_ITER)
        assert (status == OK).all()
    assert storage_bytes(t) == raw
    # the subnormal is an entry and the three NaNs are not: 12 * 70 elements less the holes of the draw
    assert to_host(res)["meta"]["nnz"].tolist() == [int((~np.isnan(wide[b])).sum()) for b in range(2)]


# ---- 4. every verdict in one batch, solved problems between them -----------------------------------------------------------------
def verdict_batch():
    """(mats (B, 6, 9), shapes, prices, the planted status of every problem)."""
    N, M = 6, 9
    rng = np.random.default_rng(54)
    probs, shapes, planted = [], [], []
    prices = np.zeros((13, M))
    for b in range(13):
        n = int(rng.integers(3, N + 1))
        m = int(rng.integers(n, M + 1))
        v = signed_uniform(rng, n, m)
        kind = OK
        if b == 1:
            v[1, :] = np.nan
            kind = EMPTY_ROW
        elif b == 3:
            v[:] = np.nan
            v[0, :2] = (-1.0, 2.0)
            kind = TOO_FEW_VALUES
        elif b == 4:
            v[0, 0] = -np.inf
            kind = INFINITE_VALUE
        elif b == 5:
            prices[b, :m] = rng.uniform(0, 20, m)
        elif b == 6:
            v[n - 1, m - 1] = np.inf
            kind = INFINITE_VALUE
        elif b == 7:  # rows 0 .. 2 reach column 0 only: n - 2 rows match at most
            v[:3, 1:] = np.nan
            v[:3, 0] = (-1.0, -2.0, 3.0)
            kind = INFEASIBLE
        elif b == 9:
            kind = BAD_SHAPE
        elif b == 10:
            prices[b, m - 1] = np.nan
            kind = PRICE_NOT_FINITE
        elif b == 11:
            prices[b, 0] = -0.0
            kind = PRICE_NEGATIVE
        probs.append(v)
        shapes.append((N + 1, m) if kind == BAD_SHAPE else (n, m))
        planted.append(kind)
    mats, _ = stack_of(probs, N, M)
    return mats, np.array(shapes, dtype=np.int32), prices, planted


@pytest.mark.parametrize("layout", ["contiguous", "transposed"])
def test_every_verdict_in_one_batch(layout):
    import torch
    mats, shapes, prices, planted = verdict_batch()
    storage, view = on_device(mats, layout)
    before = storage_bytes(storage)
    kw = dict(problem="min", errors="status", entries="finite", max_iter=MAX_ITER)
    d_shapes = torch.from_numpy(shapes).cuda()  # (only a device shapes array can hold a bad entry)
    res = auction_solve_batch(view, shapes=d_shapes, prices=prices, **kw)
    status = check(res, mats, shapes, "min", prices=prices, max_iter=MAX_ITER)
    assert status.tolist() == planted and storage_bytes(storage) == before
    h = to_host(res)
    assert h["matching_size"][7] == shapes[7][0] - 2 and h["matching_size"][9] == -1
    for b in np.flatnonzero(status == OK):  # ... and equal to solving them alone
        one = to_host(auction_solve_batch(view[b:b + 1], shapes=shapes[b:b + 1], prices=prices[b:b + 1], **kw))
        assert one["status"][0] == OK and np.array_equal(one["sol"][0], h["sol"][b])
        assert np.array_equal(bits(one["prices"][0]), bits(h["prices"][b]))
        for k in ("its", "nreductions", "obj_f64", "nnz", "n_cols"):
            assert one["meta"][k][0] == h["meta"][k][b], (b, k)


# ---- 5. views ---------------------------------------------------------------------------------------------------------------
def test_column_slice_of_a_buffer_of_negative_numbers_and_nans():
    """The padding around the view holds -7.0 and NaN: under this rule -7.0 would be an entry (another count, another C,
    another column), so nothing beside the view may be read."""
    import torch
    rng = np.random.default_rng(55)
    mats = np.stack([signed_uniform(rng, 65, 130), signed_ints(rng, 65, 130, -4, 5)])
    storage, view = on_device(mats, "cols", poison=-7.0)
    assert view.storage_offset() == 3 and view.stride(2) == 1
    pad = torch.ones_like(storage, dtype=torch.bool)
    pad[:, :, 3:3 + 130] = False
    storage[pad & (torch.rand(storage.shape, device="cuda") < 0.5)] = float("nan")
    before = storage_bytes(storage)
    res = auction_solve_batch(view, problem="max", errors="status", entries="finite", max_iter=MAX_ITER)
    assert (check(res, mats, None, "max", max_iter=MAX_ITER) == OK).all() and storage_bytes(storage) == before


def test_transposed_view_with_enough_bidders_for_the_lane_mapping():
    rng = np.random.default_rng(56)
    mats = np.stack([signed_uniform(rng, 65, 130), signed_ints(rng, 65, 130, -4, 5)])
    assert mats.shape[1] > LANE_MIN_K
    storage, view = on_device(mats, "transposed")
    assert view.stride(1) == 1
    before = storage_bytes(storage)
    for problem in PROBLEMS:
        res = auction_solve_batch(view, problem=problem, errors="status", entries="finite", max_iter=MAX_ITER)
        assert (check(res, mats, None, problem, max_iter=MAX_ITER) == OK).all()
    assert storage_bytes(storage) == before


def test_expanded_matrix_from_four_starting_prices():
    import torch
    rng = np.random.default_rng(57)
    N, M = 65, 130
    one = signed_uniform(rng, N, M)
    prices = rng.uniform(0, 30, (4, M))
    prices[0] = 0.0
    d_one = torch.from_numpy(one).cuda()
    view = d_one.expand(4, N, M)
    assert view.stride(0) == 0
    before = storage_bytes(d_one)
    res = auction_solve_batch(view, prices=prices, errors="status", entries="finite", eps_start=0.5, max_iter=MAX_ITER)
    status = check(res, np.broadcast_to(one, (4, N, M)), None, "min", prices=prices, eps_start=0.5, max_iter=MAX_ITER)
    assert (status == OK).all() and storage_bytes(d_one) == before
    assert len({to_host(res)["prices"][b].tobytes() for b in range(4)}) == 4  # four different results


# ---- 6. the outside option ----------------------------------------------------------------------------------------------------
def outside_batch():
    """(mats (5, 9, 12), shapes, (B, N) outside values): mixed signs, a fully-NaN row, n_b > m_b, an all-NaN problem but
    for its last column.  Every problem has an entry in its last column, so the packed problem's columns are m_b."""
    rng = np.random.default_rng(58)
    sizes = [(9, 12), (6, 10), (9, 4), (3, 3), (5, 7)]
    probs = []
    for b, (n, m) in enumerate(sizes):
        v = rng.uniform(-50, 50, (n, m))
        v[rng.random((n, m)) < 0.4] = np.nan
        v[min(1, n - 1), m - 1] = -3.25
        probs.append(v)
    probs[0][4, :] = np.nan           # a fully-NaN row: it takes its outside option
    probs[4][:, :6] = np.nan          # one column for five rows
    probs[4][:, 6] = (-1.0, 2.0, -3.0, 4.0, -5.0)
    mats, shapes = stack_of(probs, 9, 12)
    outside = np.full((5, 9), np.nan)  # (NaN beyond n_b: never read)
    for b, (n, _) in enumerate(sizes):
        outside[b, :n] = rng.choice(np.array([-30.0, -2.5, -0.0, 0.0, 1.5, 40.0]), n)
    return mats, shapes, outside


def outside_want(mats, shapes, outside, problem, prices=None, **opts):
    """The oracle on sparse_to_augmented of every packed problem: [(want, m_b, n_b)].  outside: a float, (B,) or (B, N)."""
    out = []
    packed = dense_to_packed(mats, shapes, entries="finite")
    o = np.asarray(outside, dtype=np.float64)
    o = np.broadcast_to(o[:, None] if o.ndim == 1 else o, mats.shape[:2])
    for b, (loc, val) in enumerate(packed):
        n, m = (int(x) for x in shapes[b])
        (lo, va, m_aug, n_aug), = sparse_to_augmented(loc, val, [0, len(val)], sizes=[(m, n)], outside=o[b:b + 1, :n])
        assert (m_aug, n_aug) == (m, n) and len(lo) == len(loc) + n
        start = None if prices is None else np.concatenate([prices[b, :m], np.zeros(n)])
        out.append((sparse_expect(lo, va, problem, size=(m + n, n), p0=start, cardinality_check=False, **opts), m, n))
    return out


@pytest.mark.parametrize("problem", PROBLEMS)
@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
def test_outside_values_of_either_sign(form, problem):
    import torch
    mats, shapes, per_row = outside_batch()
    outside = {"scalar": -2.5, "per_problem": np.array([-30.0, 0.0, 1.5, -0.0, 40.0]), "per_row": per_row}[form]
    want = outside_want(mats, shapes, outside, problem, fast=True, max_iter=MAX_ITER)
    kw = dict(problem=problem, shapes=shapes, errors="status", entries="finite", max_iter=MAX_ITER)
    results = [auction_solve_batch(mats, outside=outside, **kw)]  # host arrays: the library uploads
    for layout in ("contiguous", "transposed"):
        storage, view = on_device(mats, layout)
        before = storage_bytes(storage)
        d_out = torch.from_numpy(outside).cuda() if isinstance(outside, np.ndarray) else outside
        results.append(auction_solve_batch(view, outside=d_out, **kw))
        assert storage_bytes(storage) == before
    for res in results:
        h = to_host(res)
        assert (h["status"] == OK).all() and (h["matching_size"] == -1).all()
        for b, (w, m, n) in enumerate(want):
            ell_out.compare(h, b, w, m, n)
        assert h["sol"][0, 4] == -1  # the fully-NaN row


def test_outside_verdicts_and_prices():
    mats, shapes, outside = outside_batch()
    outside = outside.copy()
    outside[1, 2] = np.nan        # BAD_OUTSIDE
    outside[2, 0] = -np.inf       # INFINITE_VALUE
    outside[3, 1] = np.inf
    mats = mats.copy()
    mats[4, 0, 6] = -np.inf       # an entry
    prices = np.random.default_rng(59).uniform(0, 10, (5, 12))
    _, view = on_device(mats)
    res = to_host(auction_solve_batch(view, shapes=shapes, outside=outside, prices=prices, errors="status",
                                      entries="finite", max_iter=MAX_ITER))
    assert res["status"].tolist() == [OK, BAD_OUTSIDE, INFINITE_VALUE, INFINITE_VALUE, INFINITE_VALUE]
    (w, m, n), = outside_want(mats[:1], shapes[:1], outside[:1], "min", prices=prices[:1], fast=True, max_iter=MAX_ITER)
    ell_out.compare(res, 0, w, m, n)
    packed = dense_to_packed(mats, shapes, entries="finite")
    for b in range(1, 5):
        n, m = (int(x) for x in shapes[b])
        condemned(res, b, n, m + n, len(packed[b][0]) + n)
    with pytest.raises(ValueError, match="problem 1: the outside value of row 2 is nan"):
        auction_solve_batch(view, shapes=shapes, outside=outside, prices=prices, entries="finite", max_iter=MAX_ITER)


# ---- 7. the matcher ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "bfloat16"])
def test_hopcroft_solve_batch_on_signed_stacks(dtype):
    rng = np.random.default_rng(60)
    mats = rng.uniform(-50, 50, (3, 65, 130))
    mats[rng.random(mats.shape) < 0.93] = np.nan  # sparse graphs: the DFS recurses and backtracks
    mats[:, 0, 0] = -1.0
    shapes = np.array([[65, 130], [40, 9], [1, 1]])
    for layout in ("contiguous", "transposed"):
        storage, view = on_device(mats, layout, dtype)
        before = storage_bytes(storage)
        for shp in (None, shapes):
            got = hopcroft_solve_batch(mats=view, shapes=shp, mat_dtype=dtype, entries="finite")
            packed = dense_to_packed(mats, shp, entries="finite")
            for b, (loc, _) in enumerate(packed):
                want = hopcroft_solve(loc=loc)
                n, m = want["left_pairings"].shape[0], want["right_pairings"].shape[0]
                left, right = host(got["left_pairings"])[b], host(got["right_pairings"])[b]
                assert got["size"][b] == want["size"] and want["size"] > 0, b
                assert np.array_equal(left[:n], want["left_pairings"]) and (left[n:] == -1).all(), b
                assert np.array_equal(right[:m], want["right_pairings"]) and (right[m:] == -1).all(), b
            nonneg = hopcroft_solve_batch(mats=view, shapes=shp, mat_dtype=dtype)  # the default rule: negatives absent
            assert (nonneg["size"] <= got["size"]).all()
        assert nonneg["size"][2] == 0 and got["size"][2] == 1  # (shapes: the 1 x 1 graph is the entry -1.0)
        assert storage_bytes(storage) == before
    if dtype == "float64":  # a host stack: uploaded, compact, the same kernels
        host_got = hopcroft_solve_batch(mats=mats, shapes=shapes, entries="finite")
        assert np.array_equal(host_got["size"], got["size"])
        assert np.array_equal(host_got["left_pairings"], host(got["left_pairings"]))


# ---- 8. the default rule is what it was, and the host path -----------------------------------------------------------------------
def test_the_default_rule_still_drops_negative_entries():
    rng = np.random.default_rng(61)
    mats = np.stack([signed_uniform(rng, 20, 33, hole_share=0.1) for _ in range(3)])
    mats[:, np.arange(20), np.arange(20)] = rng.uniform(1, 50, (3, 20))  # a non-negative diagonal: feasible under both rules
    _, view = on_device(mats)
    for kw in (dict(), dict(entries="nonneg")):
        res = to_host(auction_solve_batch(view, problem="max", errors="status", max_iter=MAX_ITER, **kw))
        assert (res["status"] == OK).all()
        for b in range(3):
            dense_compare(res, b, dense_expect(mats[b], "max", max_iter=MAX_ITER), 20, 33)
            with np.errstate(invalid="ignore"):
                assert res["meta"]["nnz"][b] == int((mats[b] >= 0).sum()) < int((~np.isnan(mats[b])).sum())
    finite = to_host(auction_solve_batch(view, problem="max", errors="status", entries="finite", max_iter=MAX_ITER))
    assert (finite["meta"]["nnz"] > res["meta"]["nnz"]).all()


def test_host_stack_with_errors_raise():
    rng = np.random.default_rng(62)
    mats = np.stack([signed_uniform(rng, 20, 33) for _ in range(3)])
    keep = mats.copy()
    res = auction_solve_batch(mats, problem="min", entries="finite", max_iter=MAX_ITER)  # errors="raise": nothing to raise
    assert isinstance(res["sol"], np.ndarray) and "status" in res and np.array_equal(bits(mats), bits(keep))
    assert (check(res, mats, None, "min", max_iter=MAX_ITER) == OK).all()
    _, view = on_device(mats)
    dev = to_host(auction_solve_batch(view, problem="min", errors="status", entries="finite", max_iter=MAX_ITER))
    for k in ("sol", "status", "matching_size"):
        assert np.array_equal(res[k], dev[k]), k
    assert np.array_equal(bits(res["prices"]), bits(dev["prices"]))
    mats[1, 17, :] = np.nan
    with pytest.raises(ValueError, match=r"^problem 1: every row must have at least one valid \(>= 0\) entry$"):
        auction_solve_batch(mats, problem="min", entries="finite", max_iter=MAX_ITER)
    assert auction_solve_batch(mats, errors="status", entries="finite", max_iter=MAX_ITER)["status"].tolist() == [0, 2, 0]
    assert _lib.DENSE_ENTRIES_FINITE == 0x100
