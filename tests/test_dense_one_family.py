"""The dense batch is one kernel family on three layouts (csrc/kernels_dense_batch.hpp: DenseContig, DenseView<false>,
DenseView<true>): which instance a call reaches must not change the answer.

One ragged non-negative stack -- the shapes cover one lane, the 64-column lane edge and the lane_min_K = 64 switch of a
transposed view -- with one problem each for TOO_FEW_VALUES, EMPTY_ROW, INFINITE_VALUE and BAD_SHAPE, is stored inside
a wider buffer of +inf and presented as
  (a) its contiguous copy                          DenseContig
  (b) a padded-row view (sM == 1)                  DenseView<false>, the contiguous-lane scan
  (c) a column-slice view (sM == 2)                DenseView<false>, the two-half scan
  (d) a transposed view (sN == 1)                  DenseView<false>, the two-half scan and bid_lanes
  (e) the contiguous copy with entries="finite"    DenseView<true> with the natural strides; holes are NaN, not -1
For float64 and bfloat16, with the guard on, in the status mode and with an outside value per row, all five return the
same bits in status, sol, prices, outside_prices, matching_size and meta.  The other dense suites tie each leg to the
oracle; this file ties the legs to each other."""
import functools

import numpy as np
import pytest

from sslap_amd import auction_solve_batch, batch_meta_to_host
from tests._batch_shapes import bits, host

pytestmark = pytest.mark.gpu

MAX_ITER = 200000
SHAPES = [(1, 1), (1, 65), (63, 64), (64, 64), (65, 130)]
N, M = 65, 130
OK, TOO_FEW_VALUES, EMPTY_ROW, INFINITE_VALUE, BAD_SHAPE = 0, 1, 2, 3, 7
LEGS = ("contiguous", "padded_rows", "column_slice", "transposed", "finite")


@functools.lru_cache(maxsize=None)
def stack():
    """(mats (9, N, M) with -1 for a hole and +inf beyond every shape, shapes, outside (9, N)).  Integers below 200: exact
    in bfloat16."""
    rng = np.random.default_rng(417)
    mats = np.full((len(SHAPES) + 4, N, M), np.inf)
    shapes = []
    for b, (n, m) in enumerate(SHAPES):
        mats[b, :n, :m] = rng.integers(0, 200, (n, m))
        shapes.append((n, m))
    b = len(SHAPES)
    mats[b, :3, :3] = -1.0  # TOO_FEW_VALUES: two entries for three rows
    mats[b, 0, 1], mats[b, 2, 0] = 5.0, 7.0
    mats[b + 1, :2, :3] = [[4.0, -1.0, 9.0], [-1.0, -1.0, -1.0]]  # EMPTY_ROW: two entries, none in row 1
    mats[b + 2, :2, :2] = [[1.0, np.inf], [2.0, 3.0]]  # INFINITE_VALUE
    shapes += [(3, 3), (2, 3), (2, 2), (0, 3)]  # ... and BAD_SHAPE
    outside = rng.integers(0, 50, (len(shapes), N)).astype(np.float64)
    return mats, np.array(shapes, dtype=np.int32), outside


def leg_view(leg, dtype):
    """The stack in dtype on the device as `leg` presents it, inside a storage of +inf."""
    import torch
    mats, _, _ = stack()
    B = mats.shape[0]
    vals = torch.from_numpy(np.where(mats == -1.0, np.nan, mats) if leg == "finite" else mats.copy())
    shape, of = {
        "contiguous": ((B, N, M), lambda s: s),
        "finite": ((B, N, M), lambda s: s),
        "padded_rows": ((B, N, M + 7), lambda s: s[:, :, 3:3 + M]),
        "column_slice": ((B, N, 2 * M), lambda s: s[:, :, ::2]),
        "transposed": ((B, M + 1, N + 2), lambda s: s[:, :M, :N].transpose(1, 2)),
    }[leg]
    storage = torch.full(shape, float("inf"), dtype=getattr(torch, dtype), device="cuda")
    view = of(storage)
    view.copy_(vals.to(getattr(torch, dtype)))
    want = {"padded_rows": (None, 1), "column_slice": (None, 2), "transposed": (1, None)}.get(leg)
    if want is None:
        assert view.is_contiguous()
    else:
        assert not view.is_contiguous()
        assert want[0] in (None, view.stride(1)) and want[1] in (None, view.stride(2))
    return view


def outputs(res):
    """Every output of a status-mode device call, as bit patterns on the host."""
    out = {k: bits(host(res[k])) if host(res[k]).dtype.kind == "f" else host(res[k])
           for k in ("status", "sol", "prices", "matching_size") + (("outside_prices",) if "outside_prices" in res else ())}
    for k, v in batch_meta_to_host(res).items():
        if isinstance(v, np.ndarray):
            out["meta." + k] = bits(v) if v.dtype.kind == "f" else v
    return out


@pytest.mark.parametrize("mode", ["status", "outside"])
@pytest.mark.parametrize("dtype", ["float64", "bfloat16"])
def test_every_layout_returns_the_same_bits(dtype, mode):
    import torch
    _, shapes, outside = stack()
    d_shapes = torch.from_numpy(shapes).cuda()  # (only a device shapes array can hold a bad entry)
    kw = dict(problem="max", shapes=d_shapes, errors="status", mat_dtype=dtype, cardinality_check=True, max_iter=MAX_ITER)
    if mode == "outside":
        kw["outside"] = torch.from_numpy(outside).cuda()
    got = {}
    for leg in LEGS:
        res = auction_solve_batch(leg_view(leg, dtype), entries="finite" if leg == "finite" else "nonneg", **kw)
        got[leg] = outputs(res)
    first = got[LEGS[0]]
    status = first["status"].tolist()
    if mode == "status":
        assert status == [OK] * len(SHAPES) + [TOO_FEW_VALUES, EMPTY_ROW, INFINITE_VALUE, BAD_SHAPE]
        assert first["matching_size"].tolist()[:len(SHAPES)] == [n for n, _ in SHAPES]  # the guard ran
    else:  # (no row of an outside call is empty, and a row may stay unmatched)
        assert status == [OK] * len(SHAPES) + [OK, OK, INFINITE_VALUE, BAD_SHAPE]
        assert "outside_prices" in first
    assert (first["sol"][:len(SHAPES)] >= -1).all() and (first["meta.its"][:len(SHAPES)] > 0).all()
    for leg in LEGS[1:]:
        assert got[leg].keys() == first.keys()
        for k, v in first.items():
            assert v.dtype == got[leg][k].dtype and np.array_equal(v, got[leg][k]), (leg, k)
