"""The batch from two box sets (auction_solve_boxes_batch, boxes_candidates; misslap_solve_boxes_batch,
misslap_boxes_batch_candidates) without a GPU: the symbols, the definition boxes_to_dense against a plain loop and
against the fused chain it must not be, the selects of the chain, the range of the costs, the verdict table derived on
the CPU, boxes_to_ell against a sort-based restatement, the gate (with outside and nothing truncated the optimum of
the lists is the optimum of the full problem), the front end's whole-call errors and the C entry points' argument
errors.
"""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sslap_amd
from sslap_amd import (_lib, auction_solve_boxes_batch, boxes_candidates, boxes_to_dense, boxes_to_ell, points_to_dense,
                       raise_for_status)
from tests._batch_shapes import bits
from tests._boxes_fixture import (BAD_BOX, DTYPES, HULL_NEGATIVE, INFINITE_VALUE, KINDS, METRICS, dense_by_loops,
                                  draw_boxes, ell_by_sorting, expected_status, pair_chain, special_boxes, verdict_batch,
                                  verdict_table)
from tests._points_candidates import same_bytes
from tests.test_points_batch_nogpu import _FakeDeviceTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_boxes_batch", "misslap_boxes_batch_candidates")
HEAD = "int64_t, int64_t, int64_t, const void *, int64_t, int64_t, int64_t, const void *, int64_t, int64_t, int64_t, int32_t, "


def test_entry_points_are_declared_bound_and_exported(built_lib):
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "#define MISSLAP_ABI_VERSION 2\n" in header and built_lib.misslap_abi_version() == 2
    codes = dict(re.findall(r"#define MISSLAP_BATCH_STATUS_([A-Z_]+) \(?(\d+)\)?", header))
    assert int(codes["BAD_BOX"]) == _lib.BATCH_STATUS_BAD_BOX == 16 == BAD_BOX
    assert sorted(int(v) for v in codes.values()) == list(range(17))  # directly behind the others, none reused
    assert "#define MISSLAP_BOXES_METRIC_IOU 1\n" in header and "#define MISSLAP_BOXES_METRIC_GIOU 2\n" in header
    assert (_lib.BOXES_METRIC_IOU, _lib.BOXES_METRIC_GIOU) == (1, 2)
    # the points calls without D and with the metric
    assert len(_lib.SYMBOLS[NAMES[0]][1]) == len(_lib.SYMBOLS["misslap_solve_points_batch"][1])
    assert len(_lib.SYMBOLS[NAMES[1]][1]) == len(_lib.SYMBOLS["misslap_points_batch_candidates"][1])
    for name in ("auction_solve_boxes_batch", "boxes_to_dense", "boxes_to_ell", "boxes_candidates"):
        assert name in sslap_amd.__all__ and callable(getattr(sslap_amd, name)), name


def test_the_header_is_c99_with_the_new_prototypes():
    prog = ['#include "misslap.h"', 'int main(void){',
            'int (*f)(' + HEAD,
            '         const int32_t *, int32_t, const double *, const misslap_options *, void *, void *,',
            '         int64_t, const double *, int64_t, int32_t *, double *, double *, int32_t, int32_t *, int32_t *,',
            '         misslap_dense_batch_meta *, misslap_dense_batch_info *) = misslap_solve_boxes_batch;',
            'int (*g)(' + HEAD,
            '         int64_t, const int32_t *, const double *, int64_t, const misslap_options *, void *, int32_t *,',
            '         double *, int32_t *, int32_t *) = misslap_boxes_batch_candidates;',
            'return (f == 0) + (g == 0) + (MISSLAP_BATCH_STATUS_BAD_BOX != 16) + (MISSLAP_BOXES_METRIC_GIOU != 2);}']
    for std in ("c99", "c11"):
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "t.c")
            open(src, "w").write("\n".join(prog))
            subprocess.check_call(["gcc", f"-std={std}", "-Wall", "-Werror", "-pedantic", "-c", "-I",
                                   os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "t.o")])


def test_build_sees_the_new_headers():
    from sslap_amd import build
    unit = open(os.path.join(build.CSRC, "misslap.hip")).read()
    order = re.findall(r'#include "([a-z_0-9]+\.hpp)"', unit)
    mine = ["kernels_boxes_batch.hpp", "abi_boxes_batch.hpp"]
    # behind what existed: no kernel above is instantiated or scheduled differently for them
    assert order[-2:] == mine and order.index(mine[0]) > order.index("abi_points_whiten.hpp")
    for name in mine:
        assert name in build.SOURCES and os.path.exists(os.path.join(build.CSRC, name)), name


# ---- the definition

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_definition_is_the_loop_and_not_the_fused_chain(dtype, metric, kind):
    rng = np.random.default_rng([12, KINDS.index(kind)])
    B, N, M = 3, 7, 6
    a, b = draw_boxes(kind, (B, N, 4), dtype, rng), draw_boxes(kind, (B, M, 4), dtype, rng)
    got = boxes_to_dense(a, b, metric=metric)
    assert got.dtype == np.float64 and got.shape == (B, N, M) and got.flags.c_contiguous
    assert np.array_equal(bits(got), bits(dense_by_loops(a, b, metric=metric)))
    assert np.isfinite(got).all() and not np.signbit(got).any()
    overlaps = (boxes_to_dense(a, b, metric="iou") < 1.0).sum(axis=2)  # the draws overlap: a stack of 1.0 tests nothing
    assert overlaps.mean() >= 2.0 and (overlaps > 0).mean() >= 0.7, overlaps
    shapes = np.array([[7, 6], [1, 1], [4, 5]])
    with_shapes = boxes_to_dense(a, b, shapes, metric)
    assert np.array_equal(bits(with_shapes), bits(dense_by_loops(a, b, shapes, metric)))
    assert np.isposinf(with_shapes[1, 1:]).all() and np.isposinf(with_shapes[2, :, 5:]).all()
    differ = int((bits(dense_by_loops(a, b, metric=metric, fused=True)) != bits(got)).sum())
    if kind == "uniform" and dtype == "float64":  # a contracted chain is another function on this draw
        assert differ >= 1, differ
    import torch
    assert np.array_equal(bits(boxes_to_dense(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(shapes), metric)),
                          bits(with_shapes))
    assert np.array_equal(bits(boxes_to_dense(a, b, shapes)), bits(boxes_to_dense(a, b, shapes, "iou")))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_selects_of_the_chain(dtype):
    a, b = special_boxes(dtype)
    iou, giou = boxes_to_dense(a, b, metric="iou")[0], boxes_to_dense(a, b, metric="giou")[0]
    for metric, got in (("iou", iou), ("giou", giou)):
        assert np.array_equal(bits(got), bits(dense_by_loops(a, b, metric=metric)[0]))
        assert np.isfinite(got).all() and not np.signbit(got).any()
    zero = bits(np.array(0.0))
    assert bits(iou[0, 0]) == zero and bits(giou[0, 0]) == zero     # identical: +0.0
    assert iou[0, 1] == 1.0 and giou[0, 1] == 1.0                    # touching: iw = 0, the hull is their union
    assert iou[1, 2] == 1.0 - 1.0 / 16.0 == giou[1, 2]               # nested: the hull is the outer box
    assert iou[0, 2] == 0.5                                          # nested, half the area
    assert iou[2, 3] == 1.0 and giou[2, 3] == 1.0                    # two points at one place: u = 0 and hull = 0
    assert (iou[:5, 4] == 1.0).all() and (giou[:5, 4] > 1.0).all()   # disjoint
    assert iou[3, 5] == 1.0 and giou[3, 5] == 1.0                    # a segment in a segment: u = 0 and hull = 0
    assert iou[4, 6] == 1.0 and giou[4, 6] == 1.0                    # the origin under both signs of zero
    assert iou[2, 0] == 1.0 and giou[2, 0] == 1.0                    # a point on a box's corner: inter = 0, hull = u
    # the pairs for which hull - u rounds negative: without the clamp r would be negative and the cost below 1 - iou
    for k, (p, q) in enumerate(HULL_NEGATIVE[:2 if dtype == "float64" else 1]):
        assert np.array_equal(np.array(p, dtype=dtype).astype(np.float64), np.array(p)), "exact in dtype"
        r = pair_chain(p, q, True)
        assert r["e_raw"] < 0.0 and not r["flagged"]
        assert np.array_equal(a[0, 5 + k], np.array(p, dtype=dtype)) and np.array_equal(b[0, 7 + k], np.array(q, dtype=dtype))
        assert bits(giou[5 + k, 7 + k]) == bits(np.array(r["c"])) == bits(iou[5 + k, 7 + k])  # r = 0: giou is iou there


def _adversarial(dtype, rng, trial, n=40):
    """The draws of the search that found HULL_NEGATIVE: uniform, an integer grid, six decades of sizes, one box
    repeated -- and the second set the first perturbed by 1e-16 .. 1 relative."""
    kind = trial % 4
    if kind == 0:
        c, s = rng.uniform(0, 10, (n, 2)), rng.uniform(0, 4, (n, 2))
    elif kind == 1:
        c, s = rng.integers(0, 4, (n, 2)).astype(float), rng.integers(0, 3, (n, 2)).astype(float)
    elif kind == 2:
        c, s = rng.uniform(0, 1, (n, 2)) * 1e6, rng.uniform(0, 1, (n, 2)) * 10 ** rng.uniform(-6, 6, (n, 2))
    else:
        c, s = np.repeat(rng.uniform(0, 10, (1, 2)), n, 0), np.repeat(rng.uniform(1, 3, (1, 2)), n, 0)
    a = np.concatenate([c - s / 2, c + s / 2], 1)
    b = a + rng.uniform(-1, 1, a.shape) * 10 ** rng.uniform(-16, 0, a.shape) * (kind != 1)
    a, b = a.astype(dtype), b.astype(dtype)
    a[:, 2:], b[:, 2:] = np.maximum(a[:, 2:], a[:, :2]), np.maximum(b[:, 2:], b[:, :2])
    return a[None], b[None]


@pytest.mark.parametrize("dtype", DTYPES)
def test_costs_lie_in_their_range_and_carry_no_sign_bit(dtype):
    rng = np.random.default_rng(7)
    pairs = below_one = above_one = 0
    for trial in range(120):
        a, b = _adversarial(dtype, rng, trial)
        iou, giou = boxes_to_dense(a, b, metric="iou"), boxes_to_dense(a, b, metric="giou")
        for c, top in ((iou, 1.0), (giou, 2.0)):
            assert np.isfinite(c).all() and (c >= 0.0).all() and (c <= top).all() and not np.signbit(c).any(), trial
        pairs += iou.size
        below_one += int((iou < 1.0).sum())
        above_one += int((giou > 1.0).sum())
    assert pairs == 120 * 1600 and below_one > pairs // 20 and above_one > pairs // 20


# ---- what is no cost, and the verdicts

def test_non_finite_and_bad_pairs_are_stored_as_inf():
    a = np.array([[[0.0, 0.0, 1.0, 1.0], [np.nan, 0.0, 1.0, 1.0], [0.0, 0.0, np.inf, 1.0], [2.0, 0.0, 1.0, 1.0],
                   [-1e308, 0.0, 1e308, 1.0], [0.0, 0.0, 1e200, 1e200], [0.0, 0.0, 1e200, 1.0], [1e308, 0.0, 1e308, 1.0]]])
    b = np.array([[[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1e200], [-1e308, 0.0, -1e308, 1.0]]])
    iou, giou = boxes_to_dense(a, b, metric="iou")[0], boxes_to_dense(a, b, metric="giou")[0]
    assert iou[0, 0] == 0.0 and np.isfinite(iou[0]).all()
    for i in (1, 2, 3, 4, 5):  # NaN, infinite, a bad box, an infinite width, an infinite area: every pair of the row
        assert np.isposinf(iou[i]).all() and np.isposinf(giou[i]).all(), i
    assert np.isfinite(iou[6]).all() and np.isposinf(giou[6, 1]) and np.isfinite(giou[6, 0])  # the hull alone overflows
    assert np.isposinf(iou[7, 2]) and np.isfinite(iou[7, :2]).all()  # iw = -inf before the clamp would be swallowed
    assert not np.isnan(iou).any() and not np.isnan(giou).any()
    assert np.array_equal(bits(iou), bits(dense_by_loops(a, b, metric="iou")[0]))
    assert np.array_equal(bits(giou), bits(dense_by_loops(a, b, metric="giou")[0]))
    # float32 boxes cannot overflow the float64 chain
    big = np.array([[[-3e38, -3e38, 3e38, 3e38], [3e38, 3e38, 3e38, 3e38]]], dtype=np.float32)
    for metric in METRICS:
        assert np.isfinite(boxes_to_dense(big, big[:, ::-1], metric=metric)).all()


@pytest.mark.parametrize("with_outside", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_verdict_expectations_of_a_mixed_batch(dtype, metric, with_outside):
    v = verdict_batch(dtype)
    outside = v["outside"] if with_outside else None
    status, size = expected_status(v["a"], v["b"], v["shapes"], v["prices"], outside, metric)
    for p, kind in enumerate(v["kinds"]):
        assert status[p] == verdict_table(kind, metric, with_outside, dtype == "float64"), (p, kind, status[p])
    assert {0, 3, 5, 6, 7, 16} <= set(status.tolist()) and (15 if with_outside else 4) in status
    # the definition tells the same story: a problem is clean iff its slice of boxes_to_dense is finite
    cost = boxes_to_dense(v["a"], v["b"], v["shapes"], metric)
    for p, (n, m) in enumerate(v["shapes"]):
        if status[p] in (INFINITE_VALUE, BAD_BOX) and v["kinds"][p] != "inf_outside":
            assert np.isposinf(cost[p, :n, :m]).any() and not np.isnan(cost[p]).any(), p
        elif status[p] == 0:
            assert np.isfinite(cost[p, :n, :m]).all(), p
    assert (size[status == 7] == -1).all() and ((size == -1).all() if with_outside else (size[status != 7] > 0).all())


def test_the_status_texts_know_code_16():
    from sslap_amd._batch import _STATUS_ERRORS
    res = dict(stack=(4, 5), layout="boxes", status=np.array([0, 16, 3]), matching_size=np.array([4, -1, -1]),
               meta=dict(n_rows=np.array([4, 4, 4]), n_cols=np.array([5, 5, 5])))
    with pytest.raises(ValueError, match=r"problem 1: a box has x2 < x1 or y2 < y1"):
        raise_for_status(res)
    text = str(_STATUS_ERRORS["boxes"](res, 2, 3, 4, 5, -1))
    assert text.startswith("problem 2: a box cost is not finite") and "outside" not in text
    assert "or an outside value is +inf" in str(_STATUS_ERRORS["boxes"](dict(res, outside_prices=0), 2, 3, 4, 5, -1))
    assert sslap_amd.boxes_batch._STATUS_TEXT.keys() == {7, 15, 3, 16, 4, 5, 6}


# ---- boxes_to_ell against the sort-based restatement

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_boxes_to_ell_is_the_sorted_lists(dtype, metric):
    rng = np.random.default_rng([15, DTYPES.index(dtype)])
    B, N, M = 6, 7, 11
    a, b = draw_boxes("grid", (B, N, 4), dtype, rng), draw_boxes("grid", (B, M, 4), dtype, rng)  # ties are common
    a[0], b[0] = draw_boxes("uniform", (N, 4), dtype, rng), draw_boxes("uniform", (M, 4), dtype, rng)
    a[1, 2] = [2.0, 1.0, 1.0, 3.0]   # a bad-box row: every pair of it is a candidate at +inf
    b[1, 4] = [1.0, 3.0, 2.0, 2.0]   # ... and a bad-box column
    b[2, 0, 1] = np.nan
    shapes = np.array([[7, 11], [7, 11], [5, 9], [0, 5], [7, 12], [1, 1]])
    cost = boxes_to_dense(a, b, metric=metric)
    srt = np.sort(np.where(np.isfinite(cost), cost, 0.0), axis=2)
    per_row = srt[:, :, 3] + np.array([0.0, 1e-3, -0.0, -1.0, np.nan, np.inf, 0.0])[None, :]  # equal to a cost, between, ...
    per_row[:, 2] = -0.0
    seen = dict(truncated=0, exact=0, holes=0)
    for limit in (None, 0.75, np.array([0.5, 1.0, 0.9, 0.1, 2.0, -0.0]), per_row):
        for shp in (None, shapes):
            for k in (1, 3, 4, 5, 11, 64):
                got = boxes_to_ell(a, b, k, shp, limit, metric)
                want = ell_by_sorting(cost, k, shp, limit)
                assert same_bytes(got, want), (k, shp is None)
                seen["truncated"] += int((got["counts"] > k).sum())
                seen["exact"] += int((got["counts"] == k).sum())
                seen["holes"] += int((got["cols"] == -1).sum())
    assert all(v > 50 for v in seen.values()), seen
    # K + 1 candidates with a tie at the K-th key: the first in column order is kept
    a1 = np.array([[[0.0, 0.0, 2.0, 2.0]]], dtype=dtype)
    b1 = np.array([[[0.0, 0.0, 1.0, 2.0], [1.0, 0.0, 2.0, 2.0], [0.0, 0.0, 2.0, 2.0], [0.0, 1.0, 2.0, 2.0]]], dtype=dtype)
    got = boxes_to_ell(a1, b1, 2, metric=metric)
    assert got["counts"][0, 0] == 4 and got["cols"][0, 0].tolist() == [0, 2] and got["vals"][0, 0].tolist() == [0.5, 0.0]
    # the bad-box row and column, and the NaN coordinate, come first and are stored as +inf
    got = boxes_to_ell(a, b, 3, None, 0.0, metric)
    assert np.isposinf(got["vals"][1, 2]).all() and got["counts"][1, 2] == M
    assert (got["cols"][1, [0, 1, 3], 0] == 4).all() and np.isposinf(got["vals"][1, [0, 1, 3], 0]).all()
    assert (got["cols"][2, :, 0] == 0).all() and np.isposinf(got["vals"][2, :, 0]).all() and not np.isnan(got["vals"]).any()
    import torch
    t = boxes_to_ell(torch.from_numpy(a), torch.from_numpy(b), 3, torch.from_numpy(shapes), torch.from_numpy(per_row), metric)
    assert same_bytes(t, boxes_to_ell(a, b, 3, shapes, per_row, metric))
    with pytest.raises(ValueError, match="limit must be a float or have shape"):
        boxes_to_ell(a, b, 3, limit=np.zeros(B + 1))
    with pytest.raises(ValueError, match="shapes must have shape"):
        boxes_to_ell(a, b, 3, shapes=shapes[:2])


# ---- the gate: outside is a cost, and the lists under it lose nothing

@pytest.mark.parametrize("metric", METRICS)
def test_the_optimum_of_the_untruncated_lists_is_the_optimum_with_outside(metric):
    """400 draws, none skipped: n, m <= 8, an outside value per row, k = m so that nothing is truncated.  scipy's
    optimum of the augmented dense problem -- every pair, or the row's own outside entry -- and of the augmented list
    problem -- only the pairs of boxes_to_ell(limit=outside) -- are sums of n terms of at most 2 over assignments of
    equal exact cost, so they agree up to the rounding of the two summations: n * 2 * 2^-52 relative (derived, not
    measured)."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng([31, METRICS.index(metric)])
    pruned = unmatched = matched = 0
    for t in range(400):
        n, m = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        kind = KINDS[t % 2]
        dtype = DTYPES[(t // 2) % 2]
        a, b = draw_boxes(kind, (1, n, 4), dtype, rng, span=3), draw_boxes(kind, (1, m, 4), dtype, rng, span=3)
        outside = rng.uniform(0.3, 1.0 if metric == "iou" else 1.4, (1, n))
        cost = boxes_to_dense(a, b, metric=metric)[0]
        ell = boxes_to_ell(a, b, m, limit=outside, metric=metric)
        assert (ell["counts"] <= m).all() and ell["rows"][0] == n
        virt = np.full((n, n), np.inf)
        virt[np.arange(n), np.arange(n)] = outside[0]
        listed = np.full((n, m), np.inf)
        for i in range(n):
            for s in range(int(ell["counts"][0, i])):
                listed[i, ell["cols"][0, i, s]] = ell["vals"][0, i, s]
        assert np.array_equal(np.isfinite(listed), cost <= outside[0][:, None])
        full, gated = np.concatenate([cost, virt], axis=1), np.concatenate([listed, virt], axis=1)
        (r, c), (r2, c2) = lsa(full), lsa(gated)
        o1, o2 = float(full[r, c].sum()), float(gated[r2, c2].sum())
        assert abs(o1 - o2) <= n * 2 * 2.0 ** -52 * max(o1, o2), (t, o1, o2)
        pruned += int((cost > outside[0][:, None]).sum())
        unmatched += int((c2 >= m).sum())
        matched += int((c2 < m).sum())
    assert pruned > 1000 and unmatched > 100 and matched > 100


# ---- the front end: every whole-call error raises before the library is reached

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    """The library is never reached: loading it, and the builder's launch on device tensors, raise _NoFFI."""
    def no_load(*args, **kw):
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setattr(sslap_amd.boxes_batch, "_candidates_launch", no_load)
    monkeypatch.setattr(sslap_amd.boxes_batch, "_upload_points", no_load)


A = np.arange(32, dtype=np.float64).reshape(2, 4, 4)
Bx = np.arange(40, dtype=np.float64).reshape(2, 5, 4) / 7


@pytest.mark.parametrize("call", ["solve", "candidates", "route"])
def test_whole_call_errors_are_raised_before_the_library(no_ffi, call):
    import torch

    def f(a=A, b=Bx, **kw):
        if call == "solve":
            return auction_solve_boxes_batch(a, b, **kw)
        if call == "candidates":
            return boxes_candidates(a, b, 4, **kw)
        return auction_solve_boxes_batch(a, b, candidates=4, **kw)

    with pytest.raises(ValueError, match="metric must be 'iou' or 'giou'"):
        f(metric="diou")
    with pytest.raises(ValueError, match="metric must be 'iou' or 'giou'"):
        f(metric=1)
    with pytest.raises(ValueError, match="one dtype"):
        f(b=Bx.astype(np.float32))
    for dt in (np.float16, np.int64):
        with pytest.raises(ValueError, match="float64 or float32"):
            f(a=A.astype(dt), b=Bx.astype(dt))
    with pytest.raises(ValueError, match="3 dimensions"):
        f(a=A[0])
    with pytest.raises(ValueError, match="a box is 4 coordinates"):
        f(a=np.zeros((2, 4, 3)), b=np.zeros((2, 5, 3)))
    with pytest.raises(ValueError, match="a box is 4 coordinates"):
        f(b=np.zeros((2, 5, 5)))
    with pytest.raises(ValueError, match="B must agree"):
        f(b=np.zeros((3, 5, 4)))
    with pytest.raises(ValueError, match="empty box sets"):
        f(a=np.zeros((2, 0, 4)))
    with pytest.raises(ValueError, match="at most 2048 x 2048"):
        f(a=np.zeros((1, 2049, 4)), b=np.zeros((1, 2, 4)))
    with pytest.raises(ValueError, match="at most 2048 x 2048"):
        f(a=np.zeros((1, 2, 4)), b=np.zeros((1, 2049, 4)))
    with pytest.raises(TypeError, match="numpy arrays or tensors on the device"):
        f(a=A.tolist())
    fa, fb = _FakeDeviceTensor(A.shape, torch.float64), _FakeDeviceTensor(Bx.shape, torch.float64)
    with pytest.raises(TypeError, match="both be numpy arrays or both tensors"):
        f(a=fa)
    with pytest.raises(ValueError, match="a is on cuda:0, b on cuda:1"):
        f(a=fa, b=_FakeDeviceTensor(Bx.shape, torch.float64, index=1))
    with pytest.raises(ValueError, match="b has strides .*a stride must be >= 0"):
        f(a=fa, b=_FakeDeviceTensor(Bx.shape, torch.float64, (20, -4, 1)))
    with pytest.raises(ValueError, match="shapes must be an integer array of shape"):
        f(shapes=np.zeros((3, 2), dtype=np.int32))
    with pytest.raises(ValueError, match=r"problem 1: shape \(5, 5\) outside"):
        f(shapes=np.array([[4, 5], [5, 5]]))
    if call == "candidates":
        with pytest.raises(ValueError, match="limit must have shape"):
            f(limit=np.zeros(3))
        with pytest.raises(TypeError, match="limit must be a float"):
            f(limit="0.7")
        with pytest.raises(ValueError, match="1 .. 64"):
            boxes_candidates(A, Bx, 65)
        with pytest.raises(TypeError, match="must be an integer"):
            boxes_candidates(A, Bx, 4.0)
    else:
        with pytest.raises(ValueError, match="errors must be"):
            f(errors="warn")
        with pytest.raises(ValueError, match="outside must have shape"):
            f(outside=np.zeros(3))
        with pytest.raises(ValueError, match="outside must be finite"):
            f(outside=float("inf"))
        with pytest.raises(ValueError, match="eps_start is NaN"):
            f(eps_start=float("nan"))
        with pytest.raises(TypeError, match="takes no finish=None"):
            f(finish=None)
        with pytest.raises(ValueError, match="finish must be left out or 'reverse'"):
            f(finish="forward")
    if call == "solve":
        with pytest.raises(ValueError, match="prices must have shape"):
            f(prices=np.zeros((2, 4)))
        with pytest.raises(ValueError, match="outside must be >= 0"):
            f(outside=-0.5)
        with pytest.raises(ValueError, match="finish='reverse' needs candidates=K"):
            f(outside=0.7, finish="reverse")
        with pytest.raises(ValueError, match="finish='reverse' needs candidates=K"):
            f(a=fa, b=fb, finish="reverse")
    if call == "route":
        with pytest.raises(ValueError, match="candidates needs problem='min'"):
            f(problem="max")
        with pytest.raises(ValueError, match="1 .. 64"):
            auction_solve_boxes_batch(A, Bx, candidates=0)
        with pytest.raises(TypeError, match="outside on the device need a / b on the device"):
            f(outside=_FakeDeviceTensor((2,), torch.float64))
    # a good call reaches the library
    with pytest.raises(_NoFFI):
        f()
    with pytest.raises(_NoFFI):
        f(metric="giou", shapes=np.array([[4, 5], [1, 1]]))
    if call != "solve":  # (one box set for the call, expanded: a batch stride of 0)
        with pytest.raises(_NoFFI):
            f(a=fa, b=_FakeDeviceTensor(Bx.shape, torch.float64, (0, 4, 1)), metric="giou")
    if call == "route":
        with pytest.raises(_NoFFI):
            f(a=fa, b=fb, finish="reverse")


# ---- the C entry points: argument errors that need no device

def test_c_entry_points_validate_their_arguments(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    a, b = np.zeros((1, 2, 4)), np.ones((1, 2, 4))
    sol, status, prices = np.empty((1, 2), dtype=np.int32), np.empty(1, dtype=np.int32), np.empty((1, 2))
    err = built_lib.misslap_last_error

    def solve(B=1, N=2, M=2, ap=a.ctypes.data, sa=(8, 4, 1), bp=b.ctypes.data, sb=(8, 4, 1), metric=1, opts=o,
              solp=sol.ctypes.data, stp=status.ctypes.data, outside=None, outside_ld=0):
        return built_lib.misslap_solve_boxes_batch(
            B, N, M, ap, *sa, bp, *sb, metric, None, 0, None, C.byref(opts), None, None, 0, outside, outside_ld, solp,
            prices.ctypes.data, None, 0, stp, None, None, None)

    for metric in (0, 3, -1):
        assert solve(metric=metric) == _lib.ERR_INVALID and b"metric" in err() and b"MISSLAP_BOXES_METRIC_IOU" in err()
    assert solve(ap=None) == _lib.ERR_INVALID and b"null" in err()
    assert solve(bp=None) == _lib.ERR_INVALID and b"null" in err()
    assert solve(solp=None) == _lib.ERR_INVALID and b"null" in err()
    assert solve(stp=None) == _lib.ERR_INVALID and b"null" in err()
    for kw in (dict(N=0), dict(N=2049), dict(M=0), dict(M=2049), dict(B=0)):
        assert solve(**kw) == _lib.ERR_INVALID and b"B, N, M" in err(), kw
    assert solve(sa=(8, -4, 1)) == _lib.ERR_INVALID and b">= 0" in err()
    assert solve(B=2, sb=(2**62, 4, 1)) == _lib.ERR_INVALID and b"62 bits" in err()
    assert solve(sa=(8, 1, 2)) == _lib.ERR_INVALID and b"device array" in err()  # a strided host array
    assert solve(outside=prices.ctypes.data, outside_ld=1) == _lib.ERR_INVALID and b"outside_ld" in err()
    f16 = _lib.Options()
    f16.struct_size, f16.mat_dtype = C.sizeof(_lib.Options), _lib.DTYPE_F16
    assert solve(opts=f16) == _lib.ERR_INVALID and b"MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32" in err()
    # the workspace is the points call's, and its size needs no GPU
    assert built_lib.misslap_points_batch_workspace_bytes(3, 2048, 2048, 1, 1) > 3 * 4096 * 8
    assert built_lib.misslap_points_batch_workspace_bytes(3, 2049, 1, 0, 0) == -1

    od = _lib.Options()
    od.struct_size = C.sizeof(_lib.Options)
    od.input_on_device = 1
    out = (np.empty(8, dtype=np.int32), np.empty(8), np.empty(2, dtype=np.int32), np.empty(1, dtype=np.int32))

    def cand(N=2, M=2, ap=a.ctypes.data, sa=(8, 4, 1), metric=2, K=4, opts=od, limit_ld=0, limit=None, outs=out):
        return built_lib.misslap_boxes_batch_candidates(
            1, N, M, ap, *sa, b.ctypes.data, 8, 4, 1, metric, K, None, limit, limit_ld, C.byref(opts), None,
            *(None if t is None else t.ctypes.data for t in outs))

    assert cand(metric=0) == _lib.ERR_INVALID and b"metric" in err()
    assert cand(metric=7) == _lib.ERR_INVALID and b"metric" in err()
    assert cand(ap=None) == _lib.ERR_INVALID and b"null" in err()
    assert cand(outs=(out[0], None, out[2], out[3])) == _lib.ERR_INVALID and b"null" in err()
    assert cand(K=0) == _lib.ERR_INVALID and b"MISSLAP_POINTS_CANDIDATES_MAX_K" in err()
    assert cand(K=65) == _lib.ERR_INVALID and b"MISSLAP_POINTS_CANDIDATES_MAX_K" in err()
    assert cand(N=2049) == _lib.ERR_INVALID and b"B, N, M" in err()
    assert cand(sa=(8, 4, -1)) == _lib.ERR_INVALID and b">= 0" in err()
    assert cand(opts=o) == _lib.ERR_INVALID and b"input_on_device" in err()
    assert cand(limit=out[1].ctypes.data, limit_ld=1) == _lib.ERR_INVALID and b"limit_ld" in err()


def test_the_plain_points_definition_is_untouched():
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-1, 1, (2, 5, 4)), rng.uniform(-1, 1, (2, 6, 4))
    from tests._points_fixture import dense_by_loops as points_by_loops
    assert np.array_equal(bits(points_to_dense(x, y)), bits(points_by_loops(x, y)))
