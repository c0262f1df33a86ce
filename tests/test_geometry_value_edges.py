"""The points batch, its whitened variant and the boxes batch on the GPU at the edges of the value range (the cases of
tests/_geometry_value_edges.py): a C = max cost that is +inf, 0, a subnormal or a tie as a float32, out of the families'
own check passes; costs of 2^52 .. 2^58, where eps falls below one ulp of the prices; stacks of +0.0; float32
coordinates that are subnormal; float64 boxes whose areas are subnormal doubles, so that inter / u and e / hull divide
subnormals, and boxes at the last scale before a sum overflows; whitening matrices that carry the magnitude alone or
share it with the coordinates; limits of the builder at the smallest subnormal and at DBL_MAX.

The cost stack is always the numpy definition (points_to_dense, boxes_to_dense) and the expected result the oracle's on
that stack; every comparison is `==` on every bit (dense_compare via check_plain, compare of the outside tests,
same_bytes, assert_is_the_model): sol, the price bits, obj_f64, the fp32 bits of start_eps / final_eps, its, eCE,
n_assigned.  As a second yardstick the same call is compared with auction_solve_batch on the stored stack.  The cases of
one (family, type, D or metric, size, eps_start, stop) travel in one batch, so a workgroup that spins at eps == 0 or at
eps == +inf until max_iter runs beside converging ones; a solve that does not end on its own always has an explicit
max_iter (test_geometry_value_edges_nogpu.py holds the oracle of every case to its stop).
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import (auction_solve_batch, auction_solve_boxes_batch, auction_solve_ell_batch, auction_solve_points_batch,
                       boxes_candidates, boxes_to_ell, ell_to_packed, points_candidates, points_to_ell)
from tests import _geometry_value_edges as ge
from tests import _list_finish as lf
from tests import _points_finish as pfin
from tests._batch_shapes import threads_for
from tests._points_candidates import KEYS, same_bytes
from tests.test_dense_outside import compare as outside_compare
from tests.test_points_batch import _dev, _host, _same, check_plain
from tests.test_points_candidates import _lists, _same_as_ell

pytestmark = pytest.mark.gpu

FAMILY_NAMES = tuple(ge.FAMILIES)
F32_TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(autouse=True)
def _quiet_narrowing():
    """eps_start = 1e39 narrows to +inf as a float32, which numpy reports: that is the case."""
    with np.errstate(over="ignore"):
        yield


class _Batch:
    """The cases of one key as one call's inputs, on the host and on the device."""

    def __init__(self, cases):
        self.cases = cases
        self.family, self.key = cases[0].family, cases[0].key
        self.x, self.y = np.stack([c.x for c in cases]), np.stack([c.y for c in cases])
        self.w = None if cases[0].w is None else np.stack([c.w for c in cases])
        self.shapes = ge.shapes_of(cases)
        self.cost = ge.cost_stack(cases)
        self.B, self.N, self.M = self.cost.shape
        self.metric = ge.metric_of(cases[0])

    def device(self):
        return (_dev(self.x), _dev(self.y), None if self.w is None else _dev(self.w),
                None if self.shapes is None else _dev(self.shapes))

    def solve(self, on_device=False, **kw):
        """auction_solve_points_batch / auction_solve_boxes_batch in status mode, from numpy arrays or device tensors."""
        x, y, w, shapes = self.device() if on_device else (self.x, self.y, self.w, self.shapes)
        if self.family == "boxes":
            return auction_solve_boxes_batch(x, y, self.metric, shapes=shapes, errors="status", **kw)
        return auction_solve_points_batch(x, y, shapes=shapes, whiten=w, errors="status", **kw)

    def to_ell(self, k, limit=None):
        if self.family == "boxes":
            return boxes_to_ell(self.x, self.y, k, self.shapes, limit, self.metric)
        return points_to_ell(self.x, self.y, k, self.shapes, limit, self.w)

    def candidates(self, k, limit=None):
        x, y, w, shapes = self.device()
        lim = _dev(limit) if isinstance(limit, np.ndarray) else limit
        if self.family == "boxes":
            return boxes_candidates(x, y, k, shapes=shapes, limit=lim, metric=self.metric)
        return points_candidates(x, y, k, shapes=shapes, limit=lim, whiten=w)


def _ok(res, batch):
    assert res["status"].dtype == np.int32 and (res["status"] == 0).all(), res["status"]
    assert res["sol"].shape == (batch.B, batch.N) and res["prices"].shape == (batch.B, batch.M)
    assert res["meta"]["gpu"]["threads"] == threads_for(ge.N) == threads_for(batch.N)
    assert res["layout"] == ("boxes" if batch.family == "boxes" else "points")


# ---- 1. the plain solve

@pytest.mark.parametrize("problem", ge.PROBLEMS)
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_plain_solve_against_the_oracle_and_the_dense_batch(family, problem):
    seen = 0
    for key, opts, stop, cases in ge.groups(ge.FAMILIES[family]()):
        batch = _Batch(cases)
        kw = dict(problem=problem, **ge.call_opts(opts, stop))
        got = batch.solve(**kw)
        _ok(got, batch)
        check_plain(got, batch.cost, batch.shapes, problem, **ge.call_opts(opts, stop))
        dev = batch.solve(on_device=True, **kw)
        assert dev["sol"].is_cuda
        _same(_host(dev), got, matching_size=True)
        dense = _host(auction_solve_batch(_dev(batch.cost), shapes=None if batch.shapes is None else _dev(batch.shapes),
                                          errors="status", cardinality_check=False, **kw))
        assert (dense["status"] == 0).all()
        _same(got, dense)
        seen += len(cases)
    assert seen == len(ge.FAMILIES[family]())


# ---- 2. outside: eps-scaling from C, so the check pass's C is used

@pytest.mark.parametrize("problem", ge.PROBLEMS)
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_outside_at_the_cases_own_magnitude(family, problem):
    """Per-row outside values in the range of the case's costs, one equal to a cost; -0.0 beside costs that are zero as a
    float32; 3.0 beside costs of 2^-160 and 2^60 beside ordinary ones, which set C alone."""
    seen = alone = 0
    for key, opts, stop, entries in ge.outside_groups(ge.FAMILIES[family]()):
        batch = _Batch([c for c, _ in entries])
        outside = np.stack([o for _, o in entries])
        kw = dict(problem=problem, max_iter=stop, **opts, **ge.OUTSIDE_OPTS)
        got = batch.solve(outside=outside, **kw)
        _ok(got, batch)
        assert (got["matching_size"] == -1).all() and got["outside_prices"].shape == (batch.B, batch.N)
        for b, (want, m, n) in enumerate(ge.outside_want(key, opts, stop, entries, problem)):
            outside_compare(got, b, want, m, n)
            if outside[b, 0] in (3.0, 2.0 ** 60):  # C is the outside value's alone
                assert np.float32(got["meta"]["start_eps_f32"][b]) == np.float32(outside[b, 0] / 2)
                alone += 1
        dev = _host(batch.solve(on_device=True, outside=_dev(outside), **kw))
        _same(dev, got, matching_size=True)
        dense = _host(auction_solve_batch(_dev(batch.cost), shapes=None if batch.shapes is None else _dev(batch.shapes),
                                          outside=_dev(outside), errors="status", **kw))
        _same(dense, got, matching_size=True)
        seen += len(entries)
    extra = len(ge.C_FROM_OUTSIDE) if family == "points" else 0
    assert seen == len(ge.FAMILIES[family]()) + extra and alone == extra


# ---- 3. the builder: the integer keys at subnormal costs and limits, at DBL_MAX, at +inf

@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_builder_is_the_definition_byte_for_byte(family):
    seen = tied = 0
    for key, cases in ge.by_key(ge.FAMILIES[family]()).items():
        batch = _Batch(cases)
        for k in ge.BUILDER_K:
            for limit in ge.limits(cases):
                got = _lists(batch.candidates(k, limit))
                want = batch.to_ell(k, limit)
                for name in KEYS:
                    assert got[name].tobytes() == want[name].tobytes(), (key, k, name, limit if np.isscalar(limit) else "3rd")
                assert same_bytes(got, want)
                if limit is None:  # where every key of a row ties, the k lowest columns are kept
                    for b, c in enumerate(cases):
                        if ge.all_costs_tie(c):
                            n = c.shape[0]
                            assert (got["cols"][b, :n] == np.arange(k)).all() and (got["counts"][b, :n] == c.shape[1]).all()
                            assert (got["vals"][b, :n] == c.cost[0, 0]).all()
                            tied += 1
            third = ge.limits(cases)[1]
            counts = _lists(batch.candidates(k, third))["counts"]
            for b, c in enumerate(cases):  # exact equality at the case's magnitude: the 3rd smallest cost is admitted
                assert (counts[b, :c.shape[0]] >= 3).all(), (key, c.name)
        seen += len(cases)
    assert seen == len(ge.FAMILIES[family]()) and tied > 0


# ---- 4. the keyword route

ROUTE = dict(points=("c_subnormal_f32", "ulp_2_53"), whiten=("w_subnormal",), boxes=(ge.box_name(-525),))


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_keyword_route_is_the_ell_call_on_the_definitions_lists(family):
    seen = 0
    for key, cases in ge.by_key(ge.FAMILIES[family]()).items():
        cases = [c for c in cases if c.name in ROUTE[family]]
        if not cases:
            continue
        batch = _Batch(cases)
        assert len({ge.outside_stop(c) for c in cases}) == 1
        kw = dict(max_iter=ge.outside_stop(cases[0]), **ge.OUTSIDE_OPTS)
        outside = np.stack([ge.outside_rows(c) for c in cases])
        do = _dev(outside)
        x, y, w, shapes = batch.device()
        if family == "boxes":
            res = auction_solve_boxes_batch(x, y, batch.metric, shapes=shapes, outside=do, candidates=8, errors="status", **kw)
        else:
            res = auction_solve_points_batch(x, y, shapes=shapes, outside=do, candidates=8, whiten=w, errors="status", **kw)
        ell = batch.to_ell(8, outside)
        ref = auction_solve_ell_batch(_dev(ell["cols"]), _dev(ell["vals"]), rows=_dev(ell["rows"]), n_cols=batch.M,
                                      problem="min", outside=do, errors="status", **kw)
        _same_as_ell(res, ref)
        assert same_bytes(_lists(res["candidates"]), ell)
        assert (res["status"].cpu().numpy() == 0).all()
        assert res["truncated"].cpu().numpy().tolist() == (ell["counts"] > 8).sum(axis=1).tolist()
        seen += len(cases)
    assert seen == dict(points=2 * len(ge.POINT_DIMS), whiten=len(ge.WHITEN_DIMS), boxes=4)[family]


# ---- 5. the reverse finish behind a forward solve that ends at a subnormal eps

def _fully_assigned(entries, wants):
    return [(c, o) for (c, o), (want, m, n) in zip(entries, wants) if want["meta"]["n_assigned"] == n]


@pytest.mark.parametrize("problem", ge.PROBLEMS)
def test_reverse_finish_of_the_points_call_with_outside(problem):
    """finish="reverse" on every unwhitened points case whose forward solve (with outside, eps-scaled from C) ends with
    every row assigned, by the oracle: the numpy model on the forward outputs of the same call, bit for bit.  Among them
    c_subnormal_f32 and c_subnormal_tie, whose final_eps is a float32 subnormal.  (The whitened call has no finish of
    its own: finish="reverse" with whiten needs candidates=K.)"""
    names = set()
    for key, opts, stop, entries in ge.outside_groups(ge.points_cases()):
        picked = _fully_assigned(entries, ge.outside_want(key, opts, stop, entries, problem))
        if not picked:
            continue
        batch = _Batch([c for c, _ in picked])
        outside = np.stack([o for _, o in picked])
        x, y, _, _ = batch.device()
        r0, r1, want = pfin.check(x, y, problem=problem, outside=outside, max_iter=stop, **opts, **ge.OUTSIDE_OPTS)
        assert want["ran"].all() and (r0["status"].cpu().numpy() == 0).all()
        eps = pfin.df.records(r0)["final_eps"]
        for b, (c, _) in enumerate(picked):
            if c.name in ("c_subnormal_f32", "c_subnormal_tie"):
                assert 0 < float(eps[b]) < F32_TINY, (c.name, eps[b])
            names.add(c.name)
    assert {"c_subnormal_f32", "c_subnormal_tie"} <= names, names


@pytest.mark.parametrize("metric", ge.METRICS)
def test_reverse_finish_of_the_boxes_lists(metric):
    """Boxes have no finish kernel of their own: candidates=13 with finish="reverse" runs the ELL finish on the box
    lists.  Every float64 case whose forward solve on the lists ends with every row assigned, by the records of the
    same call, against the list model on that call's forward outputs."""
    ran = 0
    for key, cases in ge.by_key(ge.boxes_cases()).items():
        if key[2] != metric:
            continue
        for stop in sorted({ge.outside_stop(c) for c in cases}):
            batch = _Batch([c for c in cases if ge.outside_stop(c) == stop])
            outside = np.stack([ge.outside_rows(c) for c in batch.cases])
            a, b, _, shapes = batch.device()
            kw = dict(outside=_dev(outside), candidates=13, errors="status", max_iter=stop, **ge.OUTSIDE_OPTS)
            r0 = auction_solve_boxes_batch(a, b, metric, shapes=shapes, **kw)
            r1 = auction_solve_boxes_batch(a, b, metric, shapes=shapes, finish="reverse", **kw)
            ell = batch.to_ell(13, outside)
            assert same_bytes(_lists(r0["candidates"]), ell)
            want = lf.model_of(ell_to_packed(ell["cols"], ell["vals"], ell["rows"]), r0, problem="min", outside=outside,
                               max_iter=stop)
            lf.assert_is_the_model(r1, r0, want)
            ran += int(want["ran"].sum())
    assert ran > 0
