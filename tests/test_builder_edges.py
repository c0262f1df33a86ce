"""The three candidate builders on the GPU where no other test puts them (the cases: tests/_builder_edges.py, held to
their claims by test_builder_edges_nogpu.py): points_candidates(..., whiten=) and boxes_candidates(..., metric=)
against points_to_ell / boxes_to_ell, every output byte of cols, vals, counts and rows.

  bisection   per instance (points and whitened in float64 / float32, boxes float64 / float32 x iou / giou) and per K one
              stacked batch with per-row limits, and the cases without a limit once more with limit=None: the key-range
              ladder, plain and with every column twice (T on key 0, 1, 2, ... the largest, and on lim itself), adjacent
              keys (late early exit on hi - lo == 1; convergence between two neighbours), the early exit at step 1, K + 2
              costs that are not finite (lim = 0 and T = 0 by bisection); every case at wavefronts 0 and 3 beside rows
              that are not truncated.
  first cap   B = 65535 + 9 problems of 3 x 5 (gridDim.y = 65535): the second lap of the loop over problems in all three
              kernels, with the idle fourth wavefront, a bad device shape, per-row limits.
  second cap  B = 8192 + 3 problems of 2048 x 2 (gridDim.y = 2^22 / 512) from stride-0 views, k_points_candidates<float>.
  route       auction_solve_points_batch(candidates=2, outside=) at B = 65535 + 9 against the ELL call on the uploaded
              lists of the definition.
"""
import faulthandler

import numpy as np
import pytest

from sslap_amd import auction_solve_ell_batch, auction_solve_points_batch, boxes_candidates, points_candidates
from tests import _builder_edges as be
from tests.test_points_candidates import _same_as_ell

pytestmark = pytest.mark.gpu

IDS = ["-".join(str(v) for v in inst if v) for inst in be.INSTANCES]
WANT = dict(cols=np.int32, vals=np.float64, counts=np.int32, rows=np.int32)


@pytest.fixture(autouse=True)
def _time_limit():
    """A test that hangs ends the process (with a traceback) instead of holding the GPU."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _build(family, x, y, K, shapes=None, limit=None, w=None, metric=None):
    """The family's builder on device tensors; the four arrays back on the host."""
    if family == "boxes":
        got = boxes_candidates(x, y, K, shapes=shapes, limit=limit, metric=metric)
    else:
        got = points_candidates(x, y, K, shapes=shapes, limit=limit, whiten=w)
    for key in be.KEYS:
        assert got[key].is_cuda and got[key].is_contiguous(), key
    return {key: got[key].cpu().numpy() for key in be.KEYS}


def _same(got, want, what):
    for key in be.KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype == WANT[key] and g.shape == w.shape, (what, key)
        assert g.tobytes() == w.tobytes(), (what, key, np.flatnonzero(g.ravel() != w.ravel())[:8])


# ---- the bisection of the truncated path

@pytest.mark.parametrize("inst", be.INSTANCES, ids=IDS)
def test_bisection_edges(gpu_lib, inst):
    family, dtype, metric = inst
    truncated = 0
    for group in be.stack_groups(family):
        for K in be.stack_ks(group):
            cases = be.stack_cases(family, dtype, metric, group, K)
            for s in (be.stack(cases), be.stack(cases, no_limit_only=True)):
                got = _build(family, _dev(s["x"]), _dev(s["y"]), K, shapes=s["shapes"], limit=s["limit"], w=_dev(s["w"]),
                             metric=metric)
                _same(got, be.stack_to_ell(s), (group, K, s["limit"] is None))
                for b, c in enumerate(s["cases"]):  # the claim, on what came back
                    claimed = be.case_model(c)[0] is not None
                    assert (got["counts"][b, 0] > K) == (got["counts"][b, 3] > K) == claimed, c["name"]
                    assert claimed or not c["claim"].get("truncated"), c["name"]
                    truncated += claimed
    assert truncated > 50


# ---- batches past the grid's y extent

def _lap(family, dtype, metric=None):
    return be.lap_batch(family, dtype, metric=metric, **be.FIRST_CAP)


@pytest.mark.parametrize("family, dtype, metric", [("points", "float64", None), ("points", "float32", None),
                                                   ("whitened", "float32", None), ("boxes", "float64", "giou")])
def test_second_lap_under_the_first_cap(gpu_lib, family, dtype, metric):
    lap = _lap(family, dtype, metric)
    B, K = be.FIRST_CAP["B"], be.FIRST_CAP["K"]
    assert lap["x"].shape[0] == B > be.cap(be.FIRST_CAP["N"])
    got = _build(family, _dev(lap["x"]), _dev(lap["y"]), K, shapes=_dev(lap["shapes"]), limit=_dev(lap["limit"]),
                 w=_dev(lap["w"]), metric=metric)
    _same(got, lap["want"], family)
    bad = np.flatnonzero((np.arange(B) % be.LAP_P) == 4)
    assert (bad >= 65535).any() and (lap["shapes"][bad] == [be.FIRST_CAP["N"] + 1, be.FIRST_CAP["M"]]).all()
    assert not got["rows"][bad].any() and (got["cols"][bad] == -1).all() and not got["vals"][bad].any()
    assert not got["counts"][bad].any()
    assert (got["counts"][65535:] > K).any() and got["rows"][65535:].tolist() == lap["want"]["rows"][65535 % be.LAP_P:][:9].tolist()


def test_second_lap_under_the_second_cap(gpu_lib):
    """B N >= 2^24 rows: the outputs take 270 MB and are compared on the device, as integers (bit for bit)."""
    import torch
    p = be.second_cap_problem()
    B, N, M, K = (be.SECOND_CAP[key] for key in ("B", "N", "M", "K"))
    assert B > be.cap(N)
    x, y = _dev(p["x"]).expand(B, N, 1), _dev(p["y"]).expand(B, M, 1)
    assert x.stride(0) == 0 and y.stride(0) == 0
    combo = _dev(p["combo"])
    got = points_candidates(x, y, K, shapes=_dev(p["shapes6"])[combo].contiguous(), limit=_dev(p["limit6"])[combo].contiguous())
    for key in be.KEYS:
        want = _dev(p["want6"][key])[combo]
        g = got[key]
        assert g.shape == want.shape and g.dtype == want.dtype, key
        if key == "vals":
            g, want = g.view(torch.int64), want.view(torch.int64)
        assert torch.equal(g, want), (key, torch.nonzero(g != want)[:8].tolist())
    assert got["rows"][8192:].tolist() == p["want6"]["rows"][p["combo"][8192:]].tolist()


# ---- the route

def test_the_keyword_route_past_the_first_cap(gpu_lib):
    lap = _lap("points", "float32")
    B, M, K = be.FIRST_CAP["B"], be.FIRST_CAP["M"], be.FIRST_CAP["K"]
    x, y, shapes, outside = _dev(lap["x"]), _dev(lap["y"]), _dev(lap["shapes"]), _dev(lap["limit"])
    res = auction_solve_points_batch(x, y, outside=outside, candidates=K, shapes=shapes, errors="status")
    want = lap["want"]
    ref = auction_solve_ell_batch(_dev(want["cols"]), _dev(want["vals"]), rows=_dev(want["rows"]), n_cols=M, problem="min",
                                  outside=outside, errors="status")
    _same_as_ell(res, ref)
    _same({key: res["candidates"][key].cpu().numpy() for key in be.KEYS}, want, "candidates")
    assert res["truncated"].cpu().numpy().tolist() == (want["counts"] > K).sum(axis=1).tolist()
    status = res["status"].cpu().numpy()
    assert status.shape == (B,) and (status[:be.LAP_P] == status[65534:65534 + be.LAP_P]).all()  # 65534 = 7 * 9362
    assert (status == 0).any() and (status != 0).any()
