"""The edges of auction_solve_batch(finish="reverse") on the GPU: all 16 instances of k_dense_reverse_finish<T, Lay, Out>
(csrc/kernels_dense_batch.hpp), its top-two reduction, its row scan and cropped shapes, its open-object scan, outside
objects in the loop, and the values at which eps is lost to rounding (the stall rule).  The cases and what each of them
claims are in tests/_dense_finish_edges.py; tests/test_dense_finish_edges_nogpu.py holds every case to its claim on the
CPU oracle's forward state.

The yardstick is the one of tests/test_dense_finish.py: sslap_amd.dense_reverse_finish, the numpy model, applied to the
outputs of the SAME call with finish=None, and everything compared bit for bit (tests/_dense_finish.py:
assert_is_the_model).  No tolerance anywhere.  The case's claim is then checked on the model's trace of the GPU's own
forward outputs, so a case whose situation does not occur fails here too.
"""
import numpy as np
import pytest

from sslap_amd import auction_solve_batch
from tests import _dense_finish as df
from tests import _dense_finish_edges as de

pytestmark = pytest.mark.gpu


def _device_stack(case):
    """The case's stack on the device in its element type; "transposed": the same elements behind a row stride of 1."""
    import torch
    t = torch.from_numpy(np.array(case["mats"])).cuda().to(getattr(torch, case["dtype"]))
    if case["view"] == "transposed":
        t = t.transpose(1, 2).contiguous().transpose(1, 2)
        assert t.stride(1) == 1 and not t.is_contiguous()
    assert np.array_equal(t.double().cpu().numpy(), case["mats"], equal_nan=True)  # (exact in the type)
    return t


def _run(case):
    """Both calls, the model on the first one's outputs, the bit-for-bit comparison, then the case's claim on the GPU's
    own forward state.  Returns (finished result, model)."""
    stack = _device_stack(case)
    kw = dict(case["kw"], mat_dtype=case["dtype"])
    r0 = auction_solve_batch(stack, errors="status", **kw)
    r1 = auction_solve_batch(stack, errors="status", finish="reverse", **kw)
    trace = []
    want = df.model_of(stack, r0, trace=trace, **kw)
    df.assert_is_the_model(r1, r0, want)
    rec = df.records(r0)
    assert (df.host(r0["status"]) == 0).all() and want["ran"].all()
    fwd = dict(sol=df.host(r0["sol"]), prices=df.host(r0["prices"]), final_eps=rec["final_eps"], its=rec["its"])
    if "outside_prices" in r0:
        fwd["outside_prices"] = df.host(r0["outside_prices"])
    case["claim"](case, fwd, want, trace)
    return r1, want


@pytest.mark.parametrize("dtype,entries,out,view", de.A_PARAMS)
def test_every_instance(gpu_lib, dtype, entries, out, view):
    """3 x 70 x 90, two rows per lane (the second one partial): every element type with both entry rules, with and
    without an outside value per row, contiguous and behind a row stride of 1, min and max."""
    for problem in ("min", "max"):
        _, want = _run(de.instance_case(dtype, entries, out, view, problem))
        assert (want["reverse"]["its"] > 0).all()


@pytest.mark.parametrize("name", list(de.named_cases()))
def test_the_edge_cases(gpu_lib, name):
    case = de.case(name)
    r1, want = _run(case)
    if "figures" in case:  # the stall rule decided the outputs: its / left / eCE are the pinned figures on the GPU too
        _, its, left, ece = case["figures"]
        assert df.host(r1["reverse"]["its"]).tolist() == [its] and df.host(r1["reverse"]["left"]).tolist() == [left]
        assert df.records(r1)["eCE"].tolist() == [ece]
