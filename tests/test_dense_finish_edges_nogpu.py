"""The edge cases of tests/test_dense_finish_edges.py without a GPU: every case of tests/_dense_finish_edges.py is held to
what it claims.  The forward state is the CPU oracle's (the GPU's forward solve is pinned to it bit for bit elsewhere),
the finish is sslap_amd.dense_reverse_finish with trace=, and the case's claim is asserted on that trace: a case whose
situation does not occur fails.  Cases inside the documented range of the finish (max(|a|, |p|) * 2**-52 < eps) are also
held to the structure of a finished state and to scipy's optimum; and the stall rule of the model is stated directly.
"""
import numpy as np
import pytest

from sslap_amd import dense_reverse_finish
from tests import _dense_finish_edges as de


def test_all_16_instances_are_in_the_parametrisation():
    triples = {(t, e, o) for t, e, o, _ in de.A_PARAMS}
    assert triples == {(t, e, o) for t in ("float64", "float32", "float16", "bfloat16") for e in ("nonneg", "finite")
                       for o in (False, True)} and len(triples) == 16
    for triple in triples:  # each one contiguous and behind a row stride of 1
        assert {v for t, e, o, v in de.A_PARAMS if (t, e, o) == triple} == {"contiguous", "transposed"}
    assert len(de.A_PARAMS) == 32 == len(set(de.A_PARAMS))


@pytest.mark.parametrize("dtype", de.TYPES)
def test_the_instance_values_are_exact_in_every_type(dtype):
    for entries in ("nonneg", "finite"):
        mats = de.instance_case(dtype, entries, True, "contiguous", "max")["mats"]
        if dtype == "bfloat16":  # (numpy has none: a float32 whose low 16 bits are zero)
            f32 = mats.astype(np.float32)
            back = (f32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
        else:
            back = mats.astype(dtype).astype(np.float64)
        assert np.array_equal(back, mats, equal_nan=True)
        assert np.isnan(mats).any() == (entries == "finite") and (entries == "finite" or (mats == -1.0).any())
        assert mats.shape == (3, 70, 90)


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("out", [False, True])
@pytest.mark.parametrize("entries", ["nonneg", "finite"])
def test_every_instance_has_work(entries, out, problem):
    """(the element type and the view do not change the values: one twin per entry rule, outside and problem)"""
    case = de.instance_case("float64", entries, out, "contiguous", problem)
    fwd, res, _ = de.twin(case)
    assert (res["reverse"]["its"] > 0).all() and (res["reverse"]["left"] == 0).all()
    de.assert_in_range_properties(case, fwd, res)


@pytest.mark.parametrize("name", list(de.named_cases()))
def test_the_case_meets_its_claim(name):
    case = de.case(name)
    with np.errstate(all="ignore"):
        fwd, res, _ = de.twin(case)
        if case["in_range"]:
            de.assert_in_range_properties(case, fwd, res)


def test_the_named_cases_cover_the_sections():
    names = list(de.named_cases())
    assert [n for n in names if n.startswith("B-")] == ["B-130", "B-65", "B-257"]
    assert {"C-cropped-plain", "C-cropped-outside", "C-square-255", "C-square-256", "C-square-257", "D-scan",
            "E-outside-loop"} <= set(names)
    assert len([n for n in names if n.startswith("F-")]) == len(de.F_NAMES) == 12
    sets = [s for s, near in de.reduction_case(130)["sets"]]
    for want in [(5, 70), (3, 67), (3, 67, 129), (8, 40), (128, 129, 1), (0,), (129,)]:
        assert want in sets
    for off in (1, 2, 4, 8, 16, 32):
        assert (de.B_LANE, de.B_LANE ^ off) in sets and (de.B_LANE ^ off) < 130
    assert [near for s, near in de.reduction_case(130)["sets"] if near != "tie"] == list(de.B_NEAR[1:])
    assert de.C_ROWS == (1, 63, 64, 65, 127, 128, 129, 130) and de.D_EMPTY == (0, 62, 63, 64, 65, 127, 128, 199)
    # every values case passes the budget that ends even a kernel without the stall rule
    assert all(de.case("F-" + n)["kw"]["max_iter"] == 5000 for n in de.F_NAMES)


def test_two_values_cases_end_with_ece_0_after_the_finish_ran():
    """There the eCE `bad` path of the kernel decides an output."""
    zero = [n for n in de.F_TABLE if de.twin(de.case("F-" + n))[1]["eCE"][0] == 0]
    assert len(zero) >= 2, zero


@pytest.mark.parametrize("name", list(de.F_TABLE))
def test_without_the_stall_rule_these_cases_would_run_to_the_budget_or_on(name):
    """The rule is what ends them: the iteration at which the model stops is one whose move would leave the moving row's
    profit where it was (or below), the state the termination argument of the finish excludes."""
    case = de.case("F-" + name)
    fwd = de.forward(case)
    res, trace = de.model(case, fwd)
    b, j, i, freed, _ = trace[-1]
    assert i >= 0 and freed == -1 and res["reverse"]["left"][0] > 0
    a, valid, p, p2o = de.augmented(case, res, 0)  # (a stall writes nothing: the state is the one it met)
    eps = float(fwd["final_eps"][0])
    lam = de.augmented(case, fwd, 0)[2][de.augmented(case, fwd, 0)[3]].min()
    with np.errstate(all="ignore"):
        pi = a[np.arange(a.shape[0]), p2o] - p[p2o]
        w = np.where(valid[:, j], a[:, j] - pi, -np.inf)
    assert int(np.argmax(w)) == i
    pj = max(lam, np.delete(w, i).max() - eps)
    assert not (a[i, j] - pj > pi[i]) and lam < w[i] - eps
    assert res["reverse"]["left"][0] == np.count_nonzero((p > lam) & ~np.isin(np.arange(p.size), p2o)) and p[j] > lam


def test_a_stalled_iteration_is_counted_and_changes_nothing():
    """Two rows, three objects, eps far below one ulp of the values.  Both rows hold profit 0 and tie for object 2 at
    w = 2 * big, so its price would be 2 * big - eps == 2 * big and row 0's profit 0 again: the finish ends there with
    its = 1, left = 1 (object 2 itself), nothing rewritten."""
    big = 2.0 ** 60
    mats = np.array([[[big, -1.0, 2 * big], [-1.0, big, 2 * big]]])
    sol, prices = np.array([[0, 1]], dtype=np.int32), np.array([[big, big, 3 * big]])
    trace = []
    res = dense_reverse_finish(mats, sol, prices, np.array([0.5], dtype=np.float32), problem="max", trace=trace)
    assert trace == [(0, 2, 0, -1, False)]
    assert res["reverse"]["its"].tolist() == [1] and res["reverse"]["left"].tolist() == [1]
    assert res["sol"].tolist() == [[0, 1]] and res["prices"].tolist() == [[big, big, 3 * big]]
