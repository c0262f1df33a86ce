"""The cases of tests/_builder_edges.py, held to what they claim on the CPU (test_builder_edges.py runs them on the GPU).

  bisect_model   on hand-made key rows: the three branches, both exits, lim == 0, hi - lo == 1.
  the ladder     float64: the sorted keys are 0, 0, 1, 2, ... and the key of 1.69e308; with every cost as the limit hi
                 starts on every key; with every column stored twice T lands on key 0, key 1, key 2, ... and the
                 largest key in turn as the odd K run, by convergence, and on lim itself with the K-th cost as the limit.
  adjacent keys  the sorted keys of the row differ by exactly 1 each (float32 boxes: the searched gap, neighbours in the
                 row); without a limit the loop takes at least 50 steps and ends early on lo == mid == T (distinct K-th
                 and (K+1)-th keys cannot end otherwise); with the (K+1)-th cost as the limit hi starts at T + 1; with
                 the K-th column stored twice it converges onto T after >= 50 steps, keys at T - 1 and T + 1 beside it.
  both exits     per instance and K a case that ends early at step 1 and cases that converge after >= 50 steps.
  non-finite     K + 2 keys of 0: T = 0 without a step under limit = -1.0, T = 0 by bisection without a limit.
  the stacks     the case's row sits at rows 0 and 3, and wherever the row has at most K non-finite costs the fillers at
                 rows 1 and 2 are not truncated; the definition on every stack equals the plain-loop restatements
                 (ell_by_loops, ell_by_sorting).
  the laps       the definition on the tiled batch at a small B equals the tile; the lap shapes exceed cap(N).
"""
import math

import numpy as np
import pytest

from sslap_amd import boxes_to_dense, points_to_dense, points_to_ell
from tests import _builder_edges as be
from tests._boxes_fixture import ell_by_sorting
from tests._points_candidates import ell_by_loops, same_bytes

IDS = ["-".join(str(v) for v in inst if v) for inst in be.INSTANCES]


def _key(v):
    return be.cost_keys([v])[0]


def test_the_model_on_hand_made_rows():
    assert be.limit_key(None) == be.limit_key(math.inf) == be.KEY_INF
    assert be.limit_key(0.0) == 1 and be.limit_key(-0.0) == 1 and be.limit_key(5e-324) == 2
    assert be.limit_key(-1.0) == be.limit_key(math.nan) == be.limit_key(-math.nan) == be.limit_key(-math.inf) == 0
    assert be.cost_keys([0.0, 5e-324, math.inf, math.nan, 1.7976931348623157e308]) == [1, 2, 0, 0, be.KEY_INF]
    assert be.bisect_model([1, 2, 3], 3, 10) == (None, 3, 0, 0, "none")  # not more than K candidates
    assert be.bisect_model([0, 0, 0, 5], 2, 0) == (0, 0, 2, 0, "none")  # lim == 0: lo == hi on entry
    assert be.bisect_model([1, 2, 9], 2, 16) == (8, 0, 2, 1, "early")  # mid = 8 holds exactly 2
    assert be.bisect_model([4, 5, 9], 1, 5) == (4, 0, 1, 2, "early")  # mid = 2, then lo = 3, hi = 5: mid = 4 holds 1
    assert be.bisect_model([6, 7], 1, 7) == (6, 0, 1, 3, "early")  # 3, 5, then hi - lo == 1: mid == lo == 6
    T, under, ties, steps, how = be.bisect_model([7, 7, 7, 9], 2, 16)  # a tie across the K-th key: no midpoint holds 2
    assert (T, under, ties, how) == (7, 0, 2, "converged")
    T, under, ties, steps, how = be.bisect_model([3, 7, 7, 7], 2, 16)
    assert (T, under, ties, how) == (7, 1, 1, "converged")


def test_the_cap_restated():
    assert be.cap(1) == be.cap(3) == be.cap(256) == 65535 and be.cap(257) == 2 ** 22 // 65 and be.cap(2048) == 8192
    first, second = be.FIRST_CAP, be.SECOND_CAP
    assert first["B"] > be.cap(first["N"]) == 65535 and first["N"] <= 256
    assert second["B"] > be.cap(second["N"]) == 8192 and second["N"] > 256
    assert second["B"] * second["N"] >= 2 ** 24
    assert math.gcd(be.LAP_P, 65535) == 1 and math.gcd(be.LAP_P, 8192) == 1
    assert (np.arange(second["B"] - 8192) % 6 != (np.arange(second["B"] - 8192) + 8192) % 6).all()


def _held_to_the_model(case):
    """What holds of every case: untruncated, or T is the K-th smallest admitted key where the loop converged (or did
    not run), and a midpoint from that key up to, not including, the next where it ended early."""
    keys = sorted(k for k in be.cost_keys(be.case_costs(case)) if k <= be.limit_key(case["limit"]))
    K = case["K"]
    T, under, ties, steps, how = be.case_model(case)
    if len(keys) <= K:
        assert T is None and not case["claim"].get("truncated")
    elif how == "early":
        assert keys[K - 1] <= T < keys[K] and ties == K
    else:
        assert T == keys[K - 1] and under == sum(k < T for k in keys) < K and ties == K - under
        assert (how == "none") == (be.limit_key(case["limit"]) == 0)
    return T, steps, how


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("family", ["points", "whitened"])
def test_the_ladder_spans_the_key_range(family, dtype):
    f64 = dtype == "float64"
    costs = be.case_costs(be.ladder_cases(family, dtype, 1)[0])
    plain = be.case_costs(be.ladder_cases("points", dtype, 1)[0])
    if f64:
        assert costs[:2].tolist() == [0.0, 5e-324] and costs[5] == 1.0 and costs[8] == 1.3e154 * 1.3e154 > 1.6e308
        assert np.isposinf(costs[9]) and np.isnan(costs[10])
        assert costs.tobytes() == plain.tobytes()  # W = 2 I on halved columns: the very costs of the plain ladder
    else:
        assert costs[1] == 2.0 ** (-296 if family == "whitened" else -298)
        assert costs[8] == float(np.float32(3.4028234663852886e38)) ** 2 and not np.isfinite(costs[9:]).any()
        assert np.delete(costs, 1).tobytes() == np.delete(plain, 1).tobytes()
    keys = sorted(be.cost_keys(costs))
    assert keys[:3] == [0, 0, 1] and keys[3] == (2 if f64 else _key(costs[1])) and keys[-1] == _key(costs[8])
    assert len(set(keys[1:])) == 10
    landed = []
    for K in be.stack_ks("ladder"):
        cases = be.ladder_cases(family, dtype, K)
        assert len(cases) == (13 if K <= 10 else 2)
        for c in cases:
            _held_to_the_model(c)
        if K <= 10:
            assert [c["limit"] for c in cases[1:-2]] == np.sort(costs[:9]).tolist() + [math.inf]
            assert {be.limit_key(c["limit"]) for c in cases[1:-2]} == set(keys[2:]) | {be.KEY_INF}  # hi starts on every key
            T, steps, how = _held_to_the_model(cases[0])
            assert how == ("early" if K > 1 else "converged")  # (K = 1: the two keys of 0 tie across it)
        free, fenced = cases[-2:]
        T, steps, how = _held_to_the_model(free)
        if K % 2:  # the K-th key is stored twice across K: convergence onto it
            assert how == "converged" and T == keys[K // 2] and steps >= (50 if T < 2 ** 52 else 1)
            landed.append(T)
            T2, steps2, how2 = _held_to_the_model(fenced)
            assert T2 == T == be.limit_key(fenced["limit"]) and how2 == ("converged" if T else "none")  # T = lim itself
        else:
            assert how == ("early" if K > 2 else "converged")
    assert landed == [0] + keys[1:] and landed[-1] == _key(costs[8])  # key 0, key 1, (key 2,) ... the largest, in turn
    if f64:
        assert landed[:4] == [0, 0, 1, 2] and be.KEY_INF - landed[-1] < 2 ** 50  # T close under the key of +inf


@pytest.mark.parametrize("inst", be.INSTANCES, ids=IDS)
def test_adjacent_keys(inst):
    family, dtype, metric = inst
    x, y = be.adjacent_columns(family, dtype, metric)
    base = be.adjacent_cases(family, dtype, 1, metric)[0]
    keys = sorted(be.cost_keys(be.case_costs(base)))
    assert len(keys) == be.ADJACENT_M
    searched = family == "boxes" and dtype == "float32"
    if searched:
        a, b, at, gap = be.searched_boxes(metric)
        assert keys[at + 1] - keys[at] == gap == min(q - p for p, q in zip(keys, keys[1:]) if q > p)
        assert gap == {"iou": 8, "giou": 16}[metric]  # what the docstring of searched_boxes records
        assert (a == a.astype(np.float32)).all() and b.dtype == np.float32
    else:
        assert [q - p for p, q in zip(keys, keys[1:])] == [1] * (be.ADJACENT_M - 1)
    for K in be.stack_ks("adjacent"):
        free, limited, tied = be.adjacent_cases(family, dtype, K, metric)
        T, under, ties, steps, how = be.case_model(free)
        assert ties == K and (searched or T == keys[K - 1])
        if not searched:
            # distinct K-th and (K+1)-th keys can only end early (adjacent_cases says why): late, and on lo == mid == T
            assert keys[K] == T + 1 and how == "early" and steps >= 50
        elif K == at + 1:
            assert keys[K] == keys[K - 1] + gap and keys[K - 1] <= T < keys[K]  # the K-th and (K+1)-th keys: distinct, and neighbours in the row
        for c in (free, limited, tied):
            _held_to_the_model(c)
        assert be.limit_key(limited["limit"]) == keys[K]  # hi starts on the (K+1)-th key
        T2, _, _, steps2, how2 = be.case_model(limited)
        assert how2 == "early" and (searched or (T2 == T and steps2 >= 50))
        tkeys = sorted(be.cost_keys(be.case_costs(tied)))
        assert len(tkeys) == be.ADJACENT_M + 1 and tkeys[K - 1] == tkeys[K] == keys[K - 1]
        T3, under3, ties3, steps3, how3 = be.case_model(tied)
        assert (T3, under3, ties3, how3) == (keys[K - 1], K - 1, 1, "converged") and steps3 >= 50
        if not searched:
            assert (K == 1 or tkeys[K - 2] == T - 1) and tkeys[K + 1] == T + 1


@pytest.mark.parametrize("inst", be.INSTANCES, ids=IDS)
def test_both_exits_and_many_non_finite(inst):
    family, dtype, metric = inst
    for K in be.stack_ks("adjacent"):
        early = be.early_case(family, dtype, K, metric)
        T, under, ties, steps, how = be.case_model(early)
        assert (how, steps, ties, under) == ("early", 1, K, 0)
        fenced, free = be.many_non_finite_cases(family, dtype, K, metric)
        keys = be.cost_keys(be.case_costs(free))
        assert keys.count(0) == K + 2 and len(keys) == K + 5
        assert be.limit_key(fenced["limit"]) == 0 and be.case_model(fenced) == (0, 0, K, 0, "none")
        T, under, ties, steps, how = be.case_model(free)
        assert (T, under, ties) == (0, 0, K) and steps >= 60 and how == "converged"
        steps, how = be.case_model(be.adjacent_cases(family, dtype, K, metric)[2])[3:]  # and between two neighbours
        assert how == "converged" and steps >= 50


def _loops(s):
    """The plain-loop restatement of the definition on a stack."""
    if s["family"] == "boxes":
        return ell_by_sorting(boxes_to_dense(s["x"], s["y"], metric=s["metric"]), s["K"], s["shapes"], s["limit"])
    if s["w"] is None:
        return ell_by_loops(s["x"], s["y"], s["K"], s["shapes"], s["limit"])
    return ell_by_sorting(points_to_dense(s["x"], s["y"], whiten=s["w"]), s["K"], s["shapes"], s["limit"])


@pytest.mark.parametrize("inst", be.INSTANCES, ids=IDS)
def test_the_stacks_place_every_case_and_the_definition_is_the_loop(inst):
    family, dtype, metric = inst
    for group in be.stack_groups(family):
        for K in be.stack_ks(group):
            cases = be.stack_cases(family, dtype, metric, group, K)
            s = be.stack(cases)
            want = be.stack_to_ell(s)
            assert same_bytes(want, _loops(s))
            assert s["x"].shape[1] == be.ROWS == 4 and s["y"].shape[1] == be.STACK_M and (want["rows"] == 4).all()
            truncated = 0
            for b, c in enumerate(cases):
                assert (s["x"][b] == c["x"]).all() and s["shapes"][b, 1] == len(c["y"])
                T = be.case_model(c)[0]
                counts = want["counts"][b]
                assert counts[0] == counts[3] and (counts[0] > K) == (T is not None)  # wavefronts 0 and 3
                assert want["cols"][b, 0].tobytes() == want["cols"][b, 3].tobytes()
                truncated += T is not None
                if c["claim"].get("truncated"):
                    assert T is not None
                non_finite = be.cost_keys(be.case_costs(c)).count(0)
                assert counts[1] == counts[2] == non_finite
                if non_finite <= K:
                    assert counts[1] <= K  # an untruncated row in the truncated row's workgroup
            assert truncated >= 1
            free = be.stack(cases, no_limit_only=True)
            assert free["limit"] is None and 1 <= len(free["cases"]) < len(cases)
            assert same_bytes(be.stack_to_ell(free), _loops(free))


@pytest.mark.parametrize("inst", be.INSTANCES[::2] + be.INSTANCES[-1:], ids=IDS[::2] + IDS[-1:])
def test_the_lap_batch_is_the_tile_of_its_seven_problems(inst):
    family, dtype, metric = inst
    lap = be.lap_batch(family, dtype, 23, 3, 5, 2, metric)
    assert lap["x"].shape[0] == 23 and (lap["x"][7:14] == lap["base"]["x"]).all()
    assert lap["shapes"][4].tolist() == [4, 5] and lap["shapes"][18].tolist() == [4, 5]  # the bad shape, on a later lap too
    direct = be.to_ell(family, lap["x"], lap["y"], 2, lap["shapes"], lap["limit"], lap["w"], metric)
    assert same_bytes(direct, lap["want"])
    assert lap["want"]["rows"][:7].tolist() == [3, 1, 3, 3, 0, 2, 3]
    assert (lap["want"]["cols"][4] == -1).all() and not lap["want"]["counts"][4].any()
    lim = lap["base"]["limit"]
    assert np.isnan(lim).any() and np.isposinf(lim).any() and (np.signbit(lim) & (lim == 0)).any() and (lim == -1).any()
    assert (lap["want"]["counts"] > 2).any() and (lap["want"]["counts"] == 0).any()
    seven = [{key: lap["want"][key][p].tobytes() for key in be.KEYS} for p in range(7)]
    assert all(seven[p] != seven[q] for p in range(7) for q in range(p))  # distinct: a mis-stepped lap cannot agree


def test_the_second_cap_problem():
    p = be.second_cap_problem()
    N, B = be.SECOND_CAP["N"], be.SECOND_CAP["B"]
    assert p["x"].shape == (1, N, 1) and p["y"].shape == (1, 2, 1) and p["combo"].shape == (B,)
    want = p["want6"]
    assert want["rows"].tolist() == [N, N - 1, 1, 0, N, 5]
    assert (want["counts"][0] == 2).all() and (want["cols"][3] == -1).all() and not want["counts"][5, 5:].any()
    assert len({b"".join(want[key][c].tobytes() for key in be.KEYS) for c in range(6)}) == 6
    for c in (0, 4):  # a single problem, stated alone
        one = points_to_ell(p["x"], p["y"], 1, p["shapes6"][c:c + 1].clip(max=[N, 2]), p["limit6"][c:c + 1])
        assert one["cols"][0].tobytes() == want["cols"][c].tobytes()
