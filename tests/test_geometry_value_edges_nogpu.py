"""The cases of tests/_geometry_value_edges.py on the CPU: the definitions and the oracle alone.  Every case must reach
the edge it is named for -- otherwise test_geometry_value_edges.py, which only compares the library with the oracle on
the definition's stack, would pass without the check passes and the cost chains of the points, whitened and boxes batch
ever seeing that edge -- and every oracle solve must end within its stop, so that no workgroup is sent into a solve
that only the default max_iter would end.

Also here: the definitions against their plain-loop restatements at these magnitudes (a NumPy that flushed subnormals,
or a vectorised chain that fused or reordered, would show), the per-scale properties of the box costs, and that the
augmented and the list routes hand the oracle the same problem.
"""
import numpy as np

from sslap_amd import boxes_to_dense, boxes_to_ell, dense_to_augmented, ell_to_packed, points_to_dense, points_to_ell
from tests import _boxes_fixture as bf
from tests import _geometry_value_edges as ge
from tests import _points_fixture as pf
from tests import _points_whiten as pw
from tests import _value_edges as ve
from tests._batch_shapes import bits
from tests._points_candidates import same_bytes

F32_TINY = float(np.finfo(np.float32).tiny)  # the smallest normal float32
DBL_TINY = float(np.finfo(np.float64).tiny)
N, M = ge.N, ge.M

POINT_NAMES = ("above_flt_max", "dbl_max", "c_is_zero", "zeros", "c_subnormal_f32", "c_subnormal_tie", "ulp_2_53",
               "ties_2_52") + tuple(n for n, _, _ in ve.EPS_STARTS)
WHITEN_NAMES = ("w_subnormal", "w_split", "w_above_flt_max", "w_zero")
BOX_NAMES = tuple(ge.box_name(e) for e in ge.BOX_SCALES) + ("identical", "disjoint")


def _f32(x):
    with np.errstate(over="ignore"):
        return np.float32(x)


def test_no_case_is_left_out():
    pts = ge.points_cases()
    for D in ge.POINT_DIMS:
        names = tuple(c.name for c in pts if c.key == ("points", "float64", D, (N, M)))
        assert names == tuple(n for n in POINT_NAMES if n != "c_subnormal_tie" or D == 2), D
    for D in ge.F32_DIMS:
        assert [c.name for c in pts if c.key == ("points", "float32", D, (N, M))] == ["f32_subnormal_coords", "f32_big_coords"]
    assert len(pts) == 3 * 11 + 1 + 2 * 2
    for D in ge.WHITEN_DIMS:
        assert tuple(c.name for c in ge.whiten_cases() if c.key[2] == D) == WHITEN_NAMES
    assert len(ge.whiten_cases()) == 8
    for metric in bf.METRICS:
        for size in (ge.SMALL, (N, M)):
            assert tuple(c.name for c in ge.boxes_cases() if c.key == ("boxes", "float64", metric, size)) == BOX_NAMES
        assert [c.name for c in ge.boxes_cases() if c.key[1] == "float32" and c.key[2] == metric] == ["f32_subnormal_coords"]
    assert len(ge.boxes_cases()) == 2 * (2 * 7 + 1)
    for c in ge.all_cases():
        # the 40 x 56 shape (the boxes also 9 x 13), no holes, every stop one of _value_edges', explicit and small
        assert c.shape in ((N, M), ge.SMALL) and c.cost.shape == c.shape and c.x.shape[0] >= c.shape[0], ge.case_id(c)
        assert c.stop in {s for _, _, s in ve.MAGNITUDES + ve.EPS_STARTS}, ge.case_id(c)
        assert c.stop is None or c.stop <= 300 or c.name == "eps_1e-45"
        assert c.x.dtype == c.y.dtype == np.dtype(c.key[1]) and (c.w is None or c.w.dtype == c.x.dtype)
        assert (c.name in ge.NEVER_ENDS) <= (c.stop is not None)
    # the whitened cases lie inside a larger stack whose surplus holds NaN, as do all the upper triangles
    for c in ge.whiten_cases():
        D = c.key[2]
        assert c.x.shape == (N + 2, D) and c.y.shape == (M + 3, D) and c.w.shape == (N + 2, D, D) and c.shape == (N, M)
        assert np.isnan(c.x[N:]).all() and np.isnan(c.y[M:]).all() and np.isnan(c.w[N:]).all()
        upper = ~np.tril(np.ones((D, D), dtype=bool))
        assert np.isnan(c.w[:N][:, upper]).all() and np.isfinite(c.w[:N][:, ~upper]).all()
    # one batch per (key, eps_start, stop): a workgroup that spins at eps == 0 or eps == +inf runs beside another one
    for family in ge.FAMILIES.values():
        gs = ge.groups(family())
        assert sum(len(cs) for _, _, _, cs in gs) == len(family())
        assert all(len({c.key for c in cs}) == 1 for _, _, _, cs in gs)
    by_names = [{c.name for c in cs} for _, _, _, cs in ge.groups(ge.points_cases())]
    assert {"c_is_zero", "zeros"} in by_names and {"above_flt_max", "dbl_max"} in by_names
    assert {"c_subnormal_f32", "c_subnormal_tie"} in by_names and {"ulp_2_53", "ties_2_52"} in by_names


def test_every_oracle_solve_ends_within_its_stop():
    """its == stop for a case that is cut, eCE == 1 below the stop for one that ends; never a solve that ran into the
    default max_iter.  A case of NEVER_ENDS is cut in every variant, one without a stop ends in fewer than 1000 rounds in
    every variant, each of the others is cut or ends below its stop."""
    cut = {}
    for c in ge.all_cases():
        for problem in ge.PROBLEMS:
            want = ge.want(c, problem)
            its, ece, key = want["meta"]["its"], want["meta"]["eCE"], (ge.case_id(c), problem)
            print(key, "its", its, "eCE", ece, "stop", c.stop)
            if c.stop is None:
                assert ece == 1 and its < 1000, key
            elif c.name in ge.NEVER_ENDS:
                assert its == c.stop and ece == 0, key
            else:
                assert (its == c.stop and ece == 0) or (its < c.stop and ece == 1), key
                cut[c.name] = cut.get(c.name, False) or its == c.stop
    assert cut == dict.fromkeys(("c_is_zero", "ulp_2_53", "ties_2_52", "eps_1e-45", "eps_3e38", "f32_subnormal_coords"), True)
    assert ge.ENDS_LATE == ()
    seen = 0
    for family in ge.FAMILIES.values():
        for key, opts, stop, entries in ge.outside_groups(family()):
            assert stop is not None and (stop <= 300 or opts.get("eps_start") == 1e-45)
            for problem in ge.PROBLEMS:
                for (c, o), (want, m, n) in zip(entries, ge.outside_want(key, opts, stop, entries, problem)):
                    its, ece = want["meta"]["its"], want["meta"]["eCE"]
                    print("outside", ge.case_id(c), problem, o[1], "its", its, "eCE", ece, "stop", stop)
                    assert (n, m) == c.shape and ((its == stop and ece == 0) or (its < stop and ece == 1))
                    seen += 1
    assert seen == 2 * (len(ge.all_cases()) + len(ge.C_FROM_OUTSIDE))


def test_every_case_reaches_the_edge_it_is_named_for():
    seen = set()
    for c in ge.all_cases():
        cid = ge.case_id(c)
        assert np.isfinite(c.cost).all() and not np.signbit(c.cost).any(), cid
        c64 = float(c.cost.max())
        c32 = _f32(c64)
        for problem in ge.PROBLEMS:
            want = ge.want(c, problem)
            key = (cid, problem)
            start, final, p = _f32(want["extra"]["start_eps_f32"]), _f32(want["extra"]["final_eps_f32"]), want["p"]
            assert not np.isnan(p).any() and not np.signbit(p).any(), key
            if not c.opts or c.name == "eps_1e-46":
                with np.errstate(over="ignore"):
                    assert start.view(np.uint32) == _f32(np.float64(c32) / 2.0).view(np.uint32), key  # eps = (float)(C / 2)
            if c.name in ("above_flt_max", "dbl_max", "f32_big_coords", "w_above_flt_max"):
                assert c64 > ve.FLT_MAX and np.isinf(c32) and np.isinf(start) and np.isinf(final), key
                assert np.isinf(p).any() and set(np.unique(p)) <= {0.0, np.inf}, key
                if c.name == "dbl_max":  # within a factor of 8 of DBL_MAX, and the chain did not overflow
                    assert ve.DBL_MAX / 8 < c64 <= ve.DBL_MAX, key
            elif c.name == "c_is_zero":
                assert 0 < c64 < 2.0 ** -150 and c32 == 0 and start == 0 and final == 0, key
                assert (c.cost > 0).sum() >= c.cost.size - N, key
            elif c.name in ("zeros", "w_zero", "identical"):
                assert (bits(c.cost) == 0).all() and start == 0 and (p == 0).all(), key  # every cost is +0.0
            elif c.name in ("c_subnormal_f32", "w_subnormal"):
                assert 0 < float(c32) < F32_TINY and 0 < float(start) < F32_TINY and want["meta"]["eCE"] == 1, key
                assert want["meta"]["n_assigned"] == N and 0 < float(final) < F32_TINY, key
            elif c.name == "c_subnormal_tie":
                assert c64 == 74 * 2.0 ** -152 == 9.25 * 2.0 ** -149 and (c.cost == c64).sum() >= 1, key
                assert float(c32) == 9 * 2.0 ** -149 and start.view(np.uint32) == 4 and final.view(np.uint32) == 4, key
                assert float(_f32(c64 / 2.0)) == 5 * 2.0 ** -149, key  # halved before narrowing: the odd neighbour
                assert want["meta"]["n_assigned"] == N and want["meta"]["eCE"] == 1, key
            elif c.name == "ulp_2_53":
                assert c64 > 2.0 ** 53 and want["meta"]["nreductions"] >= 17 and p.max() > 2.0 ** 53, key
                assert float(final) < np.spacing(p.max()), key  # eps below one ulp of a price: costbest - w + eps rounds
            elif c.name == "ties_2_52":
                assert (np.fmod(c.cost, 2.0 ** 50) == 0).all() and 2.0 ** 57 <= c64 <= 8 * 225 * 2.0 ** 50, key
                assert len(np.unique(c.cost)) < c.cost.size / 3, key  # exact ties
            elif c.name == "eps_1e-46":
                assert _f32(1e-46) == 0 and float(start) > 1 and want["meta"]["nreductions"] >= 2, key
            elif c.name == "eps_1e-45":
                assert start.view(np.uint32) == 1 and final.view(np.uint32) == 1 and want["meta"]["nreductions"] == 0, key
            elif c.name == "eps_3e38":
                assert start == _f32(3e38) and np.isfinite(p).all() and p.max() > ve.FLT_MAX, key
            elif c.name == "eps_1e39":
                assert np.isinf(start) and np.isinf(final) and np.isinf(p).any(), key
            elif c.name == "f32_subnormal_coords" and c.family == "points":
                assert 0 < c64 < 1e-80 and c32 == 0 and start == 0 and final == 0, key
            elif c.name == "w_split":  # the magnitude is split between W and the coordinates; the products are ordinary
                tri = c.w[:N][np.isfinite(c.w[:N])]
                assert np.abs(tri).max() < 2.0 ** -478 and np.abs(c.x[:N]).max() > 2.0 ** 498, key
                assert 1e9 < c64 < 1e15 and want["meta"]["eCE"] == 1, key
            elif c.family == "boxes":
                assert 0.0 < c64 <= 2.0 and want["meta"]["eCE"] == 1, key
            else:
                raise AssertionError(key)
        seen.add(c.name)
    assert seen == set(POINT_NAMES + WHITEN_NAMES + BOX_NAMES) | {"f32_subnormal_coords", "f32_big_coords"}


def test_the_subnormal_float32_coordinates_are_widened_exactly():
    """Every non-zero coordinate is a float32 subnormal; the definition's stack, from exactly widened values, holds
    more than 1000 distinct non-zero costs, so a kernel that flushed them (every cost +0.0) cannot agree by accident."""
    cases = [c for c in ge.all_cases() if c.name == "f32_subnormal_coords"]
    assert len(cases) == len(ge.F32_DIMS) + len(bf.METRICS)
    for c in cases:
        for a in (c.x, c.y):
            assert a.dtype == np.float32 and (np.abs(a[a != 0]) < F32_TINY).all() and (a != 0).mean() > 0.99
            assert (a.astype(np.float64) * 2.0 ** 149 == np.rint(a.astype(np.float64) * 2.0 ** 149)).all()
        if c.family == "points":
            assert len(np.unique(c.cost[c.cost != 0])) > 1000, ge.case_id(c)
            assert np.array_equal(bits(c.cost), bits(pf.dense_by_loops(c.x[None], c.y[None])[0]))
        else:  # the costs of the widened values, and of the widened values scaled back by 2^140 (exact, nothing under- or
            # overflows in float64): the loop restatement, bit for bit
            metric = ge.metric_of(c)
            wide = (c.x.astype(np.float64)[None], c.y.astype(np.float64)[None])
            assert np.array_equal(bits(c.cost), bits(bf.dense_by_loops(*wide, metric=metric)[0])), ge.case_id(c)
            back = bf.dense_by_loops(wide[0] * 2.0 ** 140, wide[1] * 2.0 ** 140, metric=metric)[0]
            assert np.array_equal(bits(c.cost), bits(back)), ge.case_id(c)
            assert len(np.unique(c.cost)) > 1000


def test_the_box_costs_per_scale():
    """What the scales are for: subnormal areas with finite costs that differ from the unscaled ones (the divisions see
    subnormal operands), areas of 0 with one cost value, and the last scale at which nothing overflows."""
    for metric in bf.METRICS:
        for size in (ge.SMALL, (N, M)):
            a, b = ge.box_base(size)
            base = boxes_to_dense(a[None], b[None], metric=metric)[0]
            cases = {c.name: c for c in ge.boxes_cases() if c.key == ("boxes", "float64", metric, size)}
            for e in ge.BOX_SCALES:
                c = cases[ge.box_name(e)]
                key = (metric, size, e)
                area = np.concatenate([(t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1]) for t in (c.x, c.y)])
                width = np.concatenate([t[:, 2] - t[:, 0] for t in (c.x, c.y)])
                assert np.isfinite(c.cost).all(), key
                differ = float((bits(c.cost) != bits(base)).mean())
                print(key, "costs that differ from the unscaled stack:", differ, "distinct:", len(np.unique(c.cost)))
                if e in (-515, -525, -537):
                    assert (width >= DBL_TINY).all() and (area < DBL_TINY).all() and (area > 0).any(), key
                    assert differ >= 1 / 3, key
                elif e == -540:
                    assert (area == 0).all() and (bits(c.cost) == bits(np.float64(1.0))).all(), key
                else:
                    assert e == 510 and differ == 0.0, key
                    with np.errstate(over="ignore"):  # ... and one more doubling overflows a sum
                        assert np.isinf(boxes_to_dense(c.x[None] * 2.0, c.y[None] * 2.0, metric=metric)).any(), key
            assert (bits(cases["identical"].cost) == 0).all()
            d = cases["disjoint"].cost
            if metric == "iou":
                assert (bits(d) == bits(np.float64(1.0))).all()  # everything ties
            else:
                assert ((d > 1.0) & (d <= 2.0)).all() and d.max() > 1.99


def _slice(c, n=5, m=7):
    """The first 5 x 7 of a case (the loops are slow), as one-problem batches."""
    return c.x[None, :n], c.y[None, :m], None if c.w is None else c.w[None, :n]


def test_the_definitions_agree_with_the_plain_loops():
    for c in ge.all_cases():
        x, y, w = _slice(c)
        cid = ge.case_id(c)
        if c.family == "boxes":
            cost = boxes_to_dense(x, y, metric=ge.metric_of(c))
            loops = bf.dense_by_loops(x, y, metric=ge.metric_of(c))
        elif c.family == "whiten":
            cost = points_to_dense(x, y, whiten=w)
            loops = pw.whitened_by_loops(x, y, w)
        else:
            cost = points_to_dense(x, y)
            loops = pf.dense_by_loops(x, y)
        assert np.array_equal(bits(cost), bits(loops)) and np.array_equal(bits(cost[0]), bits(c.cost[:5, :7])), cid
        for k in ge.BUILDER_K:
            for limit in (None, np.sort(cost, axis=2)[:, :, 2], ge.TINIEST, ge.DBL_MAX, np.inf):
                if c.family == "boxes":
                    ell = boxes_to_ell(x, y, k, limit=limit, metric=ge.metric_of(c))
                else:
                    ell = points_to_ell(x, y, k, limit=limit, whiten=w)
                assert same_bytes(ell, bf.ell_by_sorting(cost, k, limit=limit)), (cid, k)


def test_the_augmented_and_the_list_routes_give_one_problem():
    """points_to_ell / boxes_to_ell with k = M and no limit hold the whole stack, and ell_to_packed(outside=) of those
    lists has the entries of dense_to_augmented on the definition's stack, bit for bit."""
    for family in ge.FAMILIES.values():
        for key, cases in ge.by_key(family()).items():
            x, y = np.stack([c.x for c in cases]), np.stack([c.y for c in cases])
            shapes, cost = ge.shapes_of(cases), ge.cost_stack(cases)
            MS = y.shape[1]
            if key[0] == "boxes":
                ell = boxes_to_ell(x, y, MS, shapes, metric=key[2])
            else:
                ell = points_to_ell(x, y, MS, shapes, whiten=None if cases[0].w is None else np.stack([c.w for c in cases]))
            outside = np.stack([ge.outside_rows(c) for c in cases])
            augs = dense_to_augmented(cost, shapes, outside=outside)
            packed = ell_to_packed(ell["cols"], ell["vals"], ell["rows"], outside=outside)
            for b, c in enumerate(cases):
                n, m = c.shape
                assert ell["rows"][b] == n and (ell["counts"][b, :n] == m).all(), ge.case_id(c)
                assert (ell["cols"][b, :n, :m] == np.arange(m)).all() and (ell["cols"][b, :n, m:] == -1).all()
                assert np.array_equal(bits(ell["vals"][b, :n, :m]), bits(c.cost)), ge.case_id(c)
                loc, val = packed[b]
                mat = np.full((n, m + n), -1.0)
                mat[loc[:, 0], loc[:, 1]] = val
                assert len(val) == n * m + n and np.array_equal(bits(mat), bits(augs[b])), ge.case_id(c)
