"""Shared by test_geometry_value_edges.py (GPU) and test_geometry_value_edges_nogpu.py: the coordinates that take the
three solve families which form their costs in the kernel -- the points batch, its whitened variant and the boxes batch
-- to the edges of the value range, with the oracle's result for each.  tests/_value_edges.py did this for the stored
stacks; nothing of it reaches the check passes of these families (k_points_batch_check, k_points_whiten_check,
k_boxes_batch_check), their cost chains or their candidate keys.

Every case is one problem of 40 x 56 (DENSE_SHAPE; the boxes also 9 x 13) without holes.  Its coordinates are seeded
draws of tests/_points_fixture.py / tests/_points_whiten.py / tests/_boxes_fixture.py scaled by a power of two, so the
scaling is exact; its cost stack is always the numpy definition (points_to_dense, boxes_to_dense) and the expected
result the oracle on that stack.  A stop is the max_iter given to BOTH sides, every one taken from
_value_edges.MAGNITUDES / EPS_STARTS; None only where the oracle ends on its own in fewer than 1000 rounds
(test_geometry_value_edges_nogpu.py holds every case to that).  The cases of one (family, type, D, metric, size,
eps_start, stop) travel in one batch.

Rounds of the oracle for the committed seeds, "min" / "max" ("cut" = stopped at its stop; printed by
test_every_oracle_solve_ends_within_its_stop of the nogpu module):

  points float64  above_flt_max, dbl_max, zeros, ties_2_52, eps_3e38, eps_1e39: cut for every D and both problems
                  c_is_zero        D = 1, 2: cut / cut; D = 8: 6 / 36 (distinct costs: a solve at eps == 0 can end)
                  c_subnormal_f32  D = 1: 5 / 23; D = 2: 5 / 9; D = 8: 2 / 4
                  c_subnormal_tie  28 / 35
                  ulp_2_53         D = 1: 132 / 240; D = 2: cut / cut; D = 8: 77 / cut
                  eps_1e-46        D = 1: 71 / 114; D = 2: 47 / 51; D = 8: 23 / 26
                  eps_1e-45        D = 1: 1267 / cut at 2000; D = 2: 248 / 694; D = 8: 6 / 36
  points float32  f32_subnormal_coords  D = 2: 120 / cut; D = 3: 27 / 185;   f32_big_coords: cut
  whitened        w_subnormal  D = 1: 6 / 20; D = 4: 3 / 5       w_split  D = 1: 157 / 212; D = 4: 91 / 94
                  w_above_flt_max, w_zero: cut
  boxes           `identical` is cut; every other case ends: 10 .. 72 rounds where the costs differ, 128 at 2^-537
                  (16 distinct costs, 40 x 56, "max"), 36 (9 x 13) and 360 (40 x 56) where every cost is 1.0 (2^-540 and
                  `disjoint` under "iou"), 30 .. 202 for `disjoint` under "giou"
"""
import collections
import functools
import zlib

import numpy as np

from sslap_amd import boxes_to_dense, points_to_dense
from tests import _value_edges as ve
from tests._batch_shapes import dense_expect
from tests._boxes_fixture import METRICS, draw_boxes
from tests._points_fixture import draw
from tests._points_whiten import draw_whiten
from tests.test_dense_outside import expect as outside_expect

N, M = ve.DENSE_SHAPE
SMALL = (9, 13)  # the second size of the boxes cases
PROBLEMS = ve.PROBLEMS
POINT_DIMS = (1, 2, 8)
F32_DIMS = (2, 3)  # (D = 1 has fewer than 1000 distinct costs: the coordinates are integers below 512 times 2^-149)
WHITEN_DIMS = (1, 4)
WHITEN_STACK = (N + 2, M + 3)  # the whitened cases lie in a larger stack: NaN beyond the shape, in W as well
BOX_SCALES = (-515, -525, -537, -540, 510)
STOP_OF = {name: stop for name, _, stop in ve.MAGNITUDES + ve.EPS_STARTS}

# What a stop is for, as in _value_edges.py.  NEVER_ENDS: C or eps is +inf or every cost is 0 -- no variant of the case
# ends, each is cut at its stop.  ENDS_LATE: the oracle ends on its own in every variant, but in more than 1000 rounds.
# No case here does: eps_1e-45, which is one on the stored stacks, ends in 6 .. 1267 rounds on these draws and is cut at
# 2000 for D = 1 under "max".  A case without a stop ends in fewer than 1000 rounds in every variant; every other stopped
# case is cut in some variants and ends below its stop in others.
NEVER_ENDS = ("above_flt_max", "dbl_max", "zeros", "eps_1e39", "f32_big_coords", "w_above_flt_max", "w_zero", "identical")
ENDS_LATE = ()

# family: "points", "whiten" or "boxes"; key: what one batched call shares (family, dtype, D or metric, stack shape);
# x, y: the point sets (boxes: a, b) of the stack's shape; w: the matrices or None; shape: (n, m) inside the stack;
# cost: the definition's (n, m) float64 costs; opts: the call's eps_start; stop: the max_iter of both sides.
Case = collections.namedtuple("Case", "name family key x y w shape cost opts stop")


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def _seed(*parts):
    return [95] + [zlib.crc32(str(p).encode()) for p in parts]


def _scaled(a, e):
    """a * 2^e, exactly (np.ldexp), in a's type."""
    return np.ldexp(a, e)


def metric_of(case):
    return case.key[2] if case.family == "boxes" else None


def cost_stack(case_or_cases):
    """The definition's float64 stack of one case or of a list of cases of one key: (B, N_stack, M_stack), +inf beyond
    the shapes."""
    cases = [case_or_cases] if isinstance(case_or_cases, Case) else list(case_or_cases)
    c0 = cases[0]
    x, y = np.stack([c.x for c in cases]), np.stack([c.y for c in cases])
    shapes = shapes_of(cases)
    if c0.family == "boxes":
        return boxes_to_dense(x, y, shapes, metric_of(c0))
    w = None if c0.w is None else np.stack([c.w for c in cases])
    return points_to_dense(x, y, shapes, whiten=w)


def shapes_of(cases):
    """None where every case fills its stack, else the int32 (B, 2) shapes."""
    if all(c.shape == (c.x.shape[0], c.y.shape[0]) for c in cases):
        return None
    return np.array([c.shape for c in cases], dtype=np.int32)


def _case(name, family, key, x, y, w=None, shape=None, opts=(), stop=None):
    shape = (x.shape[0], y.shape[0]) if shape is None else shape
    proto = Case(name, family, key, x, y, w, shape, None, tuple(sorted(dict(opts).items())), stop)
    with np.errstate(over="raise", invalid="raise"):
        cost = np.ascontiguousarray(cost_stack(proto)[0, :shape[0], :shape[1]])
    assert np.isfinite(cost).all() and not np.signbit(cost).any(), name
    return proto._replace(x=_frozen(x), y=_frozen(y), w=_frozen(w), cost=_frozen(cost))


def tie_points():
    """Integer points (x in 0 .. 3 x 0 .. 3, y in 4 .. 7 x 3 .. 5) whose largest difference is (7, 5), planted at
    (x_0, y_0): the largest cost is 49 + 25 = 74."""
    rng = np.random.default_rng(_seed("tie"))
    x = rng.integers(0, 4, (N, 2)).astype(np.float64)
    y = np.stack([rng.integers(4, 8, M), rng.integers(3, 6, M)], axis=1).astype(np.float64)
    x[0], y[0] = (0.0, 0.0), (7.0, 5.0)
    return x, y


@functools.lru_cache(maxsize=None)
def points_cases():
    """[Case]: the float64 magnitudes for D = 1, 2, 8, the eps_start cases on the plain draw, the two float32 cases."""
    out = []
    for D in POINT_DIMS:
        key = ("points", "float64", D, (N, M))
        rng = np.random.default_rng(_seed("points", D))
        xu, yu = draw("uniform", (N, D), "float64", rng), draw("uniform", (M, D), "float64", rng)
        xg, yg = draw("grid", (N, D), "float64", rng), draw("grid", (M, D), "float64", rng)
        one = draw("uniform", (1, D), "float64", rng)

        def add(name, x, y, opts=()):
            out.append(_case(name, "points", key, x, y, opts=opts, stop=STOP_OF[name]))

        add("above_flt_max", _scaled(xu, 66), _scaled(yu, 66))
        add("dbl_max", _scaled(xu, 510), _scaled(yu, 510))
        add("c_is_zero", _scaled(xu, -80), _scaled(yu, -80))
        add("zeros", np.repeat(one, N, axis=0), np.repeat(one, M, axis=0))
        add("c_subnormal_f32", _scaled(xu, -70), _scaled(yu, -70))
        if D == 2:
            xt, yt = tie_points()
            add("c_subnormal_tie", _scaled(xt, -76), _scaled(yt, -76))
        add("ulp_2_53", _scaled(xu, 26), _scaled(yu, 26))
        add("ties_2_52", _scaled(xg, 25), _scaled(yg, 25))
        for name, eps, _ in ve.EPS_STARTS:
            add(name, xu.copy(), yu.copy(), opts=dict(eps_start=eps))
    for D in F32_DIMS:
        key = ("points", "float32", D, (N, M))
        rng = np.random.default_rng(_seed("points32", D))
        xu, yu = draw("uniform", (N, D), "float64", rng), draw("uniform", (M, D), "float64", rng)
        out.append(_case("f32_subnormal_coords", "points", key, (xu * 2.0 ** -140).astype(np.float32),
                         (yu * 2.0 ** -140).astype(np.float32), stop=STOP_OF["c_is_zero"]))
        out.append(_case("f32_big_coords", "points", key, (xu * 2.0 ** 126).astype(np.float32),
                         (yu * 2.0 ** 126).astype(np.float32), stop=STOP_OF["above_flt_max"]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def whiten_cases():
    """[Case] for D = 1, 4: W = tril(uniform) (tests/_points_whiten.py: draw_whiten) with the magnitude in W, or split
    between W and the coordinates.  The upper triangles, and W, x and y beyond the 40 x 56 shape, hold NaN."""
    out = []
    NS, MS = WHITEN_STACK
    for D in WHITEN_DIMS:
        key = ("whiten", "float64", D, WHITEN_STACK)
        rng = np.random.default_rng(_seed("whiten", D))
        x, y = np.full((NS, D), np.nan), np.full((MS, D), np.nan)
        x[:N], y[:M] = draw("uniform", (N, D), "float64", rng), draw("uniform", (M, D), "float64", rng)
        w = draw_whiten("uniform", (NS, D, D), "float64", rng)
        w[N:] = np.nan
        zero = np.where(np.isnan(w), np.nan, 0.0)

        def add(name, x_, w_, like):
            out.append(_case(name, "whiten", key, x_[0], x_[1], w_, shape=(N, M), stop=STOP_OF[like]))

        add("w_subnormal", (x.copy(), y.copy()), _scaled(w, -70), "c_subnormal_f32")
        add("w_split", (_scaled(x, 500), _scaled(y, 500)), _scaled(w, -480), "c_subnormal_f32")
        add("w_above_flt_max", (x.copy(), y.copy()), _scaled(w, 66), "above_flt_max")
        add("w_zero", (x.copy(), y.copy()), zero, "zeros")
    return tuple(out)


def box_name(e):
    return f"scale_2^{e:+d}"


@functools.lru_cache(maxsize=None)
def box_base(size):
    """(a, b): draw_boxes("uniform") of `size` = (n, m), unscaled."""
    rng = np.random.default_rng(_seed("boxes", size))
    return _frozen(draw_boxes("uniform", (size[0], 4), "float64", rng), draw_boxes("uniform", (size[1], 4), "float64", rng))


@functools.lru_cache(maxsize=None)
def boxes_cases():
    """[Case]: float64 boxes of 9 x 13 and 40 x 56 for both metrics -- the draw scaled by 2^e, every box the same box,
    unit boxes far apart on a diagonal -- and one float32 case of 40 x 56 per metric with subnormal coordinates."""
    out = []
    for metric in METRICS:
        for size in (SMALL, (N, M)):
            n, m = size
            key = ("boxes", "float64", metric, size)
            a, b = box_base(size)
            for e in BOX_SCALES:
                out.append(_case(box_name(e), "boxes", key, _scaled(a, e), _scaled(b, e), stop=None))
            out.append(_case("identical", "boxes", key, np.repeat(a[:1], n, axis=0), np.repeat(a[:1], m, axis=0),
                             stop=STOP_OF["zeros"]))
            at = 10.0 * np.arange(max(n, m))[:, None]
            unit = np.concatenate([at, at, at + 1.0, at + 1.0], axis=1)
            out.append(_case("disjoint", "boxes", key, unit[:n].copy(), unit[:m] + 5.0, stop=None))
        a, b = box_base((N, M))
        out.append(_case("f32_subnormal_coords", "boxes", ("boxes", "float32", metric, (N, M)),
                         (a * 2.0 ** -140).astype(np.float32), (b * 2.0 ** -140).astype(np.float32), stop=None))
    return tuple(out)


FAMILIES = dict(points=points_cases, whiten=whiten_cases, boxes=boxes_cases)


def all_cases():
    return points_cases() + whiten_cases() + boxes_cases()


def case_id(case):
    return (case.name,) + case.key


def by_key(cases):
    """{key: [cases]}: what one builder call can take (the builder has no eps and no stop)."""
    out = {}
    for c in cases:
        out.setdefault(c.key, []).append(c)
    return out


def groups(cases):
    """Options are per call: [(key, opts, stop, [cases])], the cases of one (key, eps_start, stop) in one batch."""
    out = {}
    for c in cases:
        out.setdefault((c.key, c.opts, c.stop), []).append(c)
    return [(key, dict(opts), stop, cs) for (key, opts, stop), cs in out.items()]


def oracle_opts(opts, stop):
    o = dict(opts, cardinality_check=False)
    if stop is not None:
        o["max_iter"] = stop
    return o


@functools.lru_cache(maxsize=None)
def _want(index, problem):
    case = all_cases()[index]
    with np.errstate(over="ignore"):  # (eps_start = 1e39 narrows to +inf)
        return dense_expect(case.cost, problem, **oracle_opts(case.opts, case.stop))


def want(case, problem):
    """The oracle's result on the case's stack (computed once)."""
    return _want(all_cases().index(case), problem)


# ---- outside: per-row values at the case's own magnitude, one of them equal to a cost; -0.0 beside costs that are zero
# as a float32; and two problems whose outside value alone sets C
ZERO_OUTSIDE = ("c_is_zero", "zeros", "w_zero", "identical")
OUTSIDE_STOP = ve.OUTSIDE_STOP
OUTSIDE_OPTS = ve.OUTSIDE_OPTS
C_FROM_OUTSIDE = (("c_is_zero", 3.0), ("eps_1e-46", 2.0 ** 60))  # (eps_1e-46 is the plain draw: the eps_start narrows to 0)


def outside_stop(case):
    return OUTSIDE_STOP if case.stop is None else case.stop


def outside_rows(case, value=None):
    """The outside values of a case's rows, NaN beyond its shape; value: that value for every row instead."""
    n, m = case.shape
    o = np.full(case.x.shape[0], np.nan)
    if value is not None:
        o[:n] = value
    elif case.name in ZERO_OUTSIDE:
        o[:n] = -0.0
    else:
        rng = np.random.default_rng(_seed("outside", *case_id(case)))
        o[:n] = rng.uniform(case.cost.min(), case.cost.max(), n)
        o[0] = case.cost[0, rng.integers(0, m)]
    assert np.isfinite(o[:n]).all()
    return o


def outside_groups(cases):
    """[(key, opts, stop, [(case, outside row values)])]: every case with its own values, and behind them the cases of
    C_FROM_OUTSIDE (the D = 2 ones) with the value that alone sets C -- one batch per (key, eps_start, stop)."""
    out = {}
    for c in cases:
        entries = out.setdefault((c.key, c.opts, outside_stop(c)), [])
        entries.append((c, _frozen(outside_rows(c))))
    for c in cases:
        for name, value in C_FROM_OUTSIDE:
            if c.name == name and c.key == ("points", "float64", 2, (N, M)):
                out[(c.key, c.opts, outside_stop(c))].append((c, _frozen(outside_rows(c, value))))
    return [(key, dict(opts), stop, entries) for (key, opts, stop), entries in out.items()]


_OUTSIDE_WANT = {}


def outside_want(key, opts, stop, entries, problem):
    """[(want, m, n)] of an outside group: the oracle on dense_to_augmented of the definition's stack (computed once)."""
    ident = (key, tuple(sorted(opts.items())), stop, problem)
    if ident not in _OUTSIDE_WANT:
        cases = [c for c, _ in entries]
        with np.errstate(over="ignore"):
            _OUTSIDE_WANT[ident] = outside_expect(cost_stack(cases), shapes_of(cases), np.stack([o for _, o in entries]),
                                                  problem, max_iter=stop, **opts, **OUTSIDE_OPTS)
    return _OUTSIDE_WANT[ident]


def call_opts(opts, stop):
    """The keywords of a library call for a group (the plain points / boxes calls have no guard to switch off)."""
    kw = dict(opts)
    if stop is not None:
        kw["max_iter"] = stop
    return kw


# ---- the builder: the limits of one call on the cases of a key
DBL_MAX = ve.DBL_MAX
TINIEST = 5e-324  # the smallest subnormal double
BUILDER_K = (1, 8)


def limits(cases):
    """[None, the 3rd smallest cost of every row (exact equality at the case's magnitude), the smallest subnormal,
    DBL_MAX, +inf] for one builder call on `cases` (of one key)."""
    third = np.ascontiguousarray(np.sort(cost_stack(cases), axis=2)[:, :, 2])  # (+inf beyond a shape: no row there)
    return [None, third, TINIEST, DBL_MAX, np.inf]


def all_costs_tie(case):
    return len(np.unique(case.cost)) == 1
