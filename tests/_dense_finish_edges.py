"""The edge cases of the reverse finish of the dense batch (k_dense_reverse_finish<T, Lay, Out> in
csrc/kernels_dense_batch.hpp) and what each of them claims, shared by test_dense_finish_edges.py (GPU) and
test_dense_finish_edges_nogpu.py.

A case is a dict: name, mats (B, N, M) float64 on the host (holes: -1, or NaN under entries="finite"), dtype (the
element type the GPU test converts it to -- every value of a case is exact in its type), view ("contiguous" or
"transposed": the same elements behind a row stride of 1), kw (the keywords of auction_solve_batch), claim (a function
(case, fwd, model, trace) that asserts the situation the case was built for) and in_range (whether structure and optimum
are asserted on the CPU: the case lies inside max(|a|, |p|) * 2**-52 < eps).

On the GPU the yardstick stays tests/_dense_finish.py: assert_is_the_model, bit for bit on the outputs of the same call
without the finish; the claim is then checked on the model's trace of the GPU's own forward outputs.  Without a GPU,
`twin` builds the forward state with the CPU oracle (the GPU's forward solve, bit for bit, is pinned to it elsewhere),
runs the model with trace= and checks the same claim: a case whose situation does not occur fails on both sides.
"""
import functools

import numpy as np

from oracle import oracle as orc
from sslap_amd import dense_reverse_finish
from tests import _dense_finish as df
from tests import _value_edges as ve

TYPES = ("float64", "float32", "float16", "bfloat16")
FINISH_BUDGET = 5000  # max_iter of every values case: even a kernel without the stall rule ends after 5 000 iterations


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def _holes(rng, shape, share):
    """A mask of holes over (B, n, m) that keeps a random injection of the rows per problem."""
    B, n, m = shape
    gated = rng.random(shape) < share
    for b in range(B):
        gated[b, np.arange(n), rng.permutation(m)[:n]] = False
    return gated


# ---- the forward state of a case by the CPU oracle, and the model on it ------------------------------------------------
def _forward_one(mat, problem, outside, entries, p0, fast):
    """The reference's solve of one n x m problem (with outside: of its augmented form, the outside entry last in its
    row) from prices p0 over the real objects: (p (mo,), p2o (n,), eps32).  A column the reference never sees (behind
    its last column with an entry) keeps its starting price, as on the GPU."""
    n, m = mat.shape
    v = np.asarray(mat, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(v) if entries == "finite" else v >= 0
    p = np.zeros(m if outside is None else m + n)
    if p0 is not None:
        p[:m] = p0[:m]
    if outside is not None:
        d = np.zeros((n, n))
        d[np.arange(n), np.arange(n)] = outside
        v, valid = np.hstack([v, d]), np.hstack([valid, np.eye(n, dtype=bool)])
    ii, jj = np.nonzero(valid)
    loc = np.ascontiguousarray(np.stack([ii, jj], axis=1).astype(np.int32))
    o = orc.from_sparse(loc, np.ascontiguousarray(v[ii, jj]), problem=problem, fast=fast, size=(v.shape[1], n),
                        cardinality_check=False)
    np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))[:] = p[:o.M]
    p2o = o.solve().astype(np.int64)
    st = o.state()
    assert o.meta["n_assigned"] == n
    p[:o.M] = st["p"]
    return p, p2o, np.float32(st["eps"]), int(o.meta["its"])


def forward(case):
    """The forward outputs of a case as the GPU call without the finish gives them: dict(sol (B, N) int32, prices
    (B, M), [outside_prices (B, N)], final_eps (B,) float32, its (B,), shapes (B, 2))."""
    mats, kw = case["mats"], case["kw"]
    B, N, M = mats.shape
    shapes = np.tile([N, M], (B, 1)) if kw.get("shapes") is None else np.asarray(kw["shapes"])
    out = kw.get("outside")
    sol, prices = np.full((B, N), -1, dtype=np.int32), np.zeros((B, M))
    oprices, eps, its = np.zeros((B, N)), np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.int64)
    for b in range(B):
        n, m = (int(x) for x in shapes[b])
        p0 = None if kw.get("prices") is None else kw["prices"][b]
        p, p2o, eps[b], its[b] = _forward_one(mats[b, :n, :m], kw.get("problem", "min"), None if out is None else out[b, :n],
                                              kw.get("entries", "nonneg"), p0, kw.get("fast", False))
        sol[b, :n] = np.where(p2o < m, p2o, -1)
        prices[b, :m] = p[:m]
        if out is not None:
            oprices[b, :n] = p[m:]
    fwd = dict(sol=sol, prices=prices, final_eps=eps, its=its, shapes=shapes)
    if out is not None:
        fwd["outside_prices"] = oprices
    return fwd


def model(case, fwd, mats=None, shapes="case"):
    """(model result, trace) of the finish on the forward outputs fwd."""
    kw = case["kw"]
    trace = []
    res = dense_reverse_finish(case["mats"] if mats is None else mats, fwd["sol"], fwd["prices"], fwd["final_eps"],
                               problem=kw.get("problem", "min"), shapes=kw.get("shapes") if shapes == "case" else shapes,
                               outside=kw.get("outside"), outside_prices=fwd.get("outside_prices"),
                               entries=kw.get("entries", "nonneg"), max_iter=kw.get("max_iter", 1000000), trace=trace)
    return res, trace


def twin(case):
    """The CPU twin of a case: the oracle's forward state, the model with its trace, the case's claim.  Returns
    (fwd, model, trace)."""
    fwd = forward(case)
    res, trace = model(case, fwd)
    assert res["ran"].all()
    case["claim"](case, fwd, res, trace)
    return fwd, res, trace


def augmented(case, fwd_or_model, b):
    """(a, valid, p, p2o) of problem b in the model's terms, from a dict that holds sol, prices, [outside_prices]."""
    kw = case["kw"]
    shapes = np.tile(case["mats"].shape[1:], (case["mats"].shape[0], 1)) if kw.get("shapes") is None else np.asarray(kw["shapes"])
    n, m = (int(x) for x in shapes[b])
    out = kw.get("outside")
    a, valid = df.maximised(case["mats"][b, :n, :m], kw.get("problem", "min"), None if out is None else out[b, :n],
                            kw.get("entries", "nonneg"))
    p = fwd_or_model["prices"][b, :m]
    if out is not None:
        p = np.concatenate([p, fwd_or_model["outside_prices"][b, :n]])
    return a, valid, np.array(p), df.augmented_p2o(fwd_or_model["sol"][b, :n], m)


def assert_in_range_properties(case, fwd, res):
    """Structure and optimum of every problem of a case inside the documented range: df.assert_structure with its slack
    scaled by max |a| (the slack is stated for values below 1e4), and scipy's optimum within n * eps."""
    for b in range(case["mats"].shape[0]):
        a, valid, p0, p2o0 = augmented(case, fwd, b)
        _, _, q, q2o = augmented(case, res, b)
        n = a.shape[0]
        eps = float(fwd["final_eps"][b])
        big = float(np.abs(a[valid]).max())
        slack = 1e-9 * max(1.0, big / 1e4)
        assert big * 2.0 ** -52 < eps and res["reverse"]["left"][b] == 0
        finite = np.isfinite(q)  # (a single-entry row's object is priced +inf and stays where it is)
        df.assert_structure(a, valid, np.where(finite, q, 1e300), q2o, eps, p0[p2o0].min(), slack)
        got, best = a[np.arange(n), q2o].sum(), df.optimum(a, valid)
        assert best - n * eps - slack <= got <= best + slack, (case["name"], b, got, best)


def _moves(trace, b):
    return [t[1:] for t in trace if t[0] == b]


def _claim_work(case, fwd, res, trace):
    assert (res["reverse"]["its"] > 0).all(), res["reverse"]["its"]


# ---- A. every instance: {4 types} x {nonneg, finite} x {no outside, outside} -------------------------------------------------
A_SHAPE = (3, 70, 90)  # two rows per lane in the column scan, the second one partial
A_PARAMS = [(t, e, o, v) for t in TYPES for e in ("nonneg", "finite") for o in (False, True)
            for v in ("contiguous", "transposed")]


@functools.lru_cache(maxsize=None)
def _a_data(entries, out):
    rng = np.random.default_rng([1, entries == "finite", out])
    B, n, m = A_SHAPE
    lo, hi = (0, 200) if entries == "nonneg" else (-128, 128)  # (integers: exact in every type)
    v = rng.integers(lo, hi, A_SHAPE).astype(np.float64)
    mats = np.where(_holes(rng, A_SHAPE, 0.3), -1.0 if entries == "nonneg" else np.nan, v)
    prices = rng.uniform(0, 300, (B, m))
    outside = rng.integers(lo, hi, (B, n)).astype(np.float64) if out else None
    return _frozen(mats), _frozen(prices), outside


def instance_case(dtype, entries, out, view, problem):
    mats, prices, outside = _a_data(entries, out)
    kw = dict(problem=problem, fast=True, prices=prices, entries=entries)
    if out:
        kw["outside"] = outside
    return dict(name=f"A-{dtype}-{entries}-{'outside' if out else 'plain'}-{view}-{problem}", mats=mats, dtype=dtype,
                view=view, kw=kw, claim=_claim_work, in_range=True)


# ---- B. the top-two reduction ---------------------------------------------------------------------------------------------
# problem="max", fast: n rows, n + 1 objects, mat[i][i] = 10, every other real entry 0, object n a hole except on the
# rows of S (30), priced 100.  Every row bids 10 + eps for its own object by the same operations, so the profits are
# bit-equal and the rows of S tie exactly: one iteration, i* = min S, p[n] = beta - eps (omega == beta).
B_LANE = 77  # (lane 13, second row of its lane; 77 ^ off < 130 for every butterfly step)
B_SETS = {
    130: [(5, 70), (3, 67), (3, 67, 129), (8, 40)] + [(B_LANE, B_LANE ^ off) for off in (1, 2, 4, 8, 16, 32)]
         + [(128, 129, 1), (0,), (129,)],
    65: [(0, 64), (0,), (64,)],
    257: [(1, 192, 256), (0,), (256,)],
}
B_NEAR = ("tie", "larger_row_one_ulp_up", "smaller_row_one_ulp_down")


def _claim_reduction(case, fwd, res, trace):
    for b, (S, near) in enumerate(case["sets"]):
        n = case["mats"].shape[1]
        eps = float(fwd["final_eps"][b])
        p0 = fwd["prices"][b]
        assert fwd["sol"][b].tolist() == list(range(n)) and p0[n] == 100.0
        pi = 10.0 - p0[:n]
        assert len(set(pi.tolist())) == 1  # the profits are bit-equal
        lam = p0[:n].min()
        w = np.sort(case["mats"][b, list(S), n] - pi[list(S)])[::-1]
        if near == "tie":
            winner, beta, omega = min(S), w[0], (w[1] if len(S) > 1 else -np.inf)
            assert len(set(w.tolist())) == 1
        else:
            winner, beta, omega = max(S), w[0], w[1]
            assert len(S) == 2 and beta > omega  # the two w differ
        want = max(lam, omega - eps)
        assert _moves(trace, b) == [(n, winner, winner, False)], (S, near, _moves(trace, b))
        assert res["prices"][b, n] == want and (len(S) > 1) == (want > lam)
        assert res["sol"][b, winner] == n and res["reverse"]["its"][b] == 1 and res["reverse"]["left"][b] == 0


def reduction_case(n):
    sets = [(S, "tie") for S in B_SETS[n]]
    if n == 130:
        sets += [((5, 70), "larger_row_one_ulp_up"), ((5, 70), "smaller_row_one_ulp_down")]
    mats = np.zeros((len(sets), n, n + 1))
    mats[:, np.arange(n), np.arange(n)] = 10.0
    mats[:, :, n] = -1.0
    for b, (S, near) in enumerate(sets):
        mats[b, list(S), n] = 30.0
        if near == "larger_row_one_ulp_up":
            mats[b, max(S), n] = np.nextafter(30.0, np.inf)
        elif near == "smaller_row_one_ulp_down":
            mats[b, min(S), n] = np.nextafter(30.0, -np.inf)
    prices = np.zeros((len(sets), n + 1))
    prices[:, n] = 100.0
    return dict(name=f"B-{n}", mats=_frozen(mats), dtype="float64", view="contiguous", sets=sets,
                kw=dict(problem="max", fast=True, prices=_frozen(prices)), claim=_claim_reduction, in_range=True)


# ---- C. rows per lane and cropped shapes -----------------------------------------------------------------------------------
C_STACK = (130, 150)
C_ROWS = (1, 63, 64, 65, 127, 128, 129, 130)
C_EXTRA = 13  # m = n + 13 < 150
C_SQUARE = (255, 256, 257)


def _claim_cropped(case, fwd, res, trace):
    """The finish has work on every problem; the part of the stack outside the crop has no influence (holes there give
    the same result); and it would matter if it were read: the solve of the uncropped stack ends elsewhere."""
    _claim_work(case, fwd, res, trace)
    mats, shapes = case["mats"], np.asarray(case["kw"]["shapes"])
    inside = np.zeros(mats.shape, dtype=bool)
    for b, (n, m) in enumerate(shapes):
        inside[b, :n, :m] = True
    blank, _ = model(case, fwd, mats=np.where(inside, mats, -1.0))
    for key in ("sol", "prices", "outside_prices"):
        if key in res:
            assert blank[key].tobytes() == res[key].tobytes(), key
    whole = dict(case, kw={k: v for k, v in case["kw"].items() if k != "shapes"})
    wres, _ = model(whole, forward(whole))
    for b, (n, m) in enumerate(shapes):
        assert not (np.array_equal(wres["sol"][b, :n], res["sol"][b, :n])
                    and np.array_equal(wres["prices"][b, :m], res["prices"][b, :m])), b


def cropped_case(out):
    rng = np.random.default_rng([3, out])
    N, M = C_STACK
    B = len(C_ROWS)
    mats = rng.uniform(0, 100, (B, N, M))  # (doubles: integer ties make the finish with outside very long)
    shapes = np.array([[n, n + C_EXTRA] for n in C_ROWS], dtype=np.int32)
    for b, (n, m) in enumerate(shapes):  # outside the crop: large attractive entries (problem="max")
        mats[b, n:, :] = rng.uniform(5000, 6000, (N - n, M))
        mats[b, :, m:] = rng.uniform(5000, 6000, (N, M - m))
    kw = dict(problem="max", fast=True, shapes=_frozen(shapes), prices=_frozen(rng.uniform(0, 150, (B, M))))
    if out:
        kw["outside"] = _frozen(rng.uniform(70, 90, (B, N)))
    return dict(name=f"C-cropped-{'outside' if out else 'plain'}", mats=_frozen(mats), dtype="float64", view="contiguous",
                kw=kw, claim=_claim_cropped, in_range=True)


def square_case(n):
    """A square stack has nothing to do without outside; with it, from high prices, many rows start on their outside
    option and the real objects they left are taken up again."""
    rng = np.random.default_rng([4, n])
    mats = np.where(_holes(rng, (1, n, n), 0.5), -1.0, rng.integers(0, 100, (1, n, n)).astype(np.float64))
    kw = dict(problem="max", fast=True, prices=_frozen(rng.uniform(0, 40, (1, n))),
              outside=_frozen(rng.integers(40, 60, (1, n)).astype(np.float64)))
    return dict(name=f"C-square-{n}", mats=_frozen(mats), dtype="float64", view="contiguous", kw=kw, claim=_claim_work,
                in_range=True)


# ---- D. the open-object scan ----------------------------------------------------------------------------------------------
D_SHAPE = (70, 200)
D_EMPTY = (0, 62, 63, 64, 65, 127, 128, 199)


def _claim_scan(case, fwd, res, trace):
    # problem 0: exactly the empty columns, ascending, each dropping to lambda without a row
    assert _moves(trace, 0) == [(j, -1, -1, False) for j in D_EMPTY], _moves(trace, 0)
    # problem 1: the first (and only) hit is three blocks of 64 behind the cursor
    assert _moves(trace, 1) == [(199, -1, -1, False)]
    # problem 2: column 64 has entries: a row moves there and a chain follows from the object it left
    t = _moves(trace, 2)
    k = next(k for k, x in enumerate(t) if x[0] == 64)
    assert [x[0] for x in t[:k]] == [0, 62, 63] and t[k][1] >= 0 and not t[k][3]
    assert t[k + 1][3] and t[k + 1][0] == t[k][2]
    rest = [x[0] for x in t if not x[3]]  # the scan's own picks: ascending, and the other empty columns among them
    assert rest == sorted(rest) and set(D_EMPTY) <= set(rest)
    assert (res["reverse"]["left"] == 0).all()


def scan_case():
    """Every row prefers a column of its own by a wide margin, so the forward solve is one round without contention
    and leaves no abandoned object: the open objects are exactly the columns priced through prices=."""
    rng = np.random.default_rng([5])
    n, m = D_SHAPE
    mats = np.empty((3, n, m))
    prices = np.zeros((3, m))
    for b, empty in enumerate((D_EMPTY, (199,), tuple(j for j in D_EMPTY if j != 64))):
        v = rng.integers(0, 10, (n, m)).astype(np.float64)
        own = rng.permutation(np.setdiff1d(np.arange(m), D_EMPTY))[:n]
        v[np.arange(n), own] = 50.0 + rng.integers(0, 10, n)
        v[:, list(empty)] = -1.0
        if b == 2:
            v[:, 64] = 200.0 + rng.integers(0, 10, n)
        mats[b] = v
        prices[b, list(D_EMPTY if b != 1 else (199,))] = 500.0
    return dict(name="D-scan", mats=_frozen(mats), dtype="float64", view="contiguous",
                kw=dict(problem="max", fast=True, prices=_frozen(prices)), claim=_claim_scan, in_range=True)


# ---- E. outside objects in the loop ---------------------------------------------------------------------------------------
E_SHAPE = (4, 70, 90)


def outside_outcomes(case, trace):
    """Per problem the set of outcomes of a chained outside object whose row is not on lane 0: "back" (the row takes it
    back) and "drop" (it falls to lambda)."""
    m = case["mats"].shape[2]
    seen = [set() for _ in range(case["mats"].shape[0])]
    for b, j, i, _, chained in trace:
        if chained and j >= m and (j - m) % 64 != 0:
            assert i in (-1, j - m)
            seen[b].add("back" if i == j - m else "drop")
    return seen


def _claim_outside_loop(case, fwd, res, trace):
    seen = set().union(*outside_outcomes(case, trace))
    assert seen == {"back", "drop"}, seen
    assert (res["reverse"]["left"] == 0).all()


def outside_loop_case(seed=0):
    """A forward solve never leaves an outside object open, so j >= m is reached only as the object a moving row has
    just left.  Outside values near the rows' best net values make rows leave their outside object and come back."""
    rng = np.random.default_rng([6, seed])
    B, n, m = E_SHAPE
    mats = np.where(_holes(rng, E_SHAPE, 0.3), -1.0, rng.integers(0, 100, E_SHAPE).astype(np.float64))
    kw = dict(problem="max", fast=True, prices=_frozen(rng.uniform(0, 120, (B, m))),
              outside=_frozen(rng.integers(0, 60, (B, n)).astype(np.float64)))
    return dict(name="E-outside-loop", mats=_frozen(mats), dtype="float64", view="contiguous", kw=kw,
                claim=_claim_outside_loop, in_range=True)


# ---- F. values -------------------------------------------------------------------------------------------------------------
# the (40, 56) matrix with 30 % holes of tests/_value_edges.py, prices P, fast (eps = float32(1 / 40)).  name ->
# (values of u, prices of P, problem, in range, expected (its, left, eCE) of the model with the stall rule)
F_PRICES = np.random.default_rng(3).uniform(0, 150, 56)
F_TABLE = {
    "2_47-max": (lambda u: np.floor(u * 2.0 ** 47), lambda p: np.floor(p * 2.0 ** 47), "max", (201, 13, 16, 1)),
    "2_47-min": (lambda u: np.floor(u * 2.0 ** 47), lambda p: np.floor(p * 2.0 ** 47), "min", (97, 37, 15, 0)),
    "2_1000-min": (lambda u: u * 2.0 ** 1000, lambda p: p * 2.0 ** 1000, "min", (97, 83, 15, 1)),
    "2_1000-max": (lambda u: u * 2.0 ** 1000, lambda p: p * 2.0 ** 1000, "max", (201, 13, 16, 1)),
    "8e307-min": (lambda u: u / 100 * 8e307, lambda p: p / 150 * 8e307, "min", (43, 65, 16, 0)),
    "8e307-max": (lambda u: u / 100 * 8e307, lambda p: p / 150 * 8e307, "max", (102, 9, 16, 1)),
}
F_NAMES = tuple(F_TABLE) + ("small_ints", "single_entry_rows", "single_entry_rows-outside", "signed_zeros",
                            "float32_flt_max_4", "float16_65504")


def _claim_stall(case, fwd, res, trace):
    """The pinned figures (forward rounds, its, left, eCE), and the last iteration is the stalled one: a row was found,
    nothing moved."""
    rounds, its, left, ece = case["figures"]
    got = (int(fwd["its"][0]), int(res["reverse"]["its"][0]), int(res["reverse"]["left"][0]), int(res["eCE"][0]))
    assert got == (rounds, its, left, ece), got
    assert rounds <= 201 and its < FINISH_BUDGET and trace[-1][2] >= 0 and trace[-1][3] == -1, trace[-1]


def _claim_small_ints(case, fwd, res, trace):
    assert fwd["its"][0] < FINISH_BUDGET and res["reverse"]["its"][0] > 0 and res["reverse"]["left"][0] == 0
    assert all(not (i >= 0 and freed == -1) for _, _, i, freed, _ in trace)  # no stall inside the range
    a, valid, p, p2o = augmented(case, fwd, 0)
    pi = a[np.arange(a.shape[0]), p2o] - p[p2o]
    assert len(set(pi.tolist())) < a.shape[0]  # rows with bit-equal profits: candidates for exact ties


def _claim_inf_prices(case, fwd, res, trace):
    p = fwd["outside_prices"] if "outside" in case["kw"] else fwd["prices"]
    assert np.isposinf(p).sum() == 2 and (res["reverse"]["its"] > 0).all() and (res["reverse"]["left"] == 0).all()
    q = res["outside_prices"] if "outside" in case["kw"] else res["prices"]
    assert np.isposinf(q).sum() == 2


def _claim_zeros(case, fwd, res, trace):
    v = case["mats"]
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any()
    _claim_work(case, fwd, res, trace)


def _claim_out_of_range(case, fwd, res, trace):
    """eps is below one ulp of the values: the finish ends, by the stall rule or without one, far below the budget."""
    big = float(np.nanmax(np.abs(case["mats"])))
    assert big * 2.0 ** -52 > float(fwd["final_eps"][0])
    assert 0 < res["reverse"]["its"][0] < FINISH_BUDGET and fwd["its"][0] < FINISH_BUDGET


def value_case(name):
    u, valid, _ = ve.dense_base()
    rng = np.random.default_rng([7, F_NAMES.index(name)])
    kw = dict(problem="max", fast=True, prices=F_PRICES[None].copy(), max_iter=FINISH_BUDGET)
    case = dict(name="F-" + name, dtype="float64", view="contiguous", in_range=False)

    def on_u(vals, hole=-1.0):
        mat = np.full(u.shape, hole)
        mat[valid] = vals
        return mat[None]

    if name in F_TABLE:
        fv, fp, problem, figures = F_TABLE[name]
        kw.update(problem=problem, prices=fp(F_PRICES)[None])
        case.update(mats=on_u(fv(u[valid])), claim=_claim_stall, figures=figures)
    elif name == "small_ints":  # values 0 .. 4: many ties
        kw.update(problem="min")
        case.update(mats=on_u(np.floor(u[valid] / 20)), claim=_claim_small_ints, in_range=True)
    elif name.startswith("single_entry_rows"):
        mat = on_u(np.floor(u[valid]))
        out = name.endswith("outside")
        mat[0, [7, 29], :] = -1.0  # with outside the outside value is the one entry of these rows
        if out:
            kw.update(outside=np.floor(rng.uniform(20, 70, (1, u.shape[0]))))
        else:
            mat[0, 7, 11], mat[0, 29, 40] = 60.0, 3.0
        case.update(mats=mat, claim=_claim_inf_prices, in_range=True)
    elif name == "signed_zeros":  # min under finite: v * -1.0 turns 0.0 into -0.0 and back
        vals = np.floor(u[valid] / 10) - 5.0
        zero = vals == 0
        vals[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)
        vals[rng.random(vals.shape) < 0.25] = 0.0
        vals[rng.random(vals.shape) < 0.15] = -0.0
        kw.update(problem="min", entries="finite", prices=(F_PRICES / 10)[None])
        case.update(mats=on_u(vals, hole=np.nan), claim=_claim_zeros, in_range=True)
    elif name == "float32_flt_max_4":
        top = float(np.finfo(np.float32).max) / 4
        vals = (u[valid] / u[valid].max() * top).astype(np.float32).astype(np.float64)
        kw.update(prices=(F_PRICES / 150 * top)[None])
        case.update(mats=on_u(vals), dtype="float32", claim=_claim_out_of_range)
        assert vals.max() == top
    elif name == "float16_65504":
        vals = (u[valid] / u[valid].max() * 65504.0).astype(np.float16).astype(np.float64)
        kw.update(prices=(F_PRICES / 150 * 65504.0)[None])
        case.update(mats=on_u(vals), dtype="float16", claim=_claim_work, in_range=True)
        assert vals.max() == 65504.0
    else:
        raise KeyError(name)
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    case["mats"].setflags(write=False)
    case["kw"] = kw
    return case


# ---- every case outside section A, by name -------------------------------------------------------------------------------
def named_cases():
    out = {}
    for n in B_SETS:
        out[f"B-{n}"] = functools.partial(reduction_case, n)
    for o in (False, True):
        out[f"C-cropped-{'outside' if o else 'plain'}"] = functools.partial(cropped_case, o)
    for n in C_SQUARE:
        out[f"C-square-{n}"] = functools.partial(square_case, n)
    out["D-scan"] = scan_case
    out["E-outside-loop"] = outside_loop_case
    for name in F_NAMES:
        out["F-" + name] = functools.partial(value_case, name)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    c = named_cases()[name]()
    assert c["name"] == name
    return c
