"""Shared by test_matching_paths.py (GPU) and test_matching_paths_nogpu.py: the graphs that take k_matching_batch
(csrc/kernels_matching_batch.hpp) through the steps of its DFS that decide *which* maximum matching comes out -- the
64-lane neighbour scan, the resume position after a failed child, the dist_nil test, the explicit stack -- and, for each
graph and each adjacency source, what the model (_matching_model.py) gives on that source's stored order.

A case is a list of rows, each the columns the row stores, in stored order.  It is expressed three ways:
  loc    the packed (nnz, 2) array; an absent row is a gap
  dense  the slice of a stack, entry iff >= 0; stored position = column, so the stored order is ascending (cases with a
         repeated entry have no dense form)
  ell    (n, K) slots; the row's stored order is kept and up to ELL_HOLES holes sit at random slots between the
         entries, the rest after them, so stored positions shift relative to loc
Seeds and parameters are frozen here; the expectations are computed once per process.
"""
import collections
import functools
import zlib

import numpy as np

import _matching_model as model

Case = collections.namedtuple("Case", "name rows n m")


def _case(name, rows):
    rows = tuple(np.ascontiguousarray(r, dtype=np.int64) for r in rows)
    for r in rows:
        r.setflags(write=False)
    assert len(rows[-1]) > 0  # (a loc's n is its largest row + 1)
    return Case(name, rows, len(rows), int(max(int(r.max()) for r in rows if len(r))) + 1)


# ---- the families ---------------------------------------------------------------------------------------------------------
def hot_graph(seed, n, m, hot):
    """Every row stores a random permutation of the same `hot` columns, then up to 3 random columns, then, with
    probability 0.7, its own column of a hidden permutation, last (a column is never stored twice in a row).  The hot
    columns are matched early and fought over from then on: rows of ~hot + 4 entries whose qualifying entries sit at
    random positions, deep in the second chunk as often as in the first."""
    rng = np.random.default_rng([11, seed, n, m])
    hidden = rng.permutation(m)[:n]
    hotset = rng.permutation(m)[:hot]
    rows = []
    for i in range(n):
        r = list(rng.permutation(hotset))
        for c in rng.integers(0, m, 3):
            if c not in r:
                r.append(int(c))
        if rng.random() < 0.7 and hidden[i] not in r:
            r.append(int(hidden[i]))
        rows.append(r)
    if max(max(r) for r in rows) < m - 1:
        rows[-1].append(m - 1)  # (m is the largest column + 1 in every source)
    return rows


def gadget(p, q=None, alt=False):
    """The last row R has a qualifying entry at stored position p whose child fails, so R resumes at p + 1; its next
    qualifying entry sits at position q > p, and without q R has length p + 1 and is exhausted (g == g1 right after the
    hit) -- the graph is then short by one row.  With Q = q, or p + 1 without q, and a = Q + 1:
      rows c = 0 .. Q-1 but p  S_c = [c]      p    X = [p]      Q    Y = [Q, a]      Q+1  Y0 = [a+1, a+2]
      Q+2  F0 = [every c < Q but p, a+1]      Q+3  R = [0 .. q], or [0 .. p] without q
    Phase 1 matches S_c, X, Y, Y0 to their first column and leaves F0 and R free.  In phase 2 (dist_nil = 2) F0 enters
    every S_c, which fails (a hit, a failed child and a resume at every position of its row), then reaches the free column
    a + 2 through Y0; R skips the dead S_c chunk by chunk, enters X at position p, X fails, R resumes at p + 1 and goes
    on over dead S_c to position q, where Y leads to the free column a.  Every row is ascending, so the dense form
    has the same stored positions.
    With `alt` a row Y2 = [Q+1, a+1] follows Y (a = Q + 2, Y0 = [a+2, a+3]) and R also stores Q + 1, at position q + 1: a
    scan that misses position q still matches every row, but R to another column."""
    Q = p + 1 if q is None else q
    assert Q > p and not (alt and q is None)
    a = Q + 2 if alt else Q + 1
    ys = [[Q, a], [Q + 1, a + 1]] if alt else [[Q, a]]
    y0 = ys[-1][1] + 1
    r = list(range(p + 1 if q is None else q + 1)) + ([Q + 1] if alt else [])
    return [[c] for c in range(Q)] + ys + [[y0, y0 + 1], [c for c in range(Q) if c != p] + [y0], r]


DEEP_JUNK, DEEP_CHAIN, DEEP_DECOYS = 70, 205, tuple(range(10, 205, 10))


def deep_graph():
    """One augmenting path of depth DEEP_CHAIN through rows of 72 or 73 entries.
      rows 0 .. 69: junk row j = [j];  then one decoy row per i in DEEP_DECOYS = [70 + 2i + 1];
      then chain row i = [0 .. 69, 70 + 2i, (70 + 2i + 1 if i is a decoy's), 70 + 2(i + 1)];  last the root = [70].
    Phase 1 matches every row but the root to its first free column (chain i to 70 + 2i).  Phase 2 has one root and one
    path: root -> chain 0 -> chain 1 -> ... -> the free column 70 + 2 * DEEP_CHAIN.  Chain i sits at depth i + 1 and finds
    its child at stored position 71 or 72, behind the 70 junk entries (which qualify for chain 0 alone: 70 failed
    children in a row) and its own column; where it has a decoy the child behind position 71 fails first.  So the stack
    holds a resume position of 72 or 73 at every depth at once.  Rows ascending: dense has the same positions."""
    rows = [[j] for j in range(DEEP_JUNK)] + [[DEEP_JUNK + 2 * i + 1] for i in DEEP_DECOYS]
    for i in range(DEEP_CHAIN):
        r = list(range(DEEP_JUNK)) + [DEEP_JUNK + 2 * i]
        if i in DEEP_DECOYS:
            r.append(DEEP_JUNK + 2 * i + 1)
        rows.append(r + [DEEP_JUNK + 2 * (i + 1)])
    return rows + [[DEEP_JUNK]]


def bfs_graph(seed, n, m, lo, hi, total=None, present=1.0):
    """n rows of lo .. hi distinct random columns, stored in random order; with `present` < 1 that share of the rows is
    kept (the others are gaps) and with `total` entries are added one row at a time until the graph holds that many."""
    rng = np.random.default_rng([12, seed, n, m])
    keep = rng.random(n) < present
    keep[-1] = True
    rows = [list(rng.choice(m, int(rng.integers(lo, hi + 1)), replace=False)) if keep[i] else [] for i in range(n)]
    if total is not None:
        order = [i for i in rng.permutation(n) if keep[i]]
        k = 0
        while sum(map(len, rows)) < total:
            r = rows[order[k % len(order)]]
            r.append(int(rng.choice(np.setdiff1d(np.arange(m), r))))
            k += 1
        assert sum(map(len, rows)) == total
    if max(max(r) for r in rows if r) < m - 1:
        rows[-1][-1] = m - 1
    return rows


def planted_graph(seed, n, lo, hi):
    """bfs_graph(n x n) whose row i also stores, last, its column of a hidden permutation: every row can be matched."""
    rows = bfs_graph(seed, n, n, lo, hi)
    hidden = np.random.default_rng([15, seed, n]).permutation(n)
    return [r if hidden[i] in r else r + [int(hidden[i])] for i, r in enumerate(rows)]


def _with_duplicate(rows, u):
    """rows with the last entry of row u stored twice."""
    rows = [list(r) for r in rows]
    rows[u].append(rows[u][-1])
    return rows


HOT_160_SEEDS = (0, 1, 2, 3)
GADGET_P = (0, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 127, 128)
# (p, q): resume at p + 1, the next hit at q.  From 11 a chunk ends at 74: q = 74 is its lane 63, and the lower q put a
# hit there once the ELL form's holes have shifted it; 90 and 140 lie in the chunk after a skipped unaligned one, 140
# after a resume beyond 63
GADGET_SKIPS = tuple((10, q) for q in range(68, 75)) + ((10, 90), (70, 140))
POSITIONS = (0, 62, 63, 64, 65, 127, 128)  # the hit's stored positions that test_required_events asks for: both sides of a chunk edge
BFS_N = 300


@functools.lru_cache(maxsize=None)
def cases():
    out = [_case(f"hot160_s{s}", hot_graph(s, 160, 160, 100)) for s in HOT_160_SEEDS]
    out += [_case(f"hot{n}", hot_graph(0, n, n, (100 * n) // 160)) for n in (63, 64, 65, 129)]
    out.append(_case("hot129x193", hot_graph(0, 129, 193, 100)))
    for p in GADGET_P:
        out.append(_case(f"gadget{p}_later", gadget(p, p + 1)))
        out.append(_case(f"gadget{p}_end", gadget(p)))
    for p, q in GADGET_SKIPS:
        out.append(_case(f"gadget{p}_skip{q}", gadget(p, q)))
    out.append(_case("gadget10_skip74_alt", gadget(10, 74, alt=True)))
    out.append(_case("deep", deep_graph()))
    out.append(_case("bfs300", bfs_graph(0, BFS_N, BFS_N, 1, 6)))
    out.append(_case("planted300", planted_graph(2, BFS_N, 1, 4)))
    lane = bfs_graph(1, BFS_N, 280, 12, 16, total=16 * BFS_N, present=0.9)
    out.append(_case("bfs300_lane", lane))            # nnz == 16 n: the loc BFS expands one row per lane
    out.append(_case("bfs300_wave", _with_duplicate(lane, 150 if lane[150] else 151)))  # 16 n + 1: one per wavefront
    return {c.name: c for c in out}


def names(source="loc"):
    """The cases a source can express, in a fixed order."""
    out = []
    for name, c in cases().items():
        if source == "dense" and has_repeated_entry(c):
            continue
        if source == "ell" and name not in ELL_K:
            continue
        out.append(name)
    return out


def has_repeated_entry(case):
    return any(len(set(r.tolist())) < len(r) for r in case.rows)


# ---- the three sources ------------------------------------------------------------------------------------------------------
def loc_of(case):
    r = np.repeat(np.arange(case.n), [len(x) for x in case.rows])
    return np.ascontiguousarray(np.stack([r, np.concatenate(case.rows)], axis=1), dtype=np.int32)


def pack(locs):
    loc = np.ascontiguousarray(np.concatenate(locs).reshape(-1, 2), dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([x.shape[0] for x in locs])]).astype(np.int64)
    return loc, offsets


def pattern_of(case):
    pat = np.zeros((case.n, case.m), dtype=bool)
    for u, r in enumerate(case.rows):
        pat[u, r] = True
    return pat


ELL_HOLES = 6
ELL_SALT = 2  # chosen so that the gadgets' hits land on every position of POSITIONS that fits (test_required_events)
# K of the stack a case is solved in: 16 is the largest with one row per lane in the BFS, 17 the smallest with one per
# wavefront; the gadgets with p = 127 and 128 have rows longer than any K here and no ELL form
ELL_K = {"bfs300": (16, 17), "planted300": (16, 17), "hot63": (64,), "hot64": (64,), "gadget0_later": (64,), "gadget0_end": (64,),
         "gadget56_later": (64,), "gadget56_end": (64,), "hot65": (65,), "gadget57_later": (65,), "gadget57_end": (65,)}
ELL_K.update({f"gadget{p}_{k}": (110,) for p in range(58, 66) for k in ("later", "end")})
ELL_K.update({f"gadget{p}_skip{q}": (110,) for p, q in GADGET_SKIPS if q + 1 + ELL_HOLES <= 110})
ELL_K.update({name: (110,) for name in ("gadget10_skip74_alt", "hot129", "hot129x193", "deep") + tuple(f"hot160_s{s}" for s in HOT_160_SEEDS)})
ELL_KS = (16, 17, 64, 65, 110)


@functools.lru_cache(maxsize=None)
def ell_slots(name, K):
    """(n, K) int64 columns of a case, -1 = hole: the entries of a row in stored order at a random ascending choice of
    its first len + ELL_HOLES slots (at most K)."""
    case = cases()[name]
    rng = np.random.default_rng([13, K, zlib.crc32(name.encode()), ELL_SALT])  # (a case keeps its holes when others are added)
    out = np.full((case.n, K), -1, dtype=np.int64)
    for u, r in enumerate(case.rows):
        assert 1 <= len(r) <= K, (name, u, len(r))
        out[u, np.sort(rng.choice(min(K, len(r) + ELL_HOLES), len(r), replace=False))] = r
    out.setflags(write=False)
    return out


def source_rows(name, source, K=None):
    """(rows, n, m) as the model takes them: the stored slots of each row of that source."""
    case = cases()[name]
    if source == "loc":
        return case.rows, case.n, case.m
    if source == "dense":
        pat = pattern_of(case)
        return [np.where(pat[u], np.arange(case.m), -1) for u in range(case.n)], case.n, case.m
    assert source == "ell" and K in ELL_K[name]
    return list(ell_slots(name, K)), case.n, case.m


Expect = collections.namedtuple("Expect", "left right size n m events")


@functools.lru_cache(maxsize=None)
def expect(name, source, K=None, variant=None):
    rows, n, m = source_rows(name, source, K)
    left, right, size, ev = model.solve(rows, m, variant)
    left.setflags(write=False)
    right.setflags(write=False)
    return Expect(left, right, size, n, m, ev)


def instances(source):
    """[(name, K)] of every graph a source holds (K None but for ell)."""
    if source == "ell":
        return [(name, K) for name in names("ell") for K in ELL_K[name]]
    return [(name, None) for name in names(source)]


# ---- dense stacks -----------------------------------------------------------------------------------------------------------
DENSE_DTYPES = ("float64", "float32", "float16", "bfloat16")
DENSE_PAD = (3, 5)  # the stack is this much larger than the largest graph


@functools.lru_cache(maxsize=1)
def dense_stack64():
    """(float64 stack, shapes): graph b in [:n_b, :m_b]; an entry is 1.0, -0.0 or +inf, anything else -1.0 or NaN (all
    five are exact in the four element types); +inf everywhere outside the shapes, which a read there would take for an
    entry."""
    cs = [cases()[name] for name in names("dense")]
    N, M = max(c.n for c in cs) + DENSE_PAD[0], max(c.m for c in cs) + DENSE_PAD[1]
    mats = np.full((len(cs), N, M), np.inf)
    for b, c in enumerate(cs):
        i, j = np.indices((c.n, c.m))
        yes = np.array([1.0, -0.0, np.inf])[(3 * i + 5 * j + b) % 3]
        no = np.array([-1.0, np.nan])[(i + j + b) % 2]
        mats[b, :c.n, :c.m] = np.where(pattern_of(c), yes, no)
    shapes = np.array([[c.n, c.m] for c in cs], dtype=np.int32)
    mats.setflags(write=False)
    shapes.setflags(write=False)
    return mats, shapes


# ---- the guards: batches of feasible graphs and graphs short by one or two rows -------------------------------------------------
def uniform_values(shape, *seed):
    return np.random.default_rng([14, *seed]).uniform(0, 100, shape)


GUARD_DENSE = ("hot160_s0", "hot160_s1", "hot160_s2", "hot160_s3", "hot129", "hot129x193", "hot65", "gadget63_later",
               "gadget63_end", "gadget64_later", "gadget64_end", "gadget128_later", "gadget128_end")
GUARD_SPARSE = GUARD_DENSE + ("deep",)
GUARD_EIGHT = ("hot160_s0", "gadget63_later", "hot160_s1", "hot160_s2", "gadget64_end", "hot160_s3", "hot129x193",
               "gadget65_later")  # the 8 graphs the 256-problem sparse batch cycles through


def guard_dense_stack(names_, pad=(0, 0)):
    """(float64 stack, shapes) for the auction: uniform [0, 100) on the entries, -1 elsewhere within the shape, +inf
    outside it (which the value check would report if it were read)."""
    cs = [cases()[name] for name in names_]
    N, M = max(c.n for c in cs) + pad[0], max(c.m for c in cs) + pad[1]
    mats = np.full((len(cs), N, M), np.inf)
    for b, c in enumerate(cs):
        mats[b, :c.n, :c.m] = np.where(pattern_of(c), uniform_values((c.n, c.m), 1, b), -1.0)
    return mats, np.array([[c.n, c.m] for c in cs], dtype=np.int32)


def guard_sparse_batch(names_):
    """(loc, val, offsets) of the packed graphs with uniform [0, 100) values."""
    locs = [loc_of(cases()[name]) for name in names_]
    loc, offsets = pack(locs)
    return loc, uniform_values(loc.shape[0], 2, len(names_)), offsets


def guard_ell_stack(K, wide):
    """(cols, vals, rows, names) of the stack of every case solved at K; holes hold -1 (int32) or a large negative
    column (int64) and a NaN value, which is never interpreted."""
    ns = [name for name in names("ell") if K in ELL_K[name]]
    N = max(cases()[name].n for name in ns)
    cols = np.full((len(ns), N, K), -1, dtype=np.int64 if wide else np.int32)
    for b, name in enumerate(ns):
        cols[b, :cases()[name].n] = ell_slots(name, K)
    if wide:
        cols[cols < 0] = -(2**40) - 7
    vals = np.where(cols >= 0, uniform_values(cols.shape, 3, K), np.nan)
    return cols, vals, np.array([cases()[name].n for name in ns], dtype=np.int32), ns
