"""A plain Python statement of the batched matcher (csrc/kernels_matching_batch.hpp), written from that kernel's header
comment and from csrc/host_matching.hpp, for tests/_matching_shapes.py and the two test_matching_paths modules.

A graph is given as it is stored: `rows[u]` is the sequence of the stored slots of row u, each a column or a negative
number for a hole, and `m` is the number of columns.  A packed loc has no holes; a dense row is its m columns with a hole
wherever the entry is invalid; an ELL row is its K slots.

  BFS  layer by layer from the free rows.  A row is labelled L + 1 by the first layer L that reaches it.  After the layer
       in which a free column is first seen the search stops with dist_nil = L + 1; the rows that layer labelled keep
       that label and are not expanded.
  DFS  from every row free at the start of the phase, in ascending order (the kernel takes them in chunks of 64 rows), on
       an explicit stack of (row, resume position).  The stored slots of a row are scanned in chunks of 64 from the
       current resume position g: the lowest qualifying slot g + k of the chunk wins and g becomes g + k + 1, a chunk
       without a hit advances g by 64.  A slot qualifies when it is no hole and Dist[Pair_V[v]] == depth + 1, a free v
       reading dist_nil.  After a child fails (its Dist becomes inf) the parent goes on from its saved g, so its chunks
       start unaligned from then on.

`solve` returns the pairings and an event log of what the DFS and the BFS did, so that the tests can require the inputs
to reach the steps they are meant to reach.  `variant=` names one deliberately wrong version of one step (VARIANTS); they
exist only here, to show that the cases tell the right algorithm from each of them.
"""
import collections

import numpy as np

INF = 2**31 - 1
WAVE = 64

VARIANTS = {
    "a": "the highest qualifying lane of a chunk wins instead of the lowest",
    "b": "after a child fails the parent resumes at the next multiple of 64: the rest of the chunk is lost",
    "c": "a chunk that starts unaligned stops at the next multiple of 64 but still advances by 64",
    "d": "a free column qualifies at depth + 1 instead of dist_nil",
    "e": "the rows labelled dist_nil are expanded one more layer before the BFS stops, and dist_nil is taken there",
    "f": "the last partial 64-row chunk of DFS roots is dropped",
    "g": "a hole does not occupy a stored position: the write-back of a path reads st_g - 1 of the compacted row",
}
# The extra layer of (e) alone -- its rows are labelled, dist_nil stays -- cannot change a result: a row
# labelled above dist_nil is only ever entered from a row at depth dist_nil, whose subtree has no free column in reach
# (a free column reads dist_nil) and fails either way.  "e_labels" is that form, kept to show it (the nogpu module asserts
# that it changes nothing); "e" also takes dist_nil from the layer where the search stops, as a loop that breaks one
# layer late would.
INVISIBLE_VARIANTS = {"e_labels": "as (e), but dist_nil keeps its value"}

Hit = collections.namedtuple("Hit", "row_len pos lane aligned depth")
# resume: the parent's stored position after the failed child's entry; later_chunk: 0 = the chunk that starts at
# `resume`, 1 = the one after it, ...; -1 without a later hit
Fail = collections.namedtuple("Fail", "row_len resume later_hit later_chunk depth")


class Events:
    def __init__(self):
        self.phases = 0            # phases with a DFS (a finite dist_nil)
        self.layers = []           # BFS layers expanded, per BFS (the last BFS, which finds nothing, included)
        self.largest_layer = 0     # rows of the largest expanded layer
        self.nil_rows = 0          # rows left labelled dist_nil and unexpanded, all phases
        self.max_depth = 0
        self.hits = []
        self.fails = []
        self.skipped = 0           # chunks without a hit
        self.skipped_unaligned = 0  # ... that started off a multiple of 64 (so: after a resume)
        self.root_chunks = set()   # (index of the 64-row chunk, whether it is a last partial one) of every DFS root
        self.augmented = 0

    def counts(self):
        f = self.fails
        return dict(phases=self.phases, layers=max(self.layers), largest_layer=self.largest_layer,
                    nil_rows=self.nil_rows, max_depth=self.max_depth, hits=len(self.hits), fails=len(f),
                    resumes_beyond_63=sum(x.resume > 63 for x in f),
                    later_chunk_hits=sum(x.later_hit and x.later_chunk > 0 for x in f),
                    skipped=self.skipped, skipped_unaligned=self.skipped_unaligned)


def solve(rows, m, variant=None):
    """(left, right, size, events) of the graph `rows` (stored slots per row, negative = hole) with m columns."""
    assert variant is None or variant in VARIANTS or variant in INVISIBLE_VARIANTS, variant
    n = len(rows)
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
    packed = [r[r >= 0] for r in rows]
    pair_u = np.full(n, -1, dtype=np.int64)
    pair_v = np.full(m, -1, dtype=np.int64)
    dist = np.zeros(n, dtype=np.int64)
    st_u, st_g = [0] * (n + 1), [0] * (n + 1)
    ev = Events()

    for phase in range(n + 2):  # (the kernel's own bound; a right algorithm ends long before it)
        # ---- BFS
        free = np.flatnonzero(pair_u == -1)
        dist[:] = INF
        dist[free] = 0
        layer, nil, L = free, INF, 0
        extra = False  # variants e / e_labels: inside the one extra layer
        while layer.size:
            ev.largest_layer = max(ev.largest_layer, int(layer.size))
            found, nxt = False, []
            for u in layer:
                pu = pair_v[packed[u]]
                found = found or bool((pu == -1).any())
                new = np.unique(pu[pu >= 0])
                new = new[dist[new] == INF]
                dist[new] = L + 1
                nxt.append(new)
            nxt = np.concatenate(nxt) if nxt else np.zeros(0, dtype=np.int64)
            L += 1
            if extra:
                if variant == "e":
                    nil = L
                break
            if found:
                nil = L
                if variant in ("e", "e_labels") and nxt.size:
                    extra, layer = True, nxt
                    continue
                ev.nil_rows += int(nxt.size)
                break
            layer = nxt
        ev.layers.append(L)
        if nil == INF:
            break
        ev.phases += 1

        # ---- DFS
        augmented = 0
        for base in range(0, n, WAVE):
            if variant == "f" and base + WAVE > n:
                break
            for root in [u for u in range(base, min(base + WAVE, n)) if pair_u[u] == -1]:
                ev.root_chunks.add((base // WAVE, base + WAVE > n))
                depth, u, g = 0, root, 0
                row = rows[u]
                g1 = len(row)
                pending = -1  # the failure record that waits to learn whether its parent finds a later hit
                while True:
                    k, chunks = -1, 0
                    while g < g1:
                        e = min(g + WAVE, g1)
                        if variant == "c" and g % WAVE:
                            e = min(e, (g // WAVE + 1) * WAVE)
                        c = row[g:e]
                        cp = pair_v[np.maximum(c, 0)]
                        d = np.where(cp == -1, depth + 1 if variant == "d" else nil, dist[np.maximum(cp, 0)])
                        q = np.flatnonzero((c >= 0) & (d != INF) & (d == depth + 1))
                        if q.size:
                            k = int(q[-1] if variant == "a" else q[0])
                            v, pu = int(c[k]), int(cp[k])
                            ev.hits.append(Hit(g1, g + k, k, g % WAVE == 0, depth))
                            if pending >= 0:
                                ev.fails[pending] = ev.fails[pending]._replace(later_hit=True, later_chunk=chunks)
                            g += k + 1
                            break
                        ev.skipped += 1
                        ev.skipped_unaligned += g % WAVE != 0
                        chunks += 1
                        g += WAVE
                    pending = -1
                    if k >= 0 and pu != -1:  # recurse into the column's row
                        st_u[depth], st_g[depth] = u, g
                        depth += 1
                        ev.max_depth = max(ev.max_depth, depth)
                        u, g = pu, 0
                        row = rows[u]
                        g1 = len(row)
                        continue
                    if k >= 0:  # a free column: every level takes the entry before its resume position
                        pair_v[v], pair_u[u] = u, v
                        for lv in range(depth):
                            uu, pos = st_u[lv], st_g[lv] - 1
                            src = packed[uu] if variant == "g" else rows[uu]
                            vv = int(src[pos]) if pos < len(src) else -1  # (only g can read past the end)
                            if vv >= 0:
                                pair_v[vv], pair_u[uu] = uu, vv
                        augmented += 1
                        break
                    dist[u] = INF
                    if depth == 0:
                        break
                    depth -= 1
                    u, g = st_u[depth], st_g[depth]
                    row = rows[u]
                    g1 = len(row)
                    ev.fails.append(Fail(g1, g, False, -1, depth))
                    pending = len(ev.fails) - 1
                    if variant == "b":
                        g = -(-g // WAVE) * WAVE
        ev.augmented += augmented
        if augmented == 0:
            break
    left, right = pair_u.astype(np.int32), pair_v.astype(np.int32)
    return left, right, int((left != -1).sum()), ev
