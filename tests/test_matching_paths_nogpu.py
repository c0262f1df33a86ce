"""The cases of _matching_shapes.py without a GPU: the model that gives their expectations is the host matcher's
algorithm (hence, through tests/golden/matching_cases.*, the reference's), the cases reach the steps of the DFS they are
drawn for, and they tell the right algorithm from each deliberately wrong variant of the model.  What the older random
graphs of test_matching_batch.py could not see is recorded at the end."""
import numpy as np
import pytest

import _matching_model as model
import _matching_shapes as S
import cases as golden_cases
from sslap_amd.check_feasible import _solve

SOURCES = ("loc", "dense", "ell")


def _host(rows, n, m):
    """The library's host Hopcroft-Karp on the entries of `rows` in stored order, the holes dropped."""
    loc = np.array([(u, c) for u, r in enumerate(rows) for c in r if c >= 0], dtype=np.int32).reshape(-1, 2)
    return _solve(loc, n, m)


def _same(got, want):
    return (got[2] == want["size"] and np.array_equal(got[0], want["left_pairings"]) and
            np.array_equal(got[1], want["right_pairings"]))


@pytest.mark.parametrize("source", SOURCES)
def test_model_equals_host_matcher_on_every_case(source, built_lib):
    for name, K in S.instances(source):
        rows, n, m = S.source_rows(name, source, K)
        e = S.expect(name, source, K)
        assert (e.n, e.m) == (n, m)
        assert _same((e.left, e.right, e.size), _host(rows, n, m)), (name, K)


def test_model_equals_the_reference_on_every_golden_matching_case(golden_matching, built_lib):
    man, arr = golden_matching
    for name, (spec, _) in golden_cases.MATCH_CASES.items():
        loc = golden_cases.matching_graph(spec)
        n, m = arr[name + "/left"].shape[0], arr[name + "/right"].shape[0]
        rows = [loc[loc[:, 0] == u, 1] for u in range(n)]
        left, right, size, _ = model.solve(rows, m)
        assert size == man["cases"][name]["size"], name
        assert np.array_equal(left, arr[name + "/left"]) and np.array_equal(right, arr[name + "/right"]), name
        assert _same((left, right, size), _host(rows, n, m)), name


def test_the_cases_are_what_their_names_say():
    cs = S.cases()
    sizes = [S.expect(f"hot160_s{s}", "loc").size for s in S.HOT_160_SEEDS]
    assert 160 in sizes and 159 in sizes  # a feasible draw and one short by exactly one row
    for src in ("loc", "dense"):
        for p in S.GADGET_P:
            assert S.expect(f"gadget{p}_later", src).size == p + 5 == cs[f"gadget{p}_later"].n
            assert S.expect(f"gadget{p}_end", src).size == p + 4 == cs[f"gadget{p}_end"].n - 1
    lane, wave = S.loc_of(cs["bfs300_lane"]), S.loc_of(cs["bfs300_wave"])
    assert lane.shape[0] == 16 * S.BFS_N and wave.shape[0] == 16 * S.BFS_N + 1  # on both sides of the loc BFS's switch
    assert cs["bfs300_lane"].n == cs["bfs300_wave"].n == S.BFS_N
    assert any(len(r) == 0 for r in cs["bfs300_lane"].rows)  # row gaps
    assert S.has_repeated_entry(cs["bfs300_wave"]) and "bfs300_wave" not in S.names("dense")
    assert max(c.n for c in cs.values() if c.name != "deep") <= 320 and max(c.m for c in cs.values() if c.name != "deep") <= 320
    for name, K in S.instances("ell"):  # the holes sit between the entries: positions shift relative to loc
        slots = S.ell_slots(name, K)
        assert all(np.array_equal(r[r >= 0], c) for r, c in zip(slots, cs[name].rows)), name
    assert any((S.ell_slots(name, K)[:, 0] < 0).any() for name, K in S.instances("ell"))
    assert {K for _, K in S.instances("ell")} == set(S.ELL_KS)


def _events(source):
    return [(name, K, S.expect(name, source, K).events) for name, K in S.instances(source)]


@pytest.mark.parametrize("source", SOURCES)
def test_required_events(source):
    """Conditions on the inputs: what the true algorithm does on them.  If a draw misses one, the draw changes."""
    evs = _events(source)
    fails = [f for _, _, e in evs for f in e.fails]
    hits = [h for _, _, e in evs for h in e.hits]
    # a hit at each listed position p whose child fails, and both outcomes after the resume at p + 1.  No ELL row here
    # is longer than 110 slots, so 127 and 128 (and a later chunk after a resume beyond 63) cannot occur in that source.
    for p in S.POSITIONS:
        if source == "ell" and p + 2 > max(S.ELL_KS):
            continue
        later = [f for f in fails if f.resume == p + 1 and f.later_hit]
        end = [f for f in fails if f.resume == p + 1 and not f.later_hit]
        assert later and end, (source, p)
        if source == "loc":  # the row has length p + 2 in one graph and p + 1 (g == g1 after the hit) in the other
            assert any(f.row_len == p + 2 for f in later) and any(f.row_len == p + 1 for f in end), p
    assert any(h.lane == 63 and not h.aligned for h in hits)
    assert any(f.resume > 63 and f.later_hit for f in fails)
    assert any(f.later_hit and f.later_chunk > 0 for f in fails)
    if source != "ell":
        assert any(f.resume > 63 and f.later_hit and f.later_chunk > 0 for f in fails)
    assert sum(e.skipped_unaligned for _, _, e in evs) > 0  # a skipped chunk after an unaligned resume
    assert any(e.max_depth >= 3 for name, _, e in evs if name != "deep")
    deep = S.expect("deep", source, 110 if source == "ell" else None).events
    assert deep.max_depth >= 200
    # ... whose stack holds a resume position beyond 63 at (nearly) every depth at once
    assert sum(h.pos > 63 and h.depth >= 1 for h in deep.hits) >= 200
    assert any(e.phases >= 3 for _, _, e in evs)
    assert any(e.nil_rows > 0 for _, _, e in evs)
    chunks = set().union(*(e.root_chunks for _, _, e in evs))
    assert any(i >= 1 and not last for i, last in chunks) and any(i >= 1 and last for i, last in chunks)
    assert any(i == 0 and last for i, last in chunks)  # (n < 64: the only chunk is a partial one)
    # the BFS: more rows in a layer than threads with one row per lane, more than wavefronts with one row per wavefront
    if source == "loc":
        assert S.expect("bfs300_lane", "loc").events.largest_layer > 256
        assert S.expect("bfs300_wave", "loc").events.largest_layer > 4
    if source == "ell":
        assert S.expect("bfs300", "ell", 16).events.largest_layer > 256
        assert S.expect("bfs300", "ell", 17).events.largest_layer > 4
    if source == "dense":
        assert max(e.largest_layer for _, _, e in evs) > 4 * 64


def _killed_by(variant, source, instances):
    """The instances of a source on which a variant changes left_pairings or size."""
    out = []
    for name, K in instances:
        want, got = S.expect(name, source, K), S.expect(name, source, K, variant)
        if got.size != want.size or not np.array_equal(got.left, want.left):
            out.append((name, K))
    return out


# (g is about the holes of ELL rows: it applies to that source alone)
@pytest.mark.parametrize("variant,source", [(v, s) for v in sorted(model.VARIANTS) for s in SOURCES if v != "g" or s == "ell"])
def test_every_variant_changes_a_result(variant, source):
    assert _killed_by(variant, source, S.instances(source)), (variant, source)


def test_labels_above_dist_nil_alone_change_nothing():
    """(e) without its dist_nil: see INVISIBLE_VARIANTS in the model."""
    for source in SOURCES:
        assert _killed_by("e_labels", source, S.instances(source)) == []


def older_random_graphs():
    """The four first 60 x 90 graphs, at most 3 entries per row, of test_matching_batch.test_random_graphs_equal_host."""
    from test_matching_batch import _random_graph
    rng = np.random.default_rng(60 * 7 + 90)
    return [_random_graph(rng, 60, 90, 3) for _ in range(4)]


def unchanged_on_the_older_graphs():
    """variant -> on how many of the four draws it leaves size and left_pairings as they are."""
    out = {}
    for variant in sorted(model.VARIANTS):
        if variant == "g":
            continue  # (a loc has no holes)
        out[variant] = 0
        for loc in older_random_graphs():
            n, m = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
            rows = [loc[loc[:, 0] == u, 1] for u in range(n)]
            want, got = model.solve(rows, m), model.solve(rows, m, variant)
            out[variant] += got[2] == want[2] and np.array_equal(got[0], want[0])
    return out


def test_record_of_what_the_older_random_graphs_could_not_see(built_lib):
    """Not a requirement on the library: the gap this suite closes.  On the four 60 x 90 draws the model is the host
    matcher and the DFS does recurse and fail, but never beyond stored position 2 -- and a scan that loses the tail of an
    unaligned chunk (c) leaves all four results as they are, a free column that qualifies at any depth (d) three of
    them."""
    for loc in older_random_graphs():
        n, m = int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
        rows = [loc[loc[:, 0] == u, 1] for u in range(n)]
        left, right, size, ev = model.solve(rows, m)
        assert _same((left, right, size), _host(rows, n, m))
        assert ev.max_depth >= 1 and ev.fails and max(f.resume for f in ev.fails) <= 3
    assert unchanged_on_the_older_graphs() == dict(a=0, b=0, c=4, d=3, e=0, f=0)
