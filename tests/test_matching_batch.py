"""hopcroft_solve_batch on the GPU (misslap_matching_batch / misslap_matching_dense_batch: one workgroup per graph)
against the real reference's golden vectors and against the host `hopcroft_solve` on every graph -- the same size and
the same pairing arrays, bit for bit, not just some maximum matching."""
import numpy as np
import pytest

import cases
from sslap_amd import hopcroft_solve, hopcroft_solve_batch

pytestmark = pytest.mark.gpu

CAP = 2048


def _pack(locs):
    loc = np.ascontiguousarray(np.concatenate(locs).reshape(-1, 2), dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([x.shape[0] for x in locs])]).astype(np.int64)
    return loc, offsets


def _check_row(res, b, want):
    n, m = want["left_pairings"].shape[0], want["right_pairings"].shape[0]
    left, right = np.asarray(res["left_pairings"][b]), np.asarray(res["right_pairings"][b])
    assert res["size"][b] == want["size"], b
    assert res["n_rows"][b] == n and res["n_cols"][b] == m, b
    assert np.array_equal(left[:n], want["left_pairings"]), b
    assert np.array_equal(right[:m], want["right_pairings"]), b
    assert (left[n:] == -1).all() and (right[m:] == -1).all(), b


def _check_loc(locs, res=None):
    if res is None:
        res = hopcroft_solve_batch(*_pack(locs))
    for b, lb in enumerate(locs):
        _check_row(res, b, hopcroft_solve(loc=lb))
    return res


def _random_graph(rng, n, m, per_row, gaps=False, dups=False):
    """rows ascending, per_row random columns per row (stored order random); with gaps some rows have no entry."""
    rows = np.arange(n)
    if gaps:
        rows = rows[rng.random(n) < 0.7]
        rows = np.union1d(rows, [n - 1])
    k = rng.integers(1, per_row + 1, rows.shape[0])
    r = np.repeat(rows, k)
    c = rng.integers(0, m, r.shape[0])
    if dups:
        take = rng.random(r.shape[0]) < 0.2
        r = np.concatenate([r, r[take]])
        c = np.concatenate([c, c[take]])
        order = np.argsort(r, kind="stable")
        r, c = r[order], c[order]
    c[-1] = m - 1  # (the graph's m is max column + 1)
    return np.ascontiguousarray(np.stack([r, c], axis=1), dtype=np.int32)


def test_golden_cases_batched_together(golden_matching):
    man, arr = golden_matching
    names = sorted(cases.MATCH_CASES)
    locs, mats = [], []
    for name in names:
        spec, entry = cases.MATCH_CASES[name]
        loc = cases.matching_graph(spec).astype(np.int32)
        if entry == "mat":
            mats.append((name, cases.matching_call(loc, spec, entry)["mat"]))
        else:  # (a lookup dict is its loc in stored order)
            locs.append((name, loc))
    res = hopcroft_solve_batch(*_pack([x[1] for x in locs]))
    for b, (name, _) in enumerate(locs):
        left, right = arr[name + "/left"], arr[name + "/right"]
        assert res["size"][b] == man["cases"][name]["size"], name
        assert np.array_equal(res["left_pairings"][b, :left.shape[0]], left), name
        assert np.array_equal(res["right_pairings"][b, :right.shape[0]], right), name
    assert any(res["size"][b] < res["n_rows"][b] for b in range(len(locs)))  # the infeasible thinned / narrow cases
    for name, mat in mats:
        r = hopcroft_solve_batch(mats=mat[None])
        assert r["size"][0] == man["cases"][name]["size"], name
        assert np.array_equal(r["left_pairings"][0], arr[name + "/left"]), name
        assert np.array_equal(r["right_pairings"][0], arr[name + "/right"]), name


@pytest.mark.parametrize("shape", [(60, 90, 3), (90, 60, 3), (200, 200, 2), (300, 150, 8), (64, 1000, 40)])
def test_random_graphs_equal_host(shape):
    n, m, k = shape
    rng = np.random.default_rng(n * 7 + m)
    _check_loc([_random_graph(rng, n, m, k) for _ in range(12)])


def test_row_gaps_duplicates_and_single_entry_rows():
    rng = np.random.default_rng(3)
    locs = [_random_graph(rng, 80, 70, 4, gaps=True) for _ in range(5)]
    locs += [_random_graph(rng, 70, 80, 5, dups=True) for _ in range(5)]
    locs += [_random_graph(rng, 50, 50, 1) for _ in range(3)]  # one entry per row
    locs.append(np.array([[5, 3]], dtype=np.int32))  # rows 0..4 absent, one edge
    locs.append(np.array([[0, 0], [0, 0], [0, 0]], dtype=np.int32))
    _check_loc(locs)


def test_complete_graph_at_the_cap():
    i, j = np.meshgrid(np.arange(CAP, dtype=np.int32), np.arange(CAP, dtype=np.int32), indexing="ij")
    full = np.ascontiguousarray(np.stack([i.ravel(), j.ravel()], axis=1))
    res = _check_loc([full])
    assert res["size"][0] == CAP and res["left_pairings"].shape == (1, CAP)


def test_chain_graph_reaches_full_depth():
    """Row i stores (i, i + 1) then (i, i); row n - 1 only (n - 1, n - 1): the second phase's one augmenting path runs
    through every row."""
    n = CAP
    rows = np.concatenate([np.repeat(np.arange(n - 1), 2), [n - 1]])
    cols = np.concatenate([np.stack([np.arange(1, n), np.arange(n - 1)], axis=1).ravel(), [n - 1]])
    chain = np.ascontiguousarray(np.stack([rows, cols], axis=1), dtype=np.int32)
    res = _check_loc([chain, chain[: 2 * 100 - 1].copy()])
    assert res["size"][0] == n
    assert np.array_equal(res["left_pairings"][0], np.arange(n))


@pytest.mark.parametrize("B", [1, 4096])
def test_batch_sizes(B):
    rng = np.random.default_rng(B)
    locs = [_random_graph(rng, int(rng.integers(1, 40)), int(rng.integers(1, 40)), 3) for _ in range(B)]
    _check_loc(locs)


def test_mixed_sizes_in_one_call():
    rng = np.random.default_rng(5)
    dims = [(1, 1), (2048, 16), (16, 2048), (700, 900), (3, 5), (1500, 1500), (40, 40)]
    _check_loc([_random_graph(rng, n, m, 6) for n, m in dims])


def test_list_input_equals_packed_input():
    rng = np.random.default_rng(6)
    locs = [_random_graph(rng, 30, 30, 3) for _ in range(5)]
    packed = hopcroft_solve_batch(*_pack(locs))
    listed = hopcroft_solve_batch([x.astype(np.int64) for x in locs])
    for k in ("size", "left_pairings", "right_pairings", "n_rows", "n_cols"):
        assert np.array_equal(packed[k], listed[k]), k


def _dense_stack(rng, B, N, M):
    mats = rng.uniform(-1.0, 1.0, (B, N, M))
    mats[rng.random((B, N, M)) < 0.15] = np.nan
    mats[rng.random((B, N, M)) < 0.05] = -0.0
    mats[rng.random((B, N, M)) < 0.05] = np.inf
    mats[rng.random((B, N, M)) < 0.02] = -np.inf
    return mats


def test_dense_stack_with_holes_nan_signed_zero_inf_and_shapes():
    rng = np.random.default_rng(7)
    B, N, M = 9, 70, 90
    mats = _dense_stack(rng, B, N, M)
    shapes = np.array([[70, 90], [1, 1], [70, 1], [1, 90], [33, 47], [69, 12], [12, 69], [50, 50], [70, 89]])
    before = mats.copy()
    res = hopcroft_solve_batch(mats=mats, shapes=shapes)
    assert np.array_equal(mats.view(np.uint64), before.view(np.uint64))  # never written
    assert res["left_pairings"].shape == (B, 70) and res["right_pairings"].shape == (B, 90)
    for b, (n, m) in enumerate(shapes):
        _check_row(res, b, hopcroft_solve(mat=mats[b, :n, :m]))
    full = hopcroft_solve_batch(mats=mats)
    for b in range(B):
        _check_row(full, b, hopcroft_solve(mat=mats[b]))


def test_device_tensors_in_and_out():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(8)
    mats = _dense_stack(rng, 5, 40, 60)
    want = hopcroft_solve_batch(mats=mats)
    got = hopcroft_solve_batch(mats=torch.from_numpy(mats).cuda())
    assert got["left_pairings"].is_cuda and got["right_pairings"].is_cuda
    for k in ("left_pairings", "right_pairings"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert np.array_equal(got["size"], want["size"])


def test_device_loc_written_on_a_side_stream():
    """The Python call on a loc still being written on the current stream.  (hopcroft_solve_batch reduces loc for the
    output sizes on that stream before it calls the library, so this covers the wrapper; the library's own ordering
    behind input_stream is the next test.)"""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(9)
    locs = [_random_graph(rng, int(rng.integers(10, 200)), 150, 5, gaps=True) for _ in range(32)]
    loc, offsets = _pack(locs)
    want = _check_loc(locs)
    src = torch.from_numpy(loc).cuda()
    side = torch.cuda.Stream()
    lx = torch.full_like(src, -1)
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)  # the copy below lands long after the call was made
        lx.copy_(src)
        got = hopcroft_solve_batch(lx, offsets)
    torch.cuda.synchronize()
    assert got["left_pairings"].is_cuda and got["left_pairings"].device == lx.device
    for k in ("left_pairings", "right_pairings"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    for k in ("size", "n_rows", "n_cols"):
        assert np.array_equal(got[k], want[k]), k
    assert torch.equal(lx, src)  # read in place, not written


def test_c_entry_point_orders_behind_input_stream():
    """misslap_matching_batch called directly, with options.input_stream = a side stream on which loc is still being
    written when the call is made: the library must order its reads behind that stream."""
    import ctypes as C
    torch = pytest.importorskip("torch")
    from sslap_amd import _lib
    rng = np.random.default_rng(10)
    locs = [_random_graph(rng, int(rng.integers(10, 200)), 150, 5, gaps=True) for _ in range(32)]
    loc, offsets = _pack(locs)
    want = _check_loc(locs)
    B, Nmax, Mmax = len(locs), int(loc[:, 0].max()) + 1, int(loc[:, 1].max()) + 1
    src = torch.from_numpy(loc).cuda()
    lx = torch.full_like(src, -1)
    left = torch.empty((B, Nmax), dtype=torch.int32, device=src.device)
    right = torch.empty((B, Mmax), dtype=torch.int32, device=src.device)
    size, n_rows, n_cols = (np.empty(B, dtype=np.int32) for _ in range(3))
    opts = _lib.Options()
    opts.struct_size = C.sizeof(_lib.Options)
    opts.device = src.device.index or 0
    opts.input_on_device = 1
    side = torch.cuda.Stream()
    opts.input_stream = C.c_void_p(int(side.cuda_stream))
    info = _lib.MatchingBatchInfo()
    info.struct_size = C.sizeof(_lib.MatchingBatchInfo)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)  # the copy below lands long after the call was made
        lx.copy_(src)
    _lib.check(_lib.load().misslap_matching_batch(
        B, C.c_void_p(lx.data_ptr()), offsets.ctypes.data, C.byref(opts), size.ctypes.data, n_rows.ctypes.data,
        n_cols.ctypes.data, C.c_void_p(left.data_ptr()), Nmax, C.c_void_p(right.data_ptr()), Mmax, 1, C.byref(info)))
    torch.cuda.synchronize()
    assert np.array_equal(left.cpu().numpy(), want["left_pairings"])
    assert np.array_equal(right.cpu().numpy(), want["right_pairings"])
    for k, got in (("size", size), ("n_rows", n_rows), ("n_cols", n_cols)):
        assert np.array_equal(got, want[k]), k


def _error(locs, match):
    with pytest.raises(ValueError, match=match):
        hopcroft_solve_batch(*_pack(locs))


def test_errors_name_the_graph_and_match_host_texts():
    ok = np.array([[0, 0], [1, 1]], dtype=np.int32)
    _error([ok, np.zeros((0, 2), np.int32), ok], r"^graph 1: no entries$")
    neg = np.array([[0, 0], [1, -2], [2, 1]], dtype=np.int32)
    with pytest.raises(ValueError) as host:
        hopcroft_solve(loc=neg)
    _error([ok, ok, neg], "^graph 2: " + host.value.args[0].replace("(", r"\(").replace(")", r"\)") + "$")
    assert "loc entry 1 = (1, -2) outside 3 x 2" in host.value.args[0]
    unsorted = np.array([[0, 0], [2, 1], [1, 1]], dtype=np.int32)
    _error([unsorted, neg], r"^graph 0: loc rows must be sorted in ascending order$")
    negrow = np.array([[-1, 0], [0, 1]], dtype=np.int32)
    _error([ok, negrow], r"^graph 1: loc entry 0 = \(-1, 0\) outside 1 x 2$")
    big = np.array([[0, 0], [2048, 3]], dtype=np.int32)
    _error([ok, big], r"^graph 1: 2049 x 4 exceeds MISSLAP_MATCHING_BATCH_MAX_DIM \(2048\)$")
    wide = np.array([[0, 2048]], dtype=np.int32)
    _error([wide, big], r"^graph 0: 1 x 2049 exceeds MISSLAP_MATCHING_BATCH_MAX_DIM \(2048\)$")
    with pytest.raises(ValueError, match=r"^graph 0: 2049 x 3 exceeds MISSLAP_MATCHING_BATCH_MAX_DIM \(2048\)$"):
        hopcroft_solve_batch(mats=np.ones((1, 2049, 3)))
    with pytest.raises(ValueError, match=r"^graph 1: 3000 x 3 exceeds"):
        hopcroft_solve_batch(mats=np.ones((2, 3000, 3)), shapes=np.array([[5, 3], [3000, 3]]))
