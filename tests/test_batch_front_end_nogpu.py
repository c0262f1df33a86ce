"""The Python side of the six "verdict per problem" batch calls without a GPU and without the built library: what each
front end hands to its entry point comes back as its result.

A stand-in for the library returns 0 and, before it does, writes recognisable values through the output pointers it was
given: sol, prices_out, outside_prices_out, status = 0, matching_size, n_rows / n_cols / nnz of every record (at the
stride element 0's struct_size names) and info.threads.  Each front end runs on two problems of 2 x 3 from host arrays
and must return exactly those values, in arrays of its documented shapes and types, under exactly its keys.

errors="raise": the four calls that run the status call in both modes (outside=, and the ELL layout) are called with it.
For the dense and the sparse call without outside, errors="raise" on host input is the default mode's own entry point,
which gives no verdict per problem; there raise_for_status takes the errors="status" result, which is what
errors="raise" does wherever it runs the status call.
"""
import ctypes as C

import numpy as np
import pytest

from sslap_amd import (_lib, auction_solve_batch, auction_solve_ell_batch, auction_solve_sparse_batch, batch_meta_to_host,
                       ell_to_packed, raise_for_status)

B, N, M, K = 2, 2, 3, 2
RECORD = C.sizeof(_lib.DenseBatchMeta)

MATS = np.array([[[1.0, -1.0, 3.0], [2.0, 5.0, -1.0]], [[4.0, 2.0, -1.0], [0.0, 1.0, 2.0]]])
COLS = np.array([[[0, 2], [0, 1]], [[0, 1], [1, 2]]], dtype=np.int32)
VALS = np.array([[[1.0, 3.0], [2.0, 5.0]], [[4.0, 2.0], [1.0, 2.0]]])
_PACKED = ell_to_packed(COLS, VALS)
LOC = np.ascontiguousarray(np.concatenate([l for l, _ in _PACKED]), dtype=np.int32)
VAL = np.ascontiguousarray(np.concatenate([v for _, v in _PACKED]), dtype=np.float64)
OFFSETS = np.concatenate([[0], np.cumsum([len(v) for _, v in _PACKED])]).astype(np.int64)
OUTSIDE = np.array([[2.0, 9.0], [7.0, 3.0]])

# what the stand-in writes
SOL = np.array([[11, 12], [13, 14]], dtype=np.int32)
PRICES = np.array([[0.5, 1.5, 2.5], [3.5, 4.5, 5.5]])
OUTSIDE_PRICES = np.array([[100.25, 101.25], [102.25, 103.25]])
MATCHING_SIZE = np.array([7, 8], dtype=np.int32)
N_ROWS, N_COLS, NNZ, THREADS = np.array([2, 1]), np.array([3, 5]), np.array([4, 2**33 + 1]), 192

# per front end: (the call, its input, its keywords, the entry point, the result's keys)
FRONT_ENDS = {
    "dense_status": (auction_solve_batch, (MATS,), dict(), "misslap_solve_dense_batch_status",
                     {"sol", "prices", "status", "matching_size", "meta", "shapes", "stack"}),
    "dense_outside": (auction_solve_batch, (MATS,), dict(outside=OUTSIDE), "misslap_solve_dense_batch_outside",
                      {"sol", "prices", "outside_prices", "status", "matching_size", "meta", "shapes", "stack", "outside"}),
    "sparse_status": (auction_solve_sparse_batch, (LOC, VAL, OFFSETS), dict(), "misslap_solve_sparse_batch_status",
                      {"sol", "prices", "status", "matching_size", "meta", "layout", "dims", "sizes", "offsets", "loc",
                       "prices_ld"}),
    "sparse_outside": (auction_solve_sparse_batch, (LOC, VAL, OFFSETS), dict(outside=OUTSIDE),
                       "misslap_solve_sparse_batch_outside",
                       {"sol", "prices", "outside_prices", "status", "matching_size", "meta", "layout", "dims", "sizes",
                        "offsets", "loc", "prices_ld"}),
    "ell": (auction_solve_ell_batch, (COLS, VALS), dict(), "misslap_solve_ell_batch",
            {"sol", "prices", "status", "matching_size", "meta", "rows", "layout", "stack", "n_cols", "prices_ld"}),
    "ell_outside": (auction_solve_ell_batch, (COLS, VALS), dict(outside=OUTSIDE), "misslap_solve_ell_batch_outside",
                    {"sol", "prices", "outside_prices", "status", "matching_size", "meta", "rows", "layout", "stack", "n_cols",
                     "prices_ld"}),
}
RAISES_THROUGH_THE_STATUS_CALL = ("dense_outside", "sparse_outside", "ell", "ell_outside")


def _address(p):
    return p.value if isinstance(p, C.c_void_p) else int(p)


def _fill(p, values):
    ctype = np.ctypeslib.as_ctypes_type(values.dtype)
    np.ctypeslib.as_array(C.cast(_address(p), C.POINTER(ctype)), values.shape)[...] = values


class _Library:
    """Stands in for the library: every entry point records its name and its arguments, writes the values above through
    the output pointers of the argument tail the status-mode entry points share, and returns 0.  bad: the status of
    problem 1."""

    def __init__(self, bad=0):
        self.calls = []
        self.bad = bad

    def __getattr__(self, name):
        if not name.startswith("misslap_solve_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            # ..., sol, prices_out, [outside_prices_out], out_on_device, status, matching_size, meta, info
            outs = list(args[-8:-5]) if name.endswith("outside") else list(args[-7:-5])
            on_device, status, matching_size, meta, info = args[-5:]
            assert on_device == 0
            _fill(outs[0], SOL)
            _fill(outs[1], PRICES)
            if name.endswith("outside"):
                _fill(outs[2], OUTSIDE_PRICES)
            _fill(status, np.array([0, self.bad], dtype=np.int32))
            _fill(matching_size, MATCHING_SIZE)
            stride = _lib.DenseBatchMeta.from_address(_address(meta)).struct_size
            assert stride == RECORD
            for b in range(B):
                rec = _lib.DenseBatchMeta.from_address(_address(meta) + b * stride)
                rec.n_rows, rec.n_cols, rec.nnz = int(N_ROWS[b]), int(N_COLS[b]), int(NNZ[b])
            info._obj.threads = THREADS
            return 0
        return call


def _run(monkeypatch, name, bad=0, **kw):
    f, args, own, entry, keys = FRONT_ENDS[name]
    lib = _Library(bad)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    res = f(*args, **dict(own, **kw))
    assert [c[0] for c in lib.calls] == [entry]  # one call, of this front end's entry point
    return res


@pytest.mark.parametrize("name", list(FRONT_ENDS))
def test_what_the_library_writes_is_what_the_front_end_returns(monkeypatch, name):
    res = _run(monkeypatch, name, errors="status")
    assert set(res) == FRONT_ENDS[name][4]
    outside = name.endswith("outside")
    want = dict(sol=SOL, prices=PRICES, status=np.zeros(B, dtype=np.int32), matching_size=MATCHING_SIZE)
    if outside:
        want["outside_prices"] = OUTSIDE_PRICES
    for key, w in want.items():
        got = res[key]
        assert isinstance(got, np.ndarray) and got.dtype == w.dtype and got.shape == w.shape, key
        assert np.array_equal(got, w), key
    meta = res["meta"]
    for key, w in (("n_rows", N_ROWS), ("n_cols", N_COLS), ("nnz", NNZ)):
        assert meta[key].dtype == np.int64 and meta[key].shape == (B,) and np.array_equal(meta[key], w), key
    for key in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "bids_made", "obj", "obj_f64", "start_eps", "final_eps"):
        assert meta[key].shape == (B,) and not meta[key].any(), key  # the records start as zeros
    assert meta["gpu"]["threads"] == THREADS and meta["gpu"]["lds_bytes"] == 0
    assert batch_meta_to_host(res) is res["meta"]
    assert raise_for_status(res) is res
    # the keys of its own each front end adds
    if name.startswith("dense"):
        assert res["stack"] == (N, M) and res["shapes"] is None
        if outside:
            assert np.array_equal(res["outside"], OUTSIDE) and res["outside"].dtype == np.float64
    elif name.startswith("sparse"):
        assert (res["layout"], res["dims"], res["sizes"], res["prices_ld"]) == ("sparse", (N, M), None, 0)
        assert res["loc"] is LOC and np.array_equal(res["offsets"], OFFSETS) and res["offsets"].dtype == np.int64
    else:
        assert (res["layout"], res["stack"], res["n_cols"], res["rows"], res["prices_ld"]) == ("ell", (N, K), M, None, 0)


@pytest.mark.parametrize("name", list(FRONT_ENDS))
def test_a_status_that_is_not_zero_raises_for_its_problem(monkeypatch, name):
    bad = _lib.BATCH_STATUS_INFINITE_VALUE  # a code of every layout and mode
    with pytest.raises(ValueError, match=r"^problem 1: val holds a NaN or an infinity"):
        if name in RAISES_THROUGH_THE_STATUS_CALL:
            _run(monkeypatch, name, bad=bad, errors="raise")
        else:
            raise_for_status(_run(monkeypatch, name, bad=bad, errors="status"))
    res = _run(monkeypatch, name, bad=bad, errors="status")  # the status mode hands the verdict back
    assert res["status"].tolist() == [0, bad]
