"""The outside mode of auction_solve_sparse_batch (misslap_solve_sparse_batch_outside) without a GPU: the definition
(`sparse_to_augmented` against a plain double loop, and against `ell_to_packed(outside=)` on problems written in both
layouts), the front end's checks and its resolution of `fast`, the C entry point's argument errors, the workspace size,
the order of the verdict, and the optimality of the definition: on the augmented problem the oracle's single phase
(fast=True) reaches the optimum of scipy's linear_sum_assignment on every gapped draw.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from sslap_amd import _lib, auction_solve_sparse_batch, ell_to_packed, sparse_to_augmented
from tests import _sparse_outside_fixture as fxt
from tests._batch_shapes import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("misslap_solve_sparse_batch_outside", "misslap_sparse_batch_outside_workspace_bytes")


def test_entry_points_are_declared_bound_and_exported(built_lib):
    import sslap_amd
    header = open(os.path.join(ROOT, "include", "misslap.h")).read()
    declared = set(re.findall(r"\b(misslap_[a-z_0-9]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
        assert getattr(built_lib, name) is not None
        assert name in header.split("Additions since")[1].split("*/")[0], name
    assert "sparse_to_augmented" in sslap_amd.__all__ and sslap_amd.sparse_to_augmented is sparse_to_augmented


# ---- sparse_to_augmented is the definition

def augmented_by_loops(loc, val, offsets, sizes, outside):
    """Problem b: its entries in stored order, and behind the stored entries of row i (a row without any included) the
    entry (i, m_b + i) with the row's outside value; n_b = sizes[b][1], else the last stored row + 1; m_b = max column + 1."""
    out = []
    for b in range(len(offsets) - 1):
        ent = [(int(loc[k][0]), int(loc[k][1]), float(val[k])) for k in range(offsets[b], offsets[b + 1])]
        n = int(sizes[b][1]) if sizes is not None else (ent[-1][0] + 1 if ent else 0)
        m = 0
        for _, j, _ in ent:
            m = max(m, j + 1)
        lo, va = [], []
        for i in range(n):
            for r, j, v in ent:
                if r == i:
                    lo.append((i, j))
                    va.append(v)
            lo.append((i, m + i))
            o = outside if np.ndim(outside) == 0 else outside[b] if np.ndim(outside) == 1 else outside[b][i]
            va.append(float(o))
        out.append((np.array(lo, dtype=np.int32).reshape(-1, 2), np.array(va, dtype=np.float64), m, n))
    return out


def _batch():
    """Leading, middle and trailing gaps, duplicates (adjacent and apart), a problem without an entry, n_b > m_b."""
    rng = np.random.default_rng(5)
    dup = (np.array([[0, 2], [0, 2], [1, 0], [1, 3], [1, 0], [3, 1], [3, 1]], dtype=np.int32), rng.uniform(0, 9, 7))
    probs = [fxt.ragged(rng, np.array([0, 0, 2, 3]), 5, "uniform"), fxt.ragged(rng, np.array([2, 0, 0, 0, 1, 0, 2]), 4, "ints"),
             dup, (np.zeros((0, 2), dtype=np.int32), np.zeros(0)), fxt.ragged(rng, np.array([1, 1, 1, 1, 1, 1]), 2, "ints")]
    sizes = np.array([[7, 4], [0, 9], [-1, 6], [5, 3], [2, 6]], dtype=np.int64)  # trailing gaps where n_b > last row + 1
    return probs, sizes


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row", "default"])
@pytest.mark.parametrize("with_sizes", [False, True])
def test_sparse_to_augmented_is_the_double_loop(form, with_sizes):
    probs, sizes = _batch()
    loc, val, off = fxt.pack(probs)
    B = len(probs)
    rng = np.random.default_rng(7)
    outside = {"scalar": -2.5, "per_problem": rng.uniform(-5, 10, B), "per_row": rng.uniform(-5, 10, (B, 11)),
               "default": 0.0}[form]
    sz = sizes if with_sizes else None
    got = sparse_to_augmented(loc, val, off, sz) if form == "default" else sparse_to_augmented(loc, val, off, sz, outside)
    want = augmented_by_loops(loc, val, off, sz, outside)
    assert len(got) == len(want) == B
    for b, ((gl, gv, gm, gn), (wl, wv, wm, wn)) in enumerate(zip(got, want)):
        assert gl.dtype == np.int32 and gv.dtype == np.float64 and gl.shape == wl.shape and gl.flags.c_contiguous, b
        assert np.array_equal(gl, wl) and np.array_equal(bits(gv), bits(wv)) and (gm, gn) == (wm, wn), b
        last = np.flatnonzero(np.diff(np.append(gl[:, 0], gn)))  # the last stored entry of every row
        assert np.array_equal(gl[last], np.stack([np.arange(gn), gm + np.arange(gn)], axis=1)), b
        assert gl.shape[0] == probs[b][0].shape[0] + gn
    assert [(m, n) for _, _, m, n in got][3] == ((0, 3) if with_sizes else (0, 0))  # the problem without an entry
    assert got[2][0][:, 1].tolist().count(2) == 2  # duplicates are kept
    if with_sizes:
        assert [n for _, _, _, n in got] == [4, 9, 6, 3, 6] and got[4][2] < got[4][3]  # sizes[:, 0] is not read; n_b > m_b
    with pytest.raises(ValueError, match="outside must"):
        sparse_to_augmented(loc, val, off, sz, np.zeros(B + 1))
    with pytest.raises(ValueError, match="rows must ascend"):
        sparse_to_augmented(loc[::-1], val, off, sz)


@pytest.mark.parametrize("form", ["scalar", "per_problem", "per_row"])
def test_one_definition_for_the_sparse_and_the_ell_layout(form):
    """The same problems as packed loc / val with sizes and as an ELL stack padded with holes: identical augmented
    problems, so the two outside modes share one definition."""
    probs, sizes = _batch()
    rng = np.random.default_rng(11)
    for k in range(6):  # ragged draws with rows without entries
        n = int(rng.integers(1, 12))
        probs.append(fxt.ragged(rng, rng.integers(0, 5, n), 6, "ints"))
        sizes = np.concatenate([sizes, [[0, n + int(rng.integers(0, 3))]]])
    ns = [int(s[1]) for s in sizes]
    B, N = len(probs), max(ns)
    outside = {"scalar": 1.5, "per_problem": rng.uniform(0, 10, B), "per_row": rng.uniform(0, 10, (B, N))}[form]
    cols, vals, rows = fxt.to_ell(probs, ns, N)
    assert (cols < 0).any() and cols.shape[2] >= 3
    packed = ell_to_packed(cols, vals, rows, outside=outside)
    for b, ((sl, sv, m, n), (el, ev)) in enumerate(zip(sparse_to_augmented(*fxt.pack(probs), sizes, outside), packed)):
        assert np.array_equal(sl, el) and np.array_equal(bits(sv), bits(ev)) and n == ns[b], b


# ---- the front end: checks before the FFI, and the resolution of `fast`

class _NoFFI(Exception):
    pass


@pytest.fixture
def no_ffi(monkeypatch):
    def no_load():
        raise _NoFFI()
    monkeypatch.setattr(_lib, "load", no_load)


class _FakeDeviceTensor:
    is_cuda = True

    def data_ptr(self):
        return 0


LOC = np.array([[0, 1], [0, 0], [2, 1], [0, 0], [1, 2]], dtype=np.int32)
VAL = np.arange(5, dtype=np.float64)
OFF = np.array([0, 3, 5])  # problem 0: rows 0 and 2 (row 1 without an entry); problem 1: rows 0, 1


def test_outside_and_dims_are_checked_before_the_ffi(no_ffi):
    f = auction_solve_sparse_batch
    for bad in (float("nan"), float("inf"), -np.inf, np.float64("nan")):
        with pytest.raises(ValueError, match="outside must be finite"):
            f(LOC, VAL, OFF, outside=bad)
    for bad in (np.zeros(2, dtype=np.float32), np.zeros((2, 3), dtype=np.int64)):
        with pytest.raises(ValueError, match="outside must be float64"):
            f(LOC, VAL, OFF, outside=bad)
    for bad in (np.zeros(3), np.zeros((3, 3)), np.zeros((2, 3, 1)), np.zeros(()), np.zeros((2, 0))):
        with pytest.raises(ValueError, match="outside must have shape"):
            f(LOC, VAL, OFF, outside=bad)
    with pytest.raises(ValueError, match="P >= Nmax = 3"):  # (Nmax from the data ...
        f(LOC, VAL, OFF, outside=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="P >= Nmax = 5"):  # ... from sizes ...
        f(LOC, VAL, OFF, outside=np.zeros((2, 4)), sizes=[[0, 5], [0, 2]])
    with pytest.raises(ValueError, match="P >= Nmax = 8"):  # ... or from dims)
        f(LOC, VAL, OFF, outside=np.zeros((2, 7)), dims=(8, 4))
    with pytest.raises(TypeError, match="outside on the device"):  # a device tensor with host input: the wrong side
        f(LOC, VAL, OFF, outside=_FakeDeviceTensor())
    for bad in ("1.0", [1.0, 2.0], object(), True):
        with pytest.raises(TypeError, match="outside must be a float"):
            f(LOC, VAL, OFF, outside=bad)
    for bad in ((0, 4), (4, 2049), (4,), "ab", (2.5, 4)):
        for errors in ("raise", "status"):
            with pytest.raises(ValueError, match="dims must be"):
                f(LOC, VAL, OFF, outside=1.0, dims=bad, errors=errors)
    with pytest.raises(ValueError, match="dims is taken with errors='status' only"):  # without outside: as it was
        f(LOC, VAL, OFF, dims=(4, 4))
    # what belongs to one problem or one row does not raise, negative values are values: the library is reached
    for ok in (0.0, -3, np.float32(1.5), np.array([-1.0, np.nan]), np.full((2, 3), np.inf), np.zeros((2, 9))):
        for errors in ("raise", "status"):
            with pytest.raises(_NoFFI):
                f(LOC, VAL, OFF, outside=ok, errors=errors, dims=(3, 3))


class _Recorder:
    """Stands in for the library: records what the front end passes and fills nothing."""
    AT = {"misslap_solve_sparse_batch": (None, 9), "misslap_solve_sparse_batch_status": (6, 10),
          "misslap_solve_sparse_batch_outside": (6, 9)}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in self.AT:
            raise AttributeError(name)
        fast_at, opts_at = self.AT[name]

        def call(*args):
            opts = args[opts_at]._obj
            c = dict(name=name, fast=None if fast_at is None else args[fast_at], eps_start=opts.eps_start,
                     maximize=opts.maximize, max_iter=opts.max_iter, args=args)
            if name == "misslap_solve_sparse_batch":  # eps_start per problem: NULL, or 1 / N_b of `fast`
                c["eps_b"] = None if args[5] is None else np.ctypeslib.as_array(C.cast(args[5], C.POINTER(C.c_float)), (2,)).copy()
            self.calls.append(c)
            raise _NoFFI()
        return call


def _record(monkeypatch, **kw):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    with pytest.raises(_NoFFI):
        auction_solve_sparse_batch(LOC, VAL, OFF, **kw)
    (call,) = rec.calls
    return call


def test_fast_is_resolved_in_the_front_end(monkeypatch):
    # without outside: today's calls and today's arguments, whether fast is left alone, None or given
    for kw, eps in ((dict(), None), (dict(fast=None), None), (dict(fast=False), None), (dict(fast=True), [0.5, 1.0]),
                    (dict(eps_start=0.5), None)):
        c = _record(monkeypatch, **kw)
        assert c["name"] == "misslap_solve_sparse_batch" and c["eps_start"] == kw.get("eps_start", 0.0), kw
        assert (c["eps_b"] is None) if eps is None else np.array_equal(c["eps_b"], np.float32(eps)), kw
        assert c["args"][8] == 1 and c["args"][4] is None and c["max_iter"] == 1000000 and c["maximize"] == 0
    for kw, fast in ((dict(), 0), (dict(fast=None), 0), (dict(fast=False), 0), (dict(fast=True), 1)):
        c = _record(monkeypatch, errors="status", cardinality_check=False, **kw)
        assert (c["name"], c["fast"], c["args"][9]) == ("misslap_solve_sparse_batch_status", fast, 0), kw
        assert c["args"][14:16] == (3, 3)  # Nmax, Mmax from the data
    # with outside: a single phase unless eps_start > 0 was given; explicit settings pass through
    for kw, fast, eps in ((dict(), 1, 0.0), (dict(eps_start=0.5), 0, 0.5), (dict(eps_start=1e-3), 0, float(np.float32(1e-3))),
                          (dict(fast=False), 0, 0.0), (dict(fast=True, eps_start=0.5), 1, 0.5), (dict(fast=True), 1, 0.0),
                          (dict(eps_start=0.0), 1, 0.0), (dict(fast=None), 1, 0.0)):
        for errors in ("raise", "status"):
            c = _record(monkeypatch, outside=1.0, problem="max", errors=errors, **kw)
            assert (c["name"], c["fast"], c["eps_start"]) == ("misslap_solve_sparse_batch_outside", fast, eps), kw
            assert c["maximize"] == 1 and c["args"][13:15] == (3, 3)
    # Nmax: the largest of the stored rows and of sizes[:, 1]; Mmax: the real columns; dims as given
    assert _record(monkeypatch, outside=1.0, sizes=[[9, 2], [9, 7]])["args"][13:15] == (7, 3)
    assert _record(monkeypatch, outside=1.0, sizes=[[9, 3], [9, 2]], dims=(40, 50))["args"][13:15] == (40, 50)
    # the scalar and (B,) travel as one value per problem (outside_ld = 0), (B, P) with outside_ld = P
    assert _record(monkeypatch, outside=2.0)["args"][16] == 0
    assert _record(monkeypatch, outside=np.array([1.0, 2.0]))["args"][16] == 0
    assert _record(monkeypatch, outside=np.ones((2, 5)))["args"][16] == 5


# ---- the C entry point and the workspace

def test_workspace_bytes_needs_no_gpu(built_lib):
    f = built_lib.misslap_sparse_batch_outside_workspace_bytes
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for B, N, M in ((1, 1, 1), (2, 7, 5), (64, cap, cap), (100000, 256, 40), (2**31 - 1, 1, 1)):
        a, b = f(B, N, M, 0), f(B, N, M, 1)
        assert a > 0 and a % 256 == 0 and b % 256 == 0, (B, N, M)
        assert b >= a + 8 * B * (M + N)  # the staged starting prices of the augmented problems
        assert a == f(B, N, 1, 0)        # without prices the bound on the columns costs nothing
        assert a >= 32 * B + 4 * B * (N + 1)  # a check record and Nmax + 1 row starts per problem
    for bad in ((0, 4, 4), (2**31, 4, 4), (1, 0, 4), (1, cap + 1, 4), (1, 4, 0), (1, 4, cap + 1), (1, 4, -1), (-1, 4, 4)):
        assert f(*bad, 1) == -1, bad


def test_c_entry_point_validates_then_needs_a_device(built_lib):
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.max_iter = 10
    loc = np.array([[0, 1], [2, 0]], dtype=np.int32)
    val = np.array([1.0, 2.0])
    off = np.array([0, 2], dtype=np.int64)
    outside = np.array([[4.0, 5.0, 6.0, 7.0]])
    sol, status = np.empty((1, 3), dtype=np.int32), np.empty(1, dtype=np.int32)
    oprices = np.empty((1, 3))
    metas = (_lib.DenseBatchMeta * 1)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)

    def call(B=1, Nmax=3, Mmax=2, opts=o, st=status.ctypes.data, work=None, nwork=0, on_dev=0, out=outside.ctypes.data,
             ld=0, prices=None, p_ld=0, offsets=off.ctypes.data, off_dev=None, lo=loc.ctypes.data):
        return built_lib.misslap_solve_sparse_batch_outside(
            B, lo, val.ctypes.data, offsets, off_dev, None, 1, prices, p_ld, C.byref(opts), None, work, nwork, Nmax, Mmax,
            out, ld, sol.ctypes.data, None, oprices.ctypes.data, on_dev, st, None, C.cast(metas, C.c_void_p), None)

    err = built_lib.misslap_last_error
    cap = _lib.SPARSE_BATCH_MAX_DIM
    for ld in (1, 2, -1, -2048):  # outside_ld: 0 or >= Nmax
        assert call(ld=ld) == _lib.ERR_INVALID and b"outside_ld" in err(), ld
    assert call(out=None) == _lib.ERR_INVALID and b"outside" in err()
    assert call(lo=None) == _lib.ERR_INVALID and b"null loc" in err()
    assert call(offsets=None) == _lib.ERR_INVALID and b"offsets" in err()
    assert call(Nmax=cap + 1) == _lib.ERR_INVALID and b"MISSLAP_SPARSE_BATCH_MAX_DIM" in err()
    assert call(Mmax=cap + 1) == _lib.ERR_INVALID and call(Mmax=0) == _lib.ERR_INVALID and call(Nmax=0) == _lib.ERR_INVALID
    assert call(B=0) == _lib.ERR_INVALID
    assert call(st=None) == _lib.ERR_INVALID and b"status" in err()
    assert call(prices=val.ctypes.data, p_ld=0) == _lib.ERR_INVALID and b"prices_ld" in err()
    bad = _lib.Options()
    C.memmove(C.byref(bad), C.byref(o), C.sizeof(o))
    bad.tail_threshold = 5
    assert call(opts=bad) == _lib.ERR_INVALID and b"misslap_solve_sparse_batch_outside takes" in err()
    need = built_lib.misslap_sparse_batch_outside_workspace_bytes(1, 3, 2, 0)
    dev = _lib.Options()
    C.memmove(C.byref(dev), C.byref(o), C.sizeof(o))
    dev.input_on_device = 1
    assert call(work=4096, nwork=need, on_dev=1) == _lib.ERR_INVALID and b"on the device" in err()
    assert call(work=4096, nwork=need, on_dev=1, opts=dev) == _lib.ERR_INVALID and b"device copy of offsets" in err()
    assert call(work=4096, nwork=need - 1, on_dev=1, opts=dev, off_dev=off.ctypes.data) == _lib.ERR_INVALID
    assert b"misslap_sparse_batch_outside_workspace_bytes" in err()
    assert call(work=4096 + 8, nwork=need, on_dev=1, opts=dev, off_dev=off.ctypes.data) == _lib.ERR_INVALID  # misaligned
    for ld in (0, 3, 4):  # valid host arguments: only the GPU can be missing
        rc = call(ld=ld)
        assert rc in (0, _lib.ERR_NO_DEVICE), err()
        if rc:
            assert b"no CPU fallback" in err()


# ---- the order of the verdict

def test_verdict_order_is_pinned():
    """Problems with two or more defects each: the restatement (tests/_sparse_outside_fixture.expected_status, which the GPU
    tests hold the kernels to) reports the earlier check of the documented order 8, 10, 11, 7, 3, 13, 14, 5, 6."""
    dims, nan = (4, 3), np.nan
    order = [fxt.NO_ENTRIES, fxt.NEGATIVE_INDEX, fxt.ROWS_UNSORTED, fxt.BAD_SHAPE, fxt.INFINITE_VALUE, fxt.TOO_LARGE,
             fxt.PRICES_TOO_NARROW, fxt.PRICE_NOT_FINITE, fxt.PRICE_NEGATIVE]
    assert order == [8, 10, 11, 7, 3, 13, 14, 5, 6]
    # each problem: (entries (i, j, v), sizes n or None, outside row, prices row) -> the code
    cases = [
        ([], None, [nan] * 4, [nan, nan], 8),                                  # nothing else is looked at
        ([(1, 0, 1.0), (0, -1, nan)], 0, [nan] * 4, [nan, nan], 10),           # before unsorted, bad shape, NaN
        ([(1, 0, nan), (0, 0, 1.0)], 0, [1.0] * 4, [0.0, 0.0], 11),            # before bad shape and NaN
        ([(0, 0, nan), (2, 9, 1.0)], 2, [1.0] * 4, [0.0, 0.0], 7),             # before NaN and too large
        ([], 0, [1.0] * 4, [0.0, 0.0], 7),                                     # no entries, sizes name no row
        ([(0, 9, 1.0)], 9, [1.0, 1.0, 1.0, nan], [0.0, 0.0], 3),               # an outside value, before too large
        ([(0, 9, np.inf)], 1, [1.0] * 4, [0.0, 0.0], 3),                       # a value, before too large
        ([(0, 2, 1.0)], 5, [1.0] * 4, [nan, -1.0], 13),                        # rows; before narrow prices
        ([(0, 3, 1.0)], 1, [1.0, nan, nan, nan], [nan, -1.0], 13),             # columns; outside beyond n_b is not read
        ([(0, 2, 1.0)], 1, [1.0] * 4, [nan, -1.0], 14),                        # before the prices' values
        ([(0, 1, 1.0)], 1, [1.0] * 4, [-1.0, nan], 5),                         # NaN before negative
        ([(0, 1, 1.0)], 1, [1.0] * 4, [1.0, -0.0], 6),
        ([(0, 0, 1.0)], 4, [-1.0] * 4, [0.0, nan], 0),                         # a price beyond m_b is not the problem's
        ([], 3, [-1.0] * 4, [nan, nan], 0),                                    # no entries, rows named: solved
    ]
    for with_sizes in (True, False):
        use = [c for c in cases if (c[1] is not None) == with_sizes]
        loc = np.array([(i, j) for c in use for i, j, _ in c[0]], dtype=np.int32).reshape(-1, 2)
        val = np.array([v for c in use for _, _, v in c[0]], dtype=np.float64)
        off = np.concatenate([[0], np.cumsum([len(c[0]) for c in use])])
        sizes = np.array([[0, c[1]] for c in use]) if with_sizes else None
        outside, prices = np.array([c[2] for c in use]), np.array([c[3] for c in use])
        status, counts = fxt.expected_status(loc, val, off, sizes, outside, dims, prices)
        assert status.tolist() == [c[4] for c in use]
        for b, c in enumerate(use):  # the record's counts are defined behind 3, 13, 14, 5, 6 (and 0) only
            assert (counts[b] != 0).any() == (c[4] in (0, 3, 13, 14, 5, 6)), b
    # and the mixed batches of the GPU tests hold every code next to healthy problems
    for with_sizes in (True, False):
        fx = fxt.mixed(with_sizes)
        status, _ = fxt.expected_status(fx["loc"], fx["val"], fx["offsets"], fx["sizes"], fx["outside"], fxt.V_DIMS, fx["prices"])
        assert np.array_equal(status, fx["kinds"]) and (status[::2] == 0).all() and (status[1::2] != 0).sum() >= 15


# ---- the definition is optimal under the default the front end chooses

DRAWS = 480


def _draw(rng, t):
    n, m = (int(x) for x in (rng.integers(1, 45), rng.integers(1, 45)))
    lens = rng.integers(0, min(m, 8) + 1, n)
    lens[rng.random(n) < 0.25] = 0  # rows without any entry
    loc, _ = fxt.ragged(rng, lens, m, "ints")
    val = rng.integers(0, 20, loc.shape[0]).astype(np.float64)
    outside = rng.integers(0, 20, n).astype(np.float64) if rng.random() < 0.5 else float(rng.integers(0, 20))
    return n, loc, val, outside, ("min", "max")[t % 2]


def test_single_phase_on_the_augmented_problem_is_optimal():
    """480 gapped draws (n, m < 45, integer values, so eps = 1 / n < the gap between two objectives): the oracle with
    fast=True on sparse_to_augmented's problem reports eCE = 1 and its objective is linear_sum_assignment's on the
    augmented matrix, missing entries at +-1e6, within 1e-9.  Every draw counts."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(1)
    seen = dict(min=0, max=0, unmatched=0, matched=0, tall=0, empty_rows=0)
    for t in range(DRAWS):
        n, loc, val, outside, problem = _draw(rng, t)
        (lo, va, m, nb), = sparse_to_augmented(loc, val, [0, len(val)], [[0, n]], outside if np.ndim(outside) == 0 else outside[None])
        assert nb == n and lo.shape[0] == loc.shape[0] + n
        res = orc.auction_solve(loc=lo, val=va.copy(), size=(m + n, n), problem=problem, fast=True, cardinality_check=False)
        assert res["meta"]["eCE"] == 1, t
        sol = np.asarray(res["sol"])
        assert (sol >= 0).all() and len(set(sol.tolist())) == n, t
        full = np.full((n, m + n), 1e6 if problem == "min" else -1e6)
        for (i, j), v in zip(lo, va):  # (a row's columns are distinct: no entry is stored twice)
            full[i, j] = v
        ri, ci = lsa(full, maximize=problem == "max")
        best = float(full[ri, ci].sum())
        assert abs(res["extra"]["obj_f64"] - best) <= 1e-9, (t, problem, res["extra"]["obj_f64"], best)
        seen[problem] += 1
        seen["unmatched"] += int((sol >= m).sum())
        seen["matched"] += int((sol < m).sum())
        seen["tall"] += n > m
        seen["empty_rows"] += int(n - len(np.unique(loc[:, 0])))
    assert seen["min"] == seen["max"] == DRAWS // 2 and DRAWS >= 400
    assert min(seen["unmatched"], seen["matched"], seen["tall"], seen["empty_rows"]) > 0
