"""Warm-started re-solve on the GPU (misslap_resolve / misslap_update_values / misslap_update_dense) against the oracle
started from the same prices: the reference's solve loop (auction_.pyx:268-306) with `self.p` set to the starting prices
instead of zeros (:220), every person unassigned, its = nreductions = 0 and eps0 = eps_start or C / 2 of the current
values.  Everything bit for bit: sol, its, nreductions, final eps, obj_f64 and the final prices."""
import zlib

import numpy as np
import pytest

import cases
from oracle import oracle as orc
from sslap_amd import from_matrix, from_sparse, synth

pytestmark = pytest.mark.gpu

SPARSE = dict(kind="sparse", n=3000, m=12000, density=0.003)
# name -> (input spec, solver options); the tile-major formats 2 / 3 need rows whose columns are not ascending
CONFIGS = {
    "tail_only": (dict(kind="sparse", n=400, m=400, density=0.05), dict(tail_threshold=512)),
    "wave_lines": (SPARSE, dict(tiled_min_k=-1)),
    "wave_nolines": (SPARSE, dict(tiled_min_k=-1, cand=0)),
    "tiled_fmt0": (SPARSE, dict(tiled_min_k=1, engine=1)),
    "tiled_fmt1": (SPARSE, dict(tiled_min_k=1, engine=1, force_f64=True)),
    "tiled_fmt2": (dict(SPARSE, kind="shuffled"), dict(tiled_min_k=1, engine=1)),
    "tiled_fmt3": (dict(SPARSE, kind="shuffled"), dict(tiled_min_k=1, engine=1, force_f64=True)),
}
FMT = {"tiled_fmt0": 0, "tiled_fmt1": 1, "tiled_fmt2": 2, "tiled_fmt3": 3}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle(o, p0):
    """Solve an OracleSolver from starting prices p0 (written into its live price array before solve())."""
    pv = np.ctypeslib.as_array(orc.lib().oracle_prices(o._h), (o.M,))
    pv[:] = p0
    sol = o.solve()
    return sol, o.state()["p"]


def _oracle_sparse(loc, val, problem, p0, eps_start=0.0):
    o = orc.OracleSolver(loc, val.copy(), problem=problem, eps_start=eps_start)  # (the oracle negates 'min' in place)
    return _oracle(o, p0) + (o,)


def _same(g, sol_g, sol_o, p_o, o):
    """GPU solver `g` after resolve() vs an oracle result."""
    assert np.array_equal(sol_g, sol_o)
    assert g.meta["its"] == o.meta["its"] and g.meta["nreductions"] == o.meta["nreductions"]
    assert g.gpu["final_eps_f32"] == o.extra["final_eps_f32"] and g.gpu["start_eps_f32"] == o.extra["start_eps_f32"]
    assert g.gpu["obj_f64"] == o.extra["obj_f64"]
    assert g.meta["eCE"] == o.meta["eCE"] and g.meta["soln_found"] == o.meta["soln_found"]
    assert np.array_equal(_bits(g.prices), _bits(p_o))
    assert g.status().error_bits == 0


def _same_gpu(a, sol_a, b, sol_b):
    assert np.array_equal(sol_a, sol_b)
    for k in ("its", "nreductions", "eCE", "soln_found", "obj", "final_eps", "start_eps"):
        assert a.meta[k] == b.meta[k], k
    assert a.gpu["obj_f64"] == b.gpu["obj_f64"]
    assert np.array_equal(_bits(a.prices), _bits(b.prices))


def _perturb(val, rng, f64, frac=0.05, step=1.0):
    """A copy of val with `frac` of the entries moved by +-step (kept fp32-exact unless f64)."""
    out = val.copy()
    idx = rng.choice(val.size, max(1, int(frac * val.size)), replace=False)
    out[idx] += rng.choice([-step, step], idx.size) * (1.0 + (rng.random(idx.size) * 0.37 if f64 else 0.0))
    return out if f64 else out.astype(np.float32).astype(np.float64)


def _solver(loc, val, problem, kw):
    return from_sparse(loc, val.copy(), problem=problem, cardinality_check=False, **kw)


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_resolve_from_zero_prices_equals_solve(name, problem, gpu_lib):
    spec, kw = CONFIGS[name]
    loc, val = cases.synth_inputs(spec)
    a = _solver(loc, val, problem, kw)
    sol_a = a.solve()
    b = _solver(loc, val, problem, kw)
    sol_b = b.resolve(prices=np.zeros(b.num_cols))
    _same_gpu(a, sol_a, b, sol_b)
    if name in FMT:
        assert b.gpu["tiled_active"] == 1 and b.gpu["tiled_format"] == FMT[name]


@pytest.mark.parametrize("start", ["random", "perturbed", "lower"])
@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_warm_start_matches_the_oracle(name, problem, start, gpu_lib):
    spec, kw = CONFIGS[name]
    loc, val = cases.synth_inputs(spec)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{problem}/{start}".encode()))
    g = _solver(loc, val, problem, kw)
    f64 = bool(kw.get("force_f64"))
    if start == "random":
        p0, eps = rng.uniform(0.0, 60.0, g.num_cols), 0.0
    elif start == "perturbed":  # the final prices of a nearby problem
        other = _solver(loc, _perturb(val, rng, f64), problem, kw)
        other.solve()
        p0, eps = other.prices, 1.0
    else:  # prices below the handle's current ones, after a solve on the same handle (its lines were built above them)
        g.solve()
        p0, eps = g.prices * 0.5, 0.5
    sol_g = g.resolve(prices=p0, eps_start=eps)
    sol_o, p_o, o = _oracle_sparse(loc, val, problem, p0, eps)
    _same(g, sol_g, sol_o, p_o, o)
    if name in FMT:
        assert g.gpu["tiled_format"] == FMT[name]


def _dense(rng, n=300, m=420, valid=0.6):
    mat = rng.uniform(0.0, 100.0, (n, m)).astype(np.float32).astype(np.float64)
    mat[rng.random((n, m)) >= valid] = -1.0
    mat[np.arange(n), rng.integers(0, m, n)] = 50.0  # every row has an entry
    return mat


@pytest.mark.parametrize("problem", ["min", "max"])
def test_dense_handle_warm_start_and_update(problem, gpu_lib):
    rng = np.random.default_rng(7 if problem == "min" else 8)
    A = _dense(rng)
    g = from_matrix(A.copy(), problem=problem, cardinality_check=False)
    g.solve()
    pA = g.prices
    # warm start from lower prices on the same handle
    sol = g.resolve(prices=pA * 0.5, eps_start=0.5)
    o = orc.from_matrix(A.copy(), problem=problem, eps_start=0.5)
    sol_o, p_o = _oracle(o, pA * 0.5)
    _same(g, sol, sol_o, p_o, o)
    # new values with the same pattern
    B = A.copy()
    ok = B >= 0
    B[ok] = np.abs(B[ok] + rng.choice([-1.0, 0.0, 0.0, 2.0], ok.sum())).astype(np.float32)  # (fp32-exact)
    delta = g.update_values(B)
    assert delta == np.abs(B[ok] - A[ok]).max()
    sol = g.resolve(prices=pA, eps_start=delta)
    o = orc.from_matrix(B.copy(), problem=problem, eps_start=delta)
    sol_o, p_o = _oracle(o, pA)
    _same(g, sol, sol_o, p_o, o)
    fresh = from_matrix(B.copy(), problem=problem, cardinality_check=False)
    _same_gpu(g, sol, fresh, fresh.resolve(prices=pA, eps_start=delta))


@pytest.mark.parametrize("problem", ["min", "max"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_update_values_then_resolve(name, problem, gpu_lib):
    """update_values(B) + resolve(prices=pA) == the oracle on B started from pA == a fresh handle on B resolved from pA."""
    spec, kw = CONFIGS[name]
    loc, A = cases.synth_inputs(spec)
    rng = np.random.default_rng(11)
    f64 = bool(kw.get("force_f64"))
    B = _perturb(A, rng, f64, frac=0.1, step=5.0)
    g = _solver(loc, A, problem, kw)
    g.solve()
    pA = g.prices
    Bc = B.copy()
    delta = g.update_values(Bc)
    assert np.array_equal(_bits(Bc), _bits(B))  # the caller's buffer is not written
    assert delta == np.abs(B - A).max()
    sol = g.resolve(prices=pA, eps_start=delta)
    sol_o, p_o, o = _oracle_sparse(loc, B, problem, pA, delta)
    _same(g, sol, sol_o, p_o, o)
    fresh = _solver(loc, B, problem, kw)
    _same_gpu(g, sol, fresh, fresh.resolve(prices=pA, eps_start=delta))
    # update + plain solve() on a handle nothing has run on == a cold solve of the new values
    h = _solver(loc, A, problem, kw)
    h.update_values(B)
    cold = _solver(loc, B, problem, kw)
    _same_gpu(h, h.solve(), cold, cold.solve())


def test_rejected_updates_leave_the_handle_unchanged(gpu_lib):
    import torch
    from sslap_amd import _lib
    spec, kw = CONFIGS["tiled_fmt0"]
    loc, A = cases.synth_inputs(spec)
    rng = np.random.default_rng(3)
    g, twin = _solver(loc, A, "max", kw), _solver(loc, A, "max", kw)
    g.solve()
    twin.solve()
    p0 = g.prices
    bad = _perturb(A, rng, False)
    bad[17] = np.nan
    t = torch.tensor(bad, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="NaN"):
        g.update_values_device(t.data_ptr())  # (the device check: the Python one would stop a host array earlier)
    with pytest.raises(ValueError, match="NaN"):
        g.update_values(bad)
    inexact = _perturb(A, rng, False)
    inexact[5] += 1e-9  # not exact in fp32: this handle keeps 8 B/edge fp32 values
    with pytest.raises(ValueError, match="force_f64"):
        g.update_values(inexact)
    with pytest.raises(ValueError):
        g.update_values(A[:-1])
    lib = _lib.load()
    short = np.ascontiguousarray(A[:-1])
    assert lib.misslap_update_values(g._h, short.ctypes.data, short.size, 0, None, None) == _lib.ERR_INVALID
    sol, sol_t = g.resolve(prices=p0 * 0.9, eps_start=0.25), twin.resolve(prices=p0 * 0.9, eps_start=0.25)
    _same_gpu(g, sol, twin, sol_t)
    # dense: a changed pattern
    D = _dense(np.random.default_rng(5))
    d, dtwin = from_matrix(D.copy(), cardinality_check=False), from_matrix(D.copy(), cardinality_check=False)
    X = D.copy()
    X[3, np.flatnonzero(D[3] >= 0)[0]] = -1.0  # one stored entry of row 3 becomes invalid
    with pytest.raises(ValueError, match="pattern"):
        d.update_values(X)
    Y = D.copy()
    Y[4, np.flatnonzero(D[4] < 0)[0]] = 1.0  # one invalid entry of row 4 becomes valid
    with pytest.raises(ValueError, match="pattern"):
        d.update_values(Y)
    _same_gpu(d, d.resolve(eps_start=0.0), dtwin, dtwin.resolve(eps_start=0.0))


def test_bad_prices_raise(gpu_lib):
    from sslap_amd import _lib
    spec, kw = CONFIGS["wave_lines"]
    loc, A = cases.synth_inputs(spec)
    g, twin = _solver(loc, A, "max", kw), _solver(loc, A, "max", kw)
    for bad in (-1.0, np.nan, np.inf, -0.0):
        p = np.ones(g.num_cols)
        p[9] = bad
        with pytest.raises(ValueError):
            g.resolve(prices=p)
        # ... and the device check behind the C entry point, past the Python one
        assert _lib.load().misslap_resolve(g._h, p.ctypes.data, 0, 0.0, None, None) == _lib.ERR_INVALID
    _same_gpu(g, g.resolve(prices=np.full(g.num_cols, 3.0)), twin, twin.resolve(prices=np.full(twin.num_cols, 3.0)))


@pytest.mark.parametrize("name", ["tiled_fmt0", "tiled_fmt3"])
def test_device_pointer_variants(name, gpu_lib):
    import torch
    spec, kw = CONFIGS[name]
    loc, A = cases.synth_inputs(spec)
    B = _perturb(A, np.random.default_rng(9), bool(kw.get("force_f64")))
    h, d = _solver(loc, A, "min", kw), _solver(loc, A, "min", kw)
    h.solve()
    d.solve()
    pA = h.prices
    dh = h.update_values(B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tB = torch.tensor(B, device="cuda")
    dd = d.update_values_device(tB.data_ptr(), input_stream=s.cuda_stream)
    assert dh == dd
    sol_h = h.resolve(prices=pA, eps_start=dh)
    sol_d = d.resolve(prices=torch.tensor(pA, device="cuda"), eps_start=dd)
    _same_gpu(h, sol_h, d, sol_d)
    # dense from a device matrix
    D = _dense(np.random.default_rng(2))
    E = np.where(D >= 0, np.floor(D), D)  # (same pattern, fp32-exact)
    x, y = from_matrix(D.copy(), cardinality_check=False), from_matrix(D.copy(), cardinality_check=False)
    tE = torch.tensor(E, device="cuda")
    torch.cuda.synchronize()
    assert x.update_values(E) == y.update_values_device(tE.data_ptr(), dense=True)
    _same_gpu(x, x.resolve(eps_start=1.0), y, y.resolve(eps_start=1.0))


def test_c2_perturbed_warm_resolve_matches_the_oracle(gpu_lib):
    """One BASELINE-size case: C2, 1 % of the values moved by +-1 (fp32-exact), warm resolve from the cold solve's prices."""
    loc, A = synth.gen_config("C2", seed=1)
    rng = np.random.default_rng(1)
    B = _perturb(A, rng, False, frac=0.01, step=1.0)
    g = from_sparse(loc, A.copy(), problem="max", cardinality_check=False)
    g.solve()
    pA = g.prices
    delta = g.update_values(B)
    sol = g.resolve(prices=pA, eps_start=delta)
    sol_o, p_o, o = _oracle_sparse(loc, B, "max", pA, delta)
    _same(g, sol, sol_o, p_o, o)
