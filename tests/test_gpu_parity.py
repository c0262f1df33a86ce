"""GPU suite: the HIP path (through the C ABI / Python front-end) against the golden vectors captured
from the real reference, against the C oracle round by round, and -- at the BASELINE sizes -- against
sha256 fixtures plus size-independent properties.  Bit-exact: sol, its, nreductions, prices, U-list."""
import numpy as np
import pytest

import cases
import cases as cases_mod
from oracle import oracle as orc
from sslap_amd import AuctionSolver, auction_solve, from_sparse, synth

pytestmark = pytest.mark.gpu

# tail_threshold variants: library default, grid kernels only, tiny tail, widest tail (= the tail workgroup)
THRESHOLDS = [None, 0, 16, 512]


def _solve_gpu(entry, loc, val, spec, kw, monkeypatch, thr):
    if thr is None:
        monkeypatch.delenv("MISSLAP_TAIL_THRESHOLD", raising=False)
    else:
        monkeypatch.setenv("MISSLAP_TAIL_THRESHOLD", str(thr))
    call = cases.call_kwargs(entry, loc, val, spec)
    return auction_solve(cardinality_check=False, **call, **kw), call


@pytest.mark.parametrize("thr", THRESHOLDS)
@pytest.mark.parametrize("name", sorted(cases.SMALL_CASES))
def test_small_cases_match_reference(name, thr, golden_small, monkeypatch, gpu_lib):
    manifest, arrays = golden_small
    spec, kw, entry = cases.SMALL_CASES[name]
    loc, val = cases.synth_inputs(spec)
    res, call = _solve_gpu(entry, loc, val.copy(), spec, kw, monkeypatch, thr)
    g = manifest["cases"][name]
    assert res["sol"].dtype == np.int32
    assert np.array_equal(res["sol"], arrays[name + "/sol"])
    for k in cases.META_KEYS:
        assert res["meta"][k] == g["meta"][k], k
    gpu = res["meta"]["gpu"]
    assert gpu["obj_f64"] == g["obj_f64"]
    assert gpu["edges_scanned"] == g["edges_scanned"]
    if "val" in call:
        assert (not np.array_equal(call["val"], val)) == g["val_mutated"]


def test_demo_cases_match_reference(golden_demo, gpu_lib):
    from scipy.sparse import coo_matrix
    manifest, arrays = golden_demo
    for name, g in manifest["cases"].items():
        mat = arrays[name + "/mat"]
        prob = "min" if name.endswith("_min") else "max"
        if name == "demo_coo_max":
            res = auction_solve(coo_mat=coo_matrix(mat), problem=prob)  # default cardinality_check=True
        else:
            res = auction_solve(mat.copy(), problem=prob)               # positional `mat`, like the examples
        assert np.array_equal(res["sol"], arrays[name + "/sol"]), name
        for k in cases.META_KEYS:
            assert res["meta"][k] == g["meta"][k], (name, k)


@pytest.mark.parametrize("thr", [None, 0])
@pytest.mark.parametrize("name", sorted(cases.TRACE_CASES))
def test_round_trace_matches_reference(name, thr, golden_trace, monkeypatch, gpu_lib):
    manifest, arrays = golden_trace
    spec, kw = cases.TRACE_CASES[name]
    loc, val = cases.synth_inputs(spec)
    want, its = arrays[name + "/p2o"], manifest["cases"][name]["its"]
    for r in range(1, manifest["rounds"] + 1):
        res, _ = _solve_gpu("locval", loc, val.copy(), spec, dict(kw, max_iter=r), monkeypatch, thr)
        assert res["meta"]["its"] == its[r - 1]
        assert np.array_equal(res["sol"], want[r - 1]), f"round {r}"


@pytest.mark.parametrize("thr", [None, 0, 7])
@pytest.mark.parametrize("spec,prob", [
    (dict(kind="sparse", n=300, m=300, density=0.05), "max"),
    (dict(kind="sparse", n=200, m=200, density=0.08, ints=4), "max"),
    (dict(kind="single", n=200, density=0.05, n_single=10), "min"),
    (dict(kind="sparse", n=100, m=150, density=0.1), "max"),
    (dict(kind="f64", n=300, density=0.05), "min"),
])
def test_full_state_vs_oracle_round_by_round(spec, prob, thr, gpu_lib):
    """prices, U-list (order matters: it breaks ties), K, p2o, o2p after r rounds, r = 1..60, against the
    oracle capped at the same r (pins a4-a7 of SURVEY.md section 8 individually)."""
    loc, val = cases.synth_inputs(spec)
    for r in list(range(1, 40)) + [45, 60, 90, 150]:
        o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, tail_threshold=thr)
        g.solve()
        sg = g.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert sg["nreductions"] == so["nreductions"] and np.float32(sg["eps"]) == np.float32(so["eps"]), r


def test_forced_f64_layout_matches(golden_small, gpu_lib):
    """The 12 B/edge kernel instance on fp32-exact data gives the same bits as the 8 B/edge one."""
    manifest, arrays = golden_small
    spec, kw, _ = cases.SMALL_CASES["sq1000_max"]
    loc, val = cases.synth_inputs(spec)
    s = from_sparse(loc, val, cardinality_check=False, force_f64=True, **kw)
    sol = s.solve()
    assert s.gpu["bytes_per_edge"] == 12
    assert np.array_equal(sol, arrays["sq1000_max/sol"])
    assert s.meta["its"] == manifest["cases"]["sq1000_max"]["meta"]["its"]


@pytest.mark.parametrize("name", ["C1", "C1_min", "C4", "C2", "C3", "C5"])
def test_baseline_configs_match_reference_hashes(name, golden_large, gpu_lib):
    g = golden_large["cases"].get(name)
    if g is None:
        pytest.skip(f"{name} fixture not generated")
    spec, kw = cases.LARGE_CASES[name]
    loc, val = _config_arrays(spec["name"])[:2]  # (generated once per session: the sharded tests use the same arrays)
    assert synth.input_digest(loc, val) == g["input_sha256"]
    res = auction_solve(loc=loc, val=val.copy(), cardinality_check=False, **kw)
    sol, meta = res["sol"], res["meta"]
    assert synth.sol_digest(sol) == g["sol_sha256"]
    for k in cases.META_KEYS:
        assert meta[k] == g["meta"][k], k
    assert meta["gpu"]["obj_f64"] == g["obj_f64"]
    assert meta["gpu"]["edges_scanned"] == g["edges_scanned"]
    assert meta["gpu"]["bids_made"] == g["bids_made"]
    # size-independent properties
    n = synth.CONFIGS[spec["name"]]["n_rows"]
    assert len(np.unique(sol)) == n and sol.min() >= 0
    assert meta["eCE"] == 1 and meta["soln_found"] == 1


def test_fullsize_properties_without_fixture(gpu_lib):
    """A BASELINE-sized instance with a seed no fixture covers: permutation, every chosen edge exists,
    eps-complementary slackness at 1/N holds (checked on the host from prices), optimal vs duality gap."""
    loc, val = synth.gen_sparse(50_000, 50_000, 0.005, seed=7)
    s = from_sparse(loc, val.copy(), problem="max", max_iter=10**8, cardinality_check=False)
    sol = s.solve()
    st = s.state()
    n = 50_000
    assert len(np.unique(sol)) == n
    assert s.meta["soln_found"] == 1 and st["K"] == 0
    # chosen edges exist, objective re-derived on the host
    key = loc[:, 0].astype(np.int64) * n + loc[:, 1]
    pick = np.searchsorted(key, np.arange(n, dtype=np.int64) * n + sol)
    assert np.array_equal(key[pick], np.arange(n, dtype=np.int64) * n + sol)
    obj = val[pick].sum()
    assert abs(obj - s.gpu["obj_f64"]) <= 1e-9 * abs(obj)
    # eps-CS: for every edge  (a_ij* - p_j*) + eps >= a_ik - p_k
    p = st["p"]
    v = val - p[loc[:, 1]]
    rowmax = np.maximum.reduceat(v, np.searchsorted(loc[:, 0], np.arange(n)))
    chosen = val[pick] - p[sol]
    assert (chosen + 1.0 / n + 1e-7 >= rowmax).all()
    # weak duality: sum of prices + sum of row maxima bounds the optimum within n * eps
    assert obj >= p.sum() + rowmax.sum() - 1.0 - 1e-6 * abs(obj)


def test_input_contract_errors(gpu_lib):
    loc, val = synth.gen_sparse(50, 50, 0.2, seed=3)
    bad = loc[::-1].copy()
    with pytest.raises(ValueError, match="sorted"):
        from_sparse(bad, val.copy(), cardinality_check=False)
    gap = loc[loc[:, 0] != 7]
    with pytest.raises(ValueError, match="at least one entry"):
        from_sparse(gap, val[loc[:, 0] != 7].copy(), cardinality_check=False)
    with pytest.raises(ValueError, match="Buffer dtype mismatch"):
        from_sparse(loc, val.astype(np.float32), cardinality_check=False)
    with pytest.raises(ValueError, match="Fewer than"):
        auction_solve(mat=np.full((4, 4), -1.0))
    with pytest.raises(ValueError, match="Maximum matching possible only involves 1 out of 2 rows"):
        auction_solve(mat=np.array([[1., -1.], [1., -1.]]))
    with pytest.raises(ValueError, match="One of the following formats"):
        auction_solve()


def test_device_resident_input(gpu_lib):
    """The bench path: COO already in HBM (torch tensors), no host arrays involved."""
    import torch
    loc, val = synth.gen_sparse(2000, 2000, 0.01, seed=1)
    dl = torch.from_numpy(loc).cuda()
    dv = torch.from_numpy(val).cuda()
    s = AuctionSolver.from_device_pointers(dl.data_ptr(), dv.data_ptr(), loc.shape[0], problem="max")
    sol = s.solve()
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False)
    assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
    assert torch.equal(dv.cpu(), torch.from_numpy(val))  # device input untouched


def test_device_resident_input_ordered_behind_the_producer_stream(gpu_lib):
    """options.input_stream: the inputs are still being PRODUCED on a side stream when create is called (a long chain
    of kernels in front of the copies that fill them); the solver's stream waits for an event on that stream instead
    of for the whole device.  Wrong ordering would read zeros (rejected: rows unsorted / empty) or stale values."""
    import torch
    loc, val = synth.gen_sparse(3000, 3000, 0.01, seed=21)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False)
    h_loc, h_val = torch.from_numpy(loc).pin_memory(), torch.from_numpy(val).pin_memory()
    side = torch.cuda.Stream()
    for _ in range(3):
        dl = torch.zeros_like(h_loc, device="cuda")
        dv = torch.zeros_like(h_val, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            x = torch.randn(4096, 4096, device="cuda")
            for _ in range(40):  # ~ tens of milliseconds of work ahead of the copies
                x = x @ x
                x = x / x.norm()
            dl.copy_(h_loc, non_blocking=True)
            dv.copy_(h_val, non_blocking=True)
        s = AuctionSolver.from_device_pointers(dl.data_ptr(), dv.data_ptr(), loc.shape[0], problem="max",
                                               input_stream=side.cuda_stream)
        sol = s.solve()
        assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
    torch.cuda.synchronize()


# (n, density, seed, integer values, tail threshold, shard_min_k): every grid round sharded / a mix of sharded
# and replicated rounds / library default (nothing sharded at this size) / the LDS-tiled kernel sharded
_DIST_GPU_CASES = ((1500, 0.02, 1, 0, 0, -1), (1500, 0.02, 2, 4, 8, 300), (1500, 0.02, 3, 0, None, None),
                   (30000, 0.002, 4, 0, None, None))


def _dist_gpu_worker(rank, world, port, out, transport="staged"):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from sslap_amd import from_sparse, synth
    from sslap_amd.dist import Comm, solve_sharded
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # custom communicator: device buffers staged through the host and reduced with gloo -- or torch.distributed's own
    # all-reduce called on the device buffers on the solver's stream (the transport bench.py falls back to; under the
    # nccl backend that is the RCCL inside torch, here gloo takes the CUDA tensors)
    comm = Comm.gloo_staged() if transport == "staged" else Comm.torch_collectives()
    res = []
    for n, dens, seed, ints, thr, smk in _DIST_GPU_CASES:
        loc, val = synth.gen_sparse(n, n, dens, seed=seed, integer_values=ints)
        s = from_sparse(loc, val, problem="max", cardinality_check=False, shard=(rank, world), tail_threshold=thr,
                        max_iter=10**8, shard_min_k=smk)
        sol = solve_sharded(s, comm)  # misslap_solve_sharded: the loop and the exchange calls are the library's
        res.append((sol.tolist(), s.meta["its"], s.meta["nreductions"], s.gpu["obj_f64"],
                    s.gpu["edges_scanned"], s.gpu["shard_edges"]))
    out.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("transport", ["staged", "torch"])
def test_sharded_driver_two_ranks_one_gpu(transport, gpu_lib):
    """The real kernels behind the library's sharded solve (misslap_solve_sharded): two processes share cuda:0 and
    exchange the best-bid buffers through a custom communicator (gloo, staged through the host -- or handed the device
    buffers directly, Comm.torch_collectives; RCCL needs one GPU per rank -- its world-1 smoke test is below).  Shard ranges, exchange on the solver's stream, replicated apply
    and the replicated tail must reproduce the single-GPU / oracle result."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_gpu_worker, args=(r, 2, port, q, transport)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for k, (n, dens, seed, ints, thr, smk) in enumerate(_DIST_GPU_CASES):
        loc, val = synth.gen_sparse(n, n, dens, seed=seed, integer_values=ints)
        ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
        one = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8, tail_threshold=thr)
        one.solve()
        for rank in (0, 1):
            sol, its, nred, obj, edges, sh = got[rank][k]
            assert sol == ref["sol"].tolist(), (rank, k)
            assert (its, nred, obj) == (ref["meta"]["its"], ref["meta"]["nreductions"], ref["extra"]["obj_f64"])
        # unique work: the sharded parts of the two ranks add up, the replicated part is the same on both
        (e0, s0), (e1, s1) = got[0][k][4:], got[1][k][4:]
        assert e0 - s0 == e1 - s1
        assert s0 + s1 + (e0 - s0) == one.gpu["edges_scanned"]
        if smk is not None or n >= 30000:
            assert s0 > 0 and s1 > 0
        else:
            assert s0 == 0 and s1 == 0


@pytest.mark.parametrize("spec,prob", [
    (dict(kind="sparse", n=6000, m=40000, density=0.001), "max"),          # 3 column tiles, rectangular
    (dict(kind="sparse", n=5000, m=5000, density=0.01, ints=6), "max"),    # heavy ties, 1 tile
    (dict(kind="sparse", n=4500, m=33000, density=0.0012, ints=3), "min"), # ties across tiles
])
@pytest.mark.parametrize("engine", [1])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_tiled_bid_kernel_round_by_round(spec, prob, engine, fmt, gpu_lib):
    """The full-scan engine k_bid_tiled (prices tiled in LDS, tile loop) forced for every grid round
    (tiled_min_k = 1, no tail kernel): full state vs the oracle after r rounds -- in each record format of the
    tile-major copy: 0 = 6 B/edge (fp32-exact values), 1 = 10 B/edge (fp64 values: the 12 B/edge layout forced), 2 / 3 =
    the same with the stored index carried, on rows whose stored order is a random permutation (the reference takes the
    stored order, auction_.pyx:343-357, and its in-row tie rule is 'the last stored index wins', :351)."""
    loc, val = cases.synth_inputs(dict(spec, kind="shuffled") if fmt >= 2 else spec)
    for r in [1, 2, 3, 5, 8, 13, 21, 40, 80, 200]:
        o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, tail_threshold=0,
                        tiled_min_k=1, engine=engine, force_f64=bool(fmt & 1))
        g.solve()
        assert g.gpu["tiled_active"] == engine and g.gpu["tiled_format"] == fmt
        sg = g.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], r


def test_tiled_and_gather_kernels_agree_end_to_end(gpu_lib):
    loc, val = synth.gen_sparse(20000, 50000, 0.001, seed=4)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    for tk, eng in ((1, 1), (0, 0), (-1, 0)):  # always tiled / default / gather only
        s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8, tiled_min_k=tk,
                        engine=eng)
        sol = s.solve()
        assert s.gpu["tiled_active"] == (0 if tk < 0 else (eng or 1))
        assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"], tk
        assert s.gpu["obj_f64"] == ref["extra"]["obj_f64"]


@pytest.mark.parametrize("ints", [0, 3])
def test_unsorted_rows_run_on_the_full_scan_engine(ints, gpu_lib):
    """Rows whose columns are not ascending (legal in the reference) keep the full-scan engine and its eCE pass: the
    tile-major copy carries every edge's stored index (formats 2 / 3), and equal values are ordered by it.  With integer
    costs (ties in nearly every row) the result depends on that order."""
    spec = dict(kind="shuffled", n=5000, m=20000, density=0.002, ints=ints)
    loc, val = cases.synth_inputs(spec)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False)
    for f64 in (False, True):
        s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, tiled_min_k=1, force_f64=f64)
        sol = s.solve()
        assert s.gpu["tiled_active"] == 1 and s.gpu["tiled_format"] == (3 if f64 else 2)
        assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
        assert s.gpu["obj_f64"] == ref["extra"]["obj_f64"] and s.meta["eCE"] == ref["meta"]["eCE"]
    if ints:  # the stored order matters here: the column-sorted version of the same instance has another solution
        loc2, val2 = cases.synth_inputs(dict(spec, kind="sparse"))
        ref2 = orc.auction_solve(loc=loc2, val=val2.copy(), problem="max", cardinality_check=False)
        assert not np.array_equal(ref2["sol"], ref["sol"])


def test_integration_md_binding_stub_works(gpu_lib):
    """The reference-side ctypes binding printed in INTEGRATION.md (what a maintainer of the reference would
    add) is executed verbatim against the built library."""
    import os
    import re
    from sslap_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(# sslap/misslap_binding.py.*?)```", text, re.S).group(1)
    code = code.replace('C.CDLL("libmisslap.so")', f'C.CDLL({_lib.LIB_PATH!r})')
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    loc, val = synth.gen_sparse(800, 800, 0.03, seed=9)
    for prob in ("max", "min"):
        solver = ns["_from_sparse"](loc, val.copy(), problem=prob, cardinality_check=False)
        sol = solver.solve()
        ref = orc.auction_solve(loc=loc, val=val.copy(), problem=prob, cardinality_check=False)
        assert np.array_equal(sol, ref["sol"])
        for k in ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj", "final_eps", "start_eps"):
            assert solver.meta[k] == ref["meta"][k], k


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_random_instances_vs_oracle(seed, gpu_lib):
    """Random shapes / densities / value kinds / problems / thresholds / engines: sol, its, nreductions, objective
    and the scanned-edge count against the C oracle.  Sizes chosen so that the tile-major engine (several
    tiles, partial rounds), k_round_small, the large-round kernels and both tail paths all occur."""
    r = np.random.default_rng(1000 + seed)
    n = int(r.choice([90, 700, 2500, 9000, 20000]))
    m = n if r.random() < 0.6 else int(n * r.uniform(1.05, 2.0))
    density = float(r.choice([3.0, 8.0, 30.0])) / m
    ints = int(r.choice([0, 0, 2, 7]))
    prob = "max" if r.random() < 0.6 else "min"
    loc, val = synth.gen_sparse(n, m, density, seed=50 + seed, integer_values=ints)
    kw = dict(problem=prob, cardinality_check=False, max_iter=int(r.choice([10**8, 10**8, 500, 37])))
    gpu = dict(tail_threshold=[None, 0, 5, 300][seed % 4], tiled_min_k=[None, 1, -1][seed % 3])
    gpu = {k: v for k, v in gpu.items() if v is not None}
    o = orc.from_sparse(loc, val.copy(), **kw)
    osol = o.solve()
    g = from_sparse(loc, val.copy(), **kw, **gpu)
    gsol = g.solve()
    assert np.array_equal(gsol, osol), (n, m, density, ints, prob, kw, gpu)
    for k in cases.META_KEYS:
        assert g.meta[k] == o.meta[k], k
    sg, so = g.state(), o.state()
    assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
    assert np.array_equal(sg["U"][:sg["K"]], so["U"][:so["K"]])
    assert g.gpu["edges_scanned"] == o.extra["edges_scanned"] and g.gpu["obj_f64"] == o.extra["obj_f64"]


@pytest.mark.parametrize("knobs", [
    dict(cand_refresh=0),                                   # lines never refreshed
    dict(cand_refresh=30),                                  # every line hit of a grid round is rescanned and rebuilt
    dict(cand_refresh=12, cand_build_max_k=300),            # lines used / built in small rounds only (lean scan above)
    dict(cand_build_max_k=5),                               # lines practically only in the tail kernels
    dict(tiled_min_k=1, engine=1),                          # full-scan engine everywhere (partial rounds in person order)
    dict(tiled_min_k=1, engine=1, tail_threshold=0),
    dict(cand=False, tail_threshold=300),                   # no lines: the 512-thread tail kernel takes every mode
    dict(cand=2),                                           # lines without the maintenance pass ahead of the tail
    dict(rounds_per_sync=1), dict(rounds_per_sync=37),      # batch length of the trailing status reads
])
def test_tuning_knobs_do_not_change_the_result(knobs, gpu_lib):
    """Lines (refresh threshold, build limit, on / off), the order of the bidders in partial full-scan rounds, the
    k_bid variant in use and the batch length of the status reads decide what is READ and WHEN -- never the bids:
    sol, round count, prices, list order and the scanned-edge count stay those of the oracle."""
    for seed, (n, m, dens, ints, prob) in enumerate([(3000, 3000, 12.0, 0, "max"), (2500, 4000, 30.0, 3, "min"),
                                                    (9000, 9000, 8.0, 0, "max")]):
        loc, val = synth.gen_sparse(n, m, dens / m, seed=900 + seed, integer_values=ints)
        kw = dict(problem=prob, cardinality_check=False, max_iter=10**8)
        o = orc.from_sparse(loc, val.copy(), **kw)
        osol = o.solve()
        g = from_sparse(loc, val.copy(), **kw, **knobs)
        gsol = g.solve()
        assert np.array_equal(gsol, osol), (knobs, n, m)
        for k in cases.META_KEYS:
            assert g.meta[k] == o.meta[k], (knobs, k)
        sg, so = g.state(), o.state()
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), knobs
        assert np.array_equal(sg["U"][:sg["K"]], so["U"][:so["K"]]), knobs
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], knobs


@pytest.mark.parametrize("env", [
    dict(MISSLAP_ROUND_FUSED="0"),                          # a round with <= 2048 bidders as k_bid + k_round_small
    dict(MISSLAP_LIVE_STATUS="0"),                          # status reads by copy + stream wait
    dict(MISSLAP_LIVE_STATUS="2"),                          # every round-closing kernel posts its status
    dict(MISSLAP_LIVE_STATUS="0", MISSLAP_ROUND_FUSED="0"),
])
def test_environment_switches_do_not_change_the_result(env, gpu_lib, monkeypatch):
    """The A/B switches of README.md (read when a handle is created) select how a round is LAUNCHED and how the host
    learns K -- never the bids: sol, round count, prices, list order and the scanned-edge count stay the oracle's."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for seed, (n, m, dens, ints, prob, gk) in enumerate([(3000, 3000, 12.0, 0, "max", {}), (2500, 4000, 30.0, 3, "min", {}),
                                                        (9000, 9000, 8.0, 0, "max", dict(rounds_per_sync=5)),
                                                        (700, 700, 40.0, 0, "max", dict(tail_threshold=0))]):
        loc, val = synth.gen_sparse(n, m, dens / m, seed=940 + seed, integer_values=ints)
        kw = dict(problem=prob, cardinality_check=False, max_iter=10**8)
        o = orc.from_sparse(loc, val.copy(), **kw)
        osol = o.solve()
        g = from_sparse(loc, val.copy(), **kw, **gk)
        gsol = g.solve()
        assert np.array_equal(gsol, osol), (env, n, m)
        for k in cases.META_KEYS:
            assert g.meta[k] == o.meta[k], (env, k)
        sg, so = g.state(), o.state()
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), env
        assert np.array_equal(sg["U"][:sg["K"]], so["U"][:so["K"]]), env
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], env


def test_concurrent_handles_on_one_gpu_match_the_reference(gpu_lib):
    """Eight host threads, each creating and solving its own problems on its own handle / HIP stream at the same time
    (what `bench.py --concurrent` does at C3): no workgroup of one handle's launches waits for another's (k_round_fused
    hands its bids over without anybody waiting), every handle polls its own live-status words, the block and stream
    caches are shared -- every solve is the oracle's, bit for bit."""
    import threading
    specs = [(1500 + 300 * k, 1500 + 300 * k + (k % 3) * 200, [6.0, 20.0, 60.0][k % 3], [0, 4][k % 2], ["max", "min"][k % 2])
             for k in range(8)]
    want = []
    for k, (n, m, dens, ints, prob) in enumerate(specs):
        loc, val = synth.gen_sparse(n, m, dens / m, seed=5100 + k, integer_values=ints)
        o = orc.from_sparse(loc, val.copy(), problem=prob, cardinality_check=False, max_iter=10**8)
        osol = o.solve()
        want.append((loc, val, prob, osol, {kk: o.meta[kk] for kk in cases.META_KEYS}, o.state()["p"].view(np.uint64).copy(),
                     o.extra["edges_scanned"]))
    errs = []
    go = threading.Barrier(len(specs))

    def worker(k):
        try:
            loc, val, prob, osol, ometa, op, oedges = want[k]
            go.wait()
            for rep in range(3):
                g = from_sparse(loc, val.copy(), problem=prob, cardinality_check=False, max_iter=10**8)
                gsol = g.solve()
                ok = (np.array_equal(gsol, osol) and all(g.meta[kk] == ometa[kk] for kk in cases.META_KEYS)
                      and np.array_equal(g.state()["p"].view(np.uint64), op) and g.gpu["edges_scanned"] == oedges)
                if not ok:
                    errs.append((k, rep, "mismatch"))
                del g
        except Exception as e:  # noqa: BLE001
            errs.append((k, repr(e)))
    th = [threading.Thread(target=worker, args=(k,)) for k in range(len(specs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


@pytest.mark.parametrize("thr", [None, 0, 12])
@pytest.mark.parametrize("lines", [True, False, 2])
def test_true_fp64_values_with_and_without_lines(lines, thr, gpu_lib):
    """Values that are NOT fp32-exact (what most callers of the reference pass): the 12 B/edge layout with candidate
    lines + fp64 cost lines, without lines, and without the maintenance pass, against the oracle -- sol, rounds,
    prices, list order, scanned edges."""
    r = np.random.default_rng(77)
    for n, m, per_row, prob in ((2500, 2500, 40, "max"), (1800, 2600, 90, "min"), (6000, 6000, 12, "max")):
        loc, _ = synth.gen_sparse(n, m, per_row / m, seed=300 + n)
        val = r.random(loc.shape[0]) * 10.0 + r.random(loc.shape[0]) * 1e-9   # full 53-bit mantissas
        assert not np.array_equal(val, val.astype(np.float32).astype(np.float64))
        kw = dict(problem=prob, cardinality_check=False, max_iter=10**8)
        o = orc.from_sparse(loc, val.copy(), **kw)
        osol = o.solve()
        g = from_sparse(loc, val.copy(), **kw, cand=lines, tail_threshold=thr)
        gsol = g.solve()
        assert g.gpu["bytes_per_edge"] == 12
        assert (g.gpu["cand_hits"] > 0) == bool(lines)
        assert np.array_equal(gsol, osol), (n, m, lines, thr)
        for k in cases.META_KEYS:
            assert g.meta[k] == o.meta[k], k
        sg, so = g.state(), o.state()
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
        assert np.array_equal(sg["U"][:sg["K"]], so["U"][:so["K"]])
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"] and g.gpu["obj_f64"] == o.extra["obj_f64"]


@pytest.mark.parametrize("exact32", [True, False])
@pytest.mark.parametrize("thr", [None, 0])
def test_lines_of_long_rows(exact32, thr, gpu_lib):
    """Rows of more than 256 edges get their candidate lines from the long-row builder of the maintenance pass
    (k_refresh_long; it runs from 1024 edges per row on average): a dense matrix and a mix of long and short rows,
    both value layouts, against the oracle -- sol, rounds, prices, list order, scanned edges."""
    r = np.random.default_rng(123)

    def check(loc, val, prob):
        if exact32:
            val = val.astype(np.float32).astype(np.float64)
        kw = dict(problem=prob, cardinality_check=False, max_iter=10**8)
        o = orc.from_sparse(loc, val.copy(), **kw)
        osol = o.solve()
        g = from_sparse(loc, val.copy(), **kw, tail_threshold=thr)
        gsol = g.solve()
        assert g.gpu["bytes_per_edge"] == (8 if exact32 else 12)
        if thr is None:
            assert g.gpu["cand_hits"] > 0 and g.tail_threshold == 192  # lines exist: the tail kernels are used widely
        assert np.array_equal(gsol, osol)
        for k in cases.META_KEYS:
            assert g.meta[k] == o.meta[k], k
        sg, so = g.state(), o.state()
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
        assert np.array_equal(sg["U"][:sg["K"]], so["U"][:so["K"]])
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"] and g.gpu["obj_f64"] == o.extra["obj_f64"]

    n = 1300  # dense
    ii, jj = np.meshgrid(np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), indexing="ij")
    check(np.stack([ii.ravel(), jj.ravel()], axis=1), r.random(n * n) * 100.0, "max")
    # three long rows (1 500 edges) for every short one (100 edges), 700 x 4 000
    n, m = 700, 4000
    rows, cols = [], []
    for i in range(n):
        k = 100 if i % 4 == 0 else 1500
        c = np.sort(r.choice(m, size=k, replace=False)).astype(np.int32)
        c[0] = min(c[0], i)  # (keeps a perfect matching of the persons possible)
        c = np.unique(np.append(c, np.int32(i)))
        rows.append(np.full(c.shape[0], i, np.int32))
        cols.append(c)
    loc = np.stack([np.concatenate(rows), np.concatenate(cols)], axis=1)
    check(loc, r.random(loc.shape[0]) * 10.0, "min")


def test_plain_c_client_of_the_c_abi(tmp_path, gpu_lib):
    """tests/cabi_client.c -- plain C, no Python / torch in the process -- solves a problem through
    include/misslap.h (create / solve / destroy + the matching guard) and must print the oracle's answer."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed for the C-ABI client test"
    exe = str(tmp_path / "cabi_client")
    subprocess.check_call([cc, "-std=c11", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cabi_client.c"), "-L", os.path.join(root, "sslap_amd"),
                           "-lmisslap", "-Wl,-rpath," + os.path.join(root, "sslap_amd"), "-o", exe])
    for prob, maximize in (("max", 1), ("min", 0)):
        loc, val = synth.gen_sparse(1200, 1500, 0.01, seed=21, integer_values=0)
        inp, out = str(tmp_path / f"in_{prob}.bin"), str(tmp_path / f"out_{prob}.txt")
        with open(inp, "wb") as f:
            f.write(np.int64(loc.shape[0]).tobytes())
            f.write(np.int32(maximize).tobytes())
            f.write(np.ascontiguousarray(loc, dtype=np.int32).tobytes())
            f.write(np.ascontiguousarray(val, dtype=np.float64).tobytes())
        env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
        subprocess.check_call([exe, inp, out], env=env, timeout=120)
        lines = open(out).read().split("\n")
        its, nred, nass, obj, card, n, m, batch_ok = lines[0].split()
        assert batch_ok == "1"  # three more handles through misslap_solve_batch: the same answer, short metas respected
        sol = np.array([int(x) for x in lines[1:1 + int(n)]], dtype=np.int32)
        ref = orc.auction_solve(loc=loc, val=val.copy(), problem=prob, cardinality_check=False, max_iter=10**8)
        assert np.array_equal(sol, ref["sol"])
        assert (int(its), int(nred), int(nass)) == (ref["meta"]["its"], ref["meta"]["nreductions"],
                                                    ref["meta"]["n_assigned"])
        assert float(obj) == ref["extra"]["obj_f64"]
        assert (int(card), int(n), int(m)) == (1200, 1200, int(loc[:, 1].max()) + 1)


# ---- robustness --------------------------------------------------------------------
def test_two_handles_on_one_device_used_alternately(gpu_lib):
    """Two live handles driven round by round in alternation (stepwise ABI): per-handle state only, and the tiled
    kernel's dynamic-LDS opt-in is set for every create."""
    specs = [(6000, 40000, 0.001, 11), (5000, 5000, 0.01, 12)]
    hs, refs = [], []
    for n, m, d, seed in specs:
        loc, val = synth.gen_sparse(n, m, d, seed=seed)
        refs.append(orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8))
        hs.append(from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8, tiled_min_k=1))
    done = [False, False]
    while not all(done):
        for k, h in enumerate(hs):
            if done[k]:
                continue
            st = h.status()
            if st.K == 0 or st.its >= 10**8:
                done[k] = h.phase_end()
            elif st.K > h.tail_threshold:
                h.round_bid()
                h.round_tiebreak()
                h.round_apply()
            else:
                h.run_tail()
    for h, ref in zip(hs, refs):
        sol = h.finish()
        assert np.array_equal(sol, ref["sol"]) and h.meta["its"] == ref["meta"]["its"]
        assert h.gpu["tiled_active"] == 1


def test_many_live_handles_and_the_stream_pool(gpu_lib):
    """Twelve handles alive at once (each on its own stream), solved interleaved, destroyed together -- more idle
    streams than the library's pool keeps (8) -- and then twelve more, which take streams from the pool: every
    result equals the oracle's."""
    import gc
    loc, val = synth.gen_sparse(1200, 1500, 0.01, seed=21)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    for _ in range(2):
        hs = [from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8,
                          tail_threshold=[None, 0, 7, 300][k % 4]) for k in range(12)]
        sols = [h.solve() for h in reversed(hs)]
        for sol, h in zip(sols, reversed(hs)):
            assert np.array_equal(sol, ref["sol"]) and h.meta["its"] == ref["meta"]["its"]
        del hs, sols
        gc.collect()


def test_create_destroy_many_times_does_not_leak(gpu_lib):
    import gc
    import torch
    loc, val = synth.gen_sparse(3000, 9000, 0.002, seed=3)
    bad = loc[::-1].copy()

    def cycle(n):
        for _ in range(n):
            s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, tiled_min_k=1)
            del s
            with pytest.raises(ValueError):  # failing constructors must release their temporaries too
                from_sparse(bad, val.copy(), cardinality_check=False)
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cycle(20)  # warm the allocator / code objects
    free0 = cycle(10)
    free1 = cycle(1000)
    assert free0 - free1 < 8 << 20, f"device memory shrank by {(free0 - free1) >> 20} MiB over 1000 create/destroy cycles"


@pytest.mark.parametrize("thr", [None, 0])
def test_degenerate_shapes(thr, gpu_lib):
    """N = 1; a single column (one object for several persons: runs to max_iter like the reference); one row of a
    wide matrix."""
    cases = [
        (np.array([[0, 0]], dtype=np.int32), np.array([3.0])),
        (np.array([[0, 0], [1, 0], [2, 0]], dtype=np.int32), np.array([3.0, 1.0, 2.0])),
        (np.array([[0, 0], [0, 3], [0, 7]], dtype=np.int32), np.array([1.0, 5.0, 2.0])),
    ]
    for loc, val in cases:
        for prob in ("max", "min"):
            o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=50, cardinality_check=False)
            osol = o.solve()
            g = from_sparse(loc, val.copy(), problem=prob, max_iter=50, cardinality_check=False, tail_threshold=thr)
            gsol = g.solve()
            assert np.array_equal(gsol, osol), (loc.tolist(), prob)
            for k in cases_mod.META_KEYS:
                assert g.meta[k] == o.meta[k], k


@pytest.mark.parametrize("cfg,lines,engine", [("C2", True, True), ("C2", False, True), ("C2", True, False), ("C3", True, True),
                                              ("C4", True, True)])
def test_f64_layout_at_baseline_sizes_matches_reference_hash(cfg, lines, engine, golden_large, gpu_lib):
    """The 12 B/edge kernel instances (int32 col + fp64 val; candidate lines with a parallel line of fp64 costs, or --
    lines off -- rows requested ahead; full scans on the engine's 10 B/edge record format, or -- engine off -- on the
    wave-per-row kernel) at the BASELINE sizes: the configs' values are fp32-exact, so forcing the layout must reproduce
    the reference's assignment."""
    g = golden_large["cases"][cfg]
    spec, kw = cases_mod.LARGE_CASES[cfg]
    loc, val = _config_arrays(cfg)[:2]
    s = from_sparse(loc, val, cardinality_check=False, force_f64=True, cand=lines, tiled_min_k=None if engine else -1, **kw)
    sol = s.solve()
    assert s.gpu["bytes_per_edge"] == 12 and (s.gpu["cand_hits"] > 0) == (lines and cfg != "C4")
    assert s.gpu["tiled_active"] == int(engine) and (not engine or s.gpu["tiled_format"] == 1)
    assert synth.sol_digest(sol) == g["sol_sha256"]
    assert s.meta["its"] == g["meta"]["its"] and s.gpu["obj_f64"] == g["obj_f64"]
    assert s.gpu["edges_scanned"] == g["edges_scanned"]


def test_dense_ingest_rejects_more_entries_than_row_pointers_can_address(gpu_lib):
    """the valid entries of a dense input are counted in 64 bits and a count the int32 row pointers
    cannot address is rejected (exercised with the limit lowered through the options)."""
    from sslap_amd import AuctionSolver
    mat = np.abs(np.random.default_rng(0).normal(size=(40, 40))) + 0.5
    rc, h, opts, nnz = AuctionSolver.from_dense(mat, problem="max", nnz_limit=1000)
    assert rc != 0 and nnz == 1600
    from sslap_amd import _lib
    assert b"valid entries" in _lib.load().misslap_last_error()
    rc, h, opts, nnz = AuctionSolver.from_dense(mat, problem="max", nnz_limit=1601)
    assert rc == 0 and nnz == 1600
    AuctionSolver._from_handle(h, opts, "max").solve()
    loc, val = synth.gen_sparse(100, 100, 0.2, seed=2)
    with pytest.raises(ValueError, match="nnz must be <"):
        from_sparse(loc, val, cardinality_check=False, nnz_limit=loc.shape[0])


def test_dense_nan_entries_are_invalid_like_in_the_reference(gpu_lib):
    """`v >= 0` (auction_.pyx:549) is false for NaN: a NaN entry is dropped exactly like a -1."""
    r = np.random.default_rng(5)
    mat = r.uniform(0, 10, size=(60, 70))
    holes = r.random(mat.shape) < 0.3
    nans = r.random(mat.shape) < 0.2
    m_nan = mat.copy()
    m_nan[holes] = -1
    m_nan[nans] = np.nan
    m_ref = mat.copy()
    m_ref[holes | nans] = -1
    for prob in ("max", "min"):
        got = auction_solve(mat=m_nan.copy(), problem=prob, cardinality_check=False)
        want = orc.auction_solve(mat=m_ref.copy(), problem=prob, cardinality_check=False)
        assert np.array_equal(got["sol"], want["sol"])
        for k in cases_mod.META_KEYS:
            assert got["meta"][k] == want["meta"][k], k


def test_malformed_indices_are_rejected_without_out_of_bounds_writes(gpu_lib):
    loc = np.array([[-2, 0], [-1, 1], [0, 0], [1, 1]], dtype=np.int32)
    with pytest.raises(ValueError, match="negative"):
        from_sparse(loc, np.ones(4), cardinality_check=False, size=(2, 2))
    loc = np.array([[0, 0], [1, -5]], dtype=np.int32)
    with pytest.raises(ValueError, match="negative"):
        from_sparse(loc, np.ones(2), cardinality_check=False, size=(2, 2))


def test_hip_runtime_is_shared_in_either_import_order(gpu_lib):
    """a pure-numpy process, `sslap_amd` before `torch` and `torch` before `sslap_amd` must all end
    with ONE HIP runtime that serves both (sslap_amd/_lib.py::_preload_hip_runtime; no torch import on the
    caller's behalf).  Each order runs in a fresh interpreter."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = f"""
import sys; sys.path.insert(0, {root!r})
import numpy as np
from sslap_amd import synth
loc, val = synth.gen_sparse(2000, 2000, 0.01, seed=1)
def solve():
    from sslap_amd import auction_solve
    r = auction_solve(loc=loc, val=val.copy(), problem='max', cardinality_check=False)
    return int(r['meta']['its']), int(r['sol'].sum())
def runtimes():
    return sorted({{l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}})
"""
    progs = {
        "numpy_only": "a = solve(); assert 'torch' not in sys.modules; print('OK', a, runtimes())",
        "misslap_then_torch": "a = solve(); assert 'torch' not in sys.modules; import torch; "
                              "x = torch.arange(10, device='cuda').sum().item(); b = solve(); "
                              "assert a == b and x == 45; print('OK', a, runtimes())",
        "torch_then_misslap": "import torch; x = torch.arange(10, device='cuda').sum().item(); a = solve(); "
                              "y = torch.ones(5, device='cuda').sum().item(); assert x == 45 and y == 5; "
                              "print('OK', a, runtimes())",
    }
    outs = {}
    for name, code in progs.items():
        try:
            p = subprocess.run([sys.executable, "-X", "faulthandler", "-c", common + code], capture_output=True, text=True, timeout=150)
        except subprocess.TimeoutExpired as ex:  # (say WHICH order hangs, and where)
            raise AssertionError((name, "timed out", (ex.stdout or b"")[-300:], (ex.stderr or b"")[-1500:]))
        assert p.returncode == 0, (name, p.stdout[-300:], p.stderr[-600:])
        line = [l for l in p.stdout.splitlines() if l.startswith("OK")][-1]
        outs[name] = line
        assert line.count("libamdhip64") == 1, (name, line)  # exactly one runtime mapped
    assert len({o.split("[")[0] for o in outs.values()}) == 1, outs  # the same answer in every process


# ---- long rows: fixtures captured from the real reference ----------------------------------------
LONG_THRESHOLDS = [None, 0, 2, 16, 64, 512]


@pytest.mark.parametrize("thr", [None, 0, 16])
@pytest.mark.parametrize("name", sorted(cases.LONG_CASES))
def test_long_row_cases_match_reference(name, thr, golden_long, monkeypatch, gpu_lib):
    manifest, arrays = golden_long
    spec, kw, entry = cases.LONG_CASES[name]
    loc, val = cases.synth_inputs(spec)
    res, call = _solve_gpu(entry, loc, val.copy(), spec, kw, monkeypatch, thr)
    g = manifest["cases"][name]
    assert np.array_equal(res["sol"], arrays[name + "/sol"])
    for k in cases.META_KEYS:
        assert res["meta"][k] == g["meta"][k], k
    assert res["meta"]["gpu"]["obj_f64"] == g["obj_f64"]
    assert res["meta"]["gpu"]["edges_scanned"] == g["edges_scanned"]


@pytest.mark.parametrize("thr", [None, 0, 512])
@pytest.mark.parametrize("name", sorted(cases.LONG_TRACE_CASES))
def test_long_row_round_trace_matches_reference(name, thr, golden_long, monkeypatch, gpu_lib):
    """person_to_object after r = 1..80 rounds against the REFERENCE's own runs capped at r."""
    manifest, arrays = golden_long
    spec, kw = cases.LONG_TRACE_CASES[name]
    loc, val = cases.synth_inputs(spec)
    want, its = arrays[name + "/p2o"], manifest["traces"][name]["its"]
    for r in range(1, manifest["rounds"] + 1):
        res, _ = _solve_gpu("locval", loc, val.copy(), spec, dict(kw, max_iter=r), monkeypatch, thr)
        assert res["meta"]["its"] == its[r - 1]
        assert np.array_equal(res["sol"], want[r - 1]), f"round {r}"


@pytest.mark.parametrize("engine", [0, 1])
@pytest.mark.parametrize("thr", LONG_THRESHOLDS)
@pytest.mark.parametrize("name", sorted(cases.LONG_TRACE_CASES))
def test_long_row_full_state_round_by_round(name, thr, engine, gpu_lib):
    """prices, U-list order, K, p2o, o2p after r rounds against the oracle capped at r, on rows of 600 and 1500
    edges: the full scan's second and later 256-edge passes, rows too long for candidate lines, the tile-major
    kernel's long-segment loop (engine 1: k_bid_tiled forced for every grid round), for every tail threshold."""
    spec, kw = cases.LONG_TRACE_CASES[name]
    loc, val = cases.synth_inputs(spec)
    gpu = dict(tail_threshold=thr)
    if engine:
        gpu.update(tiled_min_k=1, engine=engine)
    for r in [1, 2, 3, 4, 5, 7, 9, 12, 16, 20, 25, 30, 40, 50, 65, 80, 120, 200]:
        o = orc.from_sparse(loc, val.copy(), max_iter=r, cardinality_check=False, **kw)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), max_iter=r, cardinality_check=False, **kw, **gpu)
        g.solve()
        sg = g.state()
        if engine:
            assert g.gpu["tiled_active"] == engine
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], r


# ---- rows beyond 8 192 and beyond 16 384 edges: fixtures captured from the real reference -------------
@pytest.mark.parametrize("thr", [None, 0, 16])
@pytest.mark.parametrize("name", sorted(cases.XLONG_CASES))
def test_xlong_row_cases_match_reference(name, thr, golden_xlong, monkeypatch, gpu_lib):
    """dense 9000 x 9000 through `mat=` (rows in the 512-thread line builder's range, k_refresh_long<E, 512>) and rows
    of 17 000 / 20 000 edges (no lines at all, tail threshold 40): sol, meta, objective, edges scanned."""
    manifest, arrays = golden_xlong
    spec, kw, entry = cases.XLONG_CASES[name]
    loc, val = cases.synth_inputs(spec)
    res, call = _solve_gpu(entry, loc, val.copy(), spec, kw, monkeypatch, thr)
    g = manifest["cases"][name]
    assert np.array_equal(res["sol"], arrays[name + "/sol"])
    for k in cases.META_KEYS:
        assert res["meta"][k] == g["meta"][k], k
    assert res["meta"]["gpu"]["obj_f64"] == g["obj_f64"]
    assert res["meta"]["gpu"]["edges_scanned"] == g["edges_scanned"]
    assert res["meta"]["gpu"]["complete_assignment"] == (True, True, spec["n"] >= spec["m"])
    assert res["meta"]["gpu"]["valid_assignment"] is True


@pytest.mark.parametrize("thr", [None, 0])
@pytest.mark.parametrize("name", sorted(cases.XLONG_TRACE_CASES))
def test_xlong_row_round_trace_matches_reference(name, thr, golden_xlong, monkeypatch, gpu_lib):
    """person_to_object after r = 1..R rounds against the REFERENCE's own runs capped at r."""
    manifest, arrays = golden_xlong
    spec, kw, rounds = cases.XLONG_TRACE_CASES[name]
    loc, val = cases.synth_inputs(spec)
    want, its = arrays[name + "/p2o"], manifest["traces"][name]["its"]
    for r in range(1, rounds + 1):
        res, _ = _solve_gpu("locval", loc, val.copy(), spec, dict(kw, max_iter=r), monkeypatch, thr)
        assert res["meta"]["its"] == its[r - 1]
        assert np.array_equal(res["sol"], want[r - 1]), f"round {r}"


_XLONG_ORACLE_STATES = {}


def _xlong_oracle_states(name, rounds):
    """The oracle stepped ONCE per case (a round of the 9000 x 9000 instance scans 81 M edges on the host): state
    snapshots after the given round counts, shared by every parametrisation.  A capped solve breaks out before the
    eps-phase reset (auction_.pyx:275-292), a stepped solver performs it -- so the snapshot is taken from a fresh
    solve only where stepping and capping differ, i.e. never inside the first phase's rounds used here."""
    if name not in _XLONG_ORACLE_STATES:
        spec, kw, _ = cases.XLONG_TRACE_CASES[name]
        loc, val = cases.synth_inputs(spec)
        out = {}
        for r in rounds:
            o = orc.from_sparse(loc, val.copy(), max_iter=r, cardinality_check=False, **kw)
            o.solve()
            out[r] = (o.state(), o.extra["edges_scanned"])
        _XLONG_ORACLE_STATES[name] = (loc, val, out)
    return _XLONG_ORACLE_STATES[name]


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("thr", [None, 0, 16])
@pytest.mark.parametrize("name", sorted(cases.XLONG_TRACE_CASES))
def test_xlong_row_full_state_round_by_round(name, thr, f64, gpu_lib):
    """prices, U-list order, K, p2o, o2p after r rounds against the oracle capped at r, on rows of 9 000 edges (the
    512-thread line builder) and of 17 000 edges (no lines), for three tail thresholds and both value layouts."""
    spec, kw, _ = cases.XLONG_TRACE_CASES[name]
    rounds = [1, 2, 3, 5, 8, 13, 21, 40, 90] if spec["n"] >= 9000 else [1, 2, 3, 4, 5, 7, 9, 12, 16, 20, 25, 30, 40, 50, 65, 80, 120, 200, 400]
    loc, val, states = _xlong_oracle_states(name, rounds)
    for r in rounds:
        so, edges = states[r]
        g = from_sparse(loc, val.copy(), max_iter=r, cardinality_check=False, tail_threshold=thr, force_f64=f64, **kw)
        g.solve()
        sg = g.state()
        assert g.gpu["bytes_per_edge"] == (12 if f64 else 8)
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert g.gpu["edges_scanned"] == edges, r


def test_d1_dense_8000_matches_reference_hash(golden_large, gpu_lib):
    """D1 (dense 8000 x 8000, the shape of the reference's `mat=` entry; bench.py --config D1): sha256 of the
    assignment, rounds, objective against the real reference."""
    g = golden_large["cases"].get("D1")
    if g is None:
        pytest.skip("D1 fixture not generated")
    spec, kw = cases.LARGE_CASES["D1"]
    loc, val = cases.synth_inputs(spec)
    assert synth.input_digest(loc, val) == g["input_sha256"]
    res = auction_solve(loc=loc, val=val, cardinality_check=False, **kw)
    assert synth.sol_digest(res["sol"]) == g["sol_sha256"]
    for k in cases.META_KEYS:
        assert res["meta"][k] == g["meta"][k], k
    assert res["meta"]["gpu"]["obj_f64"] == g["obj_f64"] and res["meta"]["gpu"]["edges_scanned"] == g["edges_scanned"]


def test_abi1_caller_is_still_served(gpu_lib):
    """A caller built against the round-2 header: 88-byte options with the knobs in reserved[], a 376-byte meta without a
    size field.  The library recognises it by the options' struct_size and answers in the old layout."""
    import ctypes as C
    from sslap_amd import _lib
    lib = _lib.load()

    class OptionsV1(C.Structure):
        _fields_ = _lib.Options._fields_[:12] + [("reserved", C.c_int32 * 8)]

    class MetaV1(C.Structure):
        _fields_ = [f for f in _lib.Meta._fields_[2:] if f[0] not in ("complete_assignment", "valid_assignment",
                                                                     "lines_active", "reserved_i", "sharded_rounds", "tiled_format",
                                                                     "phases_with_lines", "eps_phases", "filter_undecided")]
    assert C.sizeof(OptionsV1) == 88 and C.sizeof(MetaV1) == 376
    loc, val = synth.gen_sparse(1200, 1200, 0.02, seed=3)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False)
    for knobs in ({}, {4: 1}, {0: 1, 2: 1, 1: 9}, {7: 300 | (25 << 24)}):  # defaults / no lines / tiled forced, shape 8 / line tuning
        o = OptionsV1(struct_size=88, maximize=1, max_iter=10**6, tail_threshold=-1)
        for k, v in knobs.items():
            o.reserved[k] = v
        h = C.c_void_p()
        _lib.check(lib.misslap_create(C.byref(h), loc.shape[0], loc.ctypes.data, val.ctypes.data,
                                      C.cast(C.byref(o), C.POINTER(_lib.Options))))
        sol = np.empty(1200, np.int32)
        buf = (C.c_byte * (376 + 64))()
        C.memset(buf, 0x5a, len(buf))
        _lib.check(lib.misslap_solve(h, sol.ctypes.data, C.cast(buf, C.POINTER(_lib.Meta))))
        lib.misslap_destroy(h)
        m = MetaV1.from_buffer_copy(buf)
        assert bytes(buf)[376:] == b"\x5a" * 64, "wrote past the version-1 struct"
        assert np.array_equal(sol, ref["sol"]) and m.its == ref["meta"]["its"] and m.n_rows == 1200
        assert m.obj_f64 == ref["extra"]["obj_f64"] and m.edges_scanned == ref["extra"]["edges_scanned"]
        assert m.bytes_per_edge == 8 and m.tiled_active == (1 if knobs.get(0) else 0)
    # an ABI-2 caller with a shorter struct gets exactly that many bytes
    o2 = _lib.Options(struct_size=C.sizeof(_lib.Options), maximize=1, max_iter=10**6, tail_threshold=-1)
    h = C.c_void_p()
    _lib.check(lib.misslap_create(C.byref(h), loc.shape[0], loc.ctypes.data, val.ctypes.data, C.byref(o2)))
    buf = (C.c_byte * C.sizeof(_lib.Meta))()
    C.memset(buf, 0x5a, len(buf))
    m = _lib.Meta.from_buffer(buf)
    short = _lib.Meta.edges_scanned.offset + 8
    m.struct_size = short
    _lib.check(lib.misslap_solve(h, None, C.byref(m)))
    assert m.struct_size == short and m.abi_version == 2 and m.its == ref["meta"]["its"]
    assert bytes(buf)[short:] == b"\x5a" * (len(buf) - short)
    m.struct_size = 8  # too small to hold the reference's meta fields
    with pytest.raises(ValueError, match="struct_size"):
        _lib.check(lib.misslap_finish(h, None, C.byref(m)))
    lib.misslap_destroy(h)


def test_validity_flags_equal_the_host_computation(gpu_lib):
    """complete_assignment / valid_assignment of the reference's benchmark harness (benchmarking.py:56-64), reduced on
    the device, against the same expressions on the host -- for a complete solve, a solve cut off by max_iter (sol has
    -1 entries: numpy's index wrap-around selects the LAST column), 'min' and a rectangular instance."""
    rng = np.random.RandomState(7)
    for n, m, dens, prob, max_iter in ((300, 300, 0.2, "max", 10**6), (300, 300, 0.2, "min", 10**6), (300, 300, 0.2, "max", 4),
                                      (200, 260, 0.3, "max", 10**6), (250, 250, 0.15, "min", 3), (120, 120, 1.0, "max", 2)):
        mat = rng.uniform(0, 100, (n, m))
        mask = rng.random_sample((n, m)) > dens
        mask[np.arange(n), rng.permutation(m)[:n]] = False  # feasible
        mat[mask] = -1
        res = auction_solve(mat.copy(), problem=prob, max_iter=max_iter, cardinality_check=False)
        sol = res["sol"]
        size = n  # benchmarking.py: self.size = number of rows
        sel = mat[np.arange(size), sol]
        want_complete = (np.unique(sol).size == size, bool((sol >= 0).all()), bool((sol < size).all()))
        want_valid = bool((sel >= 0).all())
        g = res["meta"]["gpu"]
        assert g["complete_assignment"] == want_complete, (n, m, prob, max_iter)
        assert g["valid_assignment"] == want_valid, (n, m, prob, max_iter)


def test_lines_are_dropped_from_the_first_phase_whose_eps_is_below_the_rounding_error(gpu_lib):
    """Candidate lines rely on prices only rising; once eps (down to 0.15 / N) comes within 2^9 ulps of the largest
    |cost|, a price update fl(fl(c - w) + eps) may round DOWN.  The guard is per eps-phase: the early phases (eps far above
    the rounding error) run WITH lines, the lines are dropped for good from the first phase below the bound
    (meta['gpu']['phases_with_lines'] < 'eps_phases', 'lines_active' == 0 at the end), and the result still equals the
    oracle bit for bit."""
    loc, val = synth.gen_sparse(800, 800, 0.03, seed=9)
    big = np.float64(np.float32(1e10)) + val * 1024.0  # |cost| ~ 1e10 (ulp 1.9e-6) against eps >= 1.9e-4
    for v in (big, np.round(val * 1e8)):
        ref = orc.auction_solve(loc=loc, val=v.copy(), problem="max", cardinality_check=False, max_iter=10**7)
        for thr in (None, 0):
            s = from_sparse(loc, v.copy(), problem="max", cardinality_check=False, max_iter=10**7, tail_threshold=thr)
            sol = s.solve()
            g = s.gpu
            assert g["eps_phases"] == s.meta["nreductions"] + 1
            assert g["lines_active"] == 0 and 0 < g["phases_with_lines"] < g["eps_phases"], (g["phases_with_lines"], g["eps_phases"])
            assert g["phases_with_lines"] >= g["eps_phases"] - 2  # only the last phase(s) are below the bound
            assert g["cand_hits"] > 0
            assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
            assert g["obj_f64"] == ref["extra"]["obj_f64"]
    s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False)
    s.solve()
    assert s.gpu["lines_active"] == 1 and s.gpu["phases_with_lines"] == s.gpu["eps_phases"] == s.meta["nreductions"] + 1


def test_integer_costs_of_1e8_at_1e5_persons_keep_their_lines_until_the_last_phases(gpu_lib):
    """Ordinary integer costs at scale (max |cost| = 1e8, N = 100 000: 1e8 x 2^-44 = 5.7e-6 against a last phase's eps of
    1.5e-6 .. 1e-5): the all-or-nothing guard of round 4 ran the whole solve without lines; now only the phases below
    the bound do.  Bit-equal to the oracle."""
    n = 100_000
    loc, val = synth.gen_sparse(n, n, 0.0005, seed=21)
    v = np.round(val * 1e6)
    assert v.max() > 9e7
    ref = orc.auction_solve(loc=loc, val=v.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    s = from_sparse(loc, v.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    sol = s.solve()
    g = s.gpu
    assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"] and g["obj_f64"] == ref["extra"]["obj_f64"]
    assert g["eps_phases"] == s.meta["nreductions"] + 1 and g["phases_with_lines"] >= g["eps_phases"] - 2
    assert g["cand_hits"] > g["bids_made"] // 2


def test_rccl_world1_smoke(gpu_lib):
    """the RCCL path of the library executes -- librccl opened at run time, ncclGetUniqueId,
    ncclCommInitRank (world 1), and ncclAllReduce MAX (int64) / MIN (int32) issued on the solver's stream between
    k_bid, k_tiebreak and k_apply for EVERY grid round (shard_min_k = -1) -- and the solve still equals the oracle."""
    from sslap_amd.dist import Comm, solve_sharded
    comm = Comm.rccl(0, 1, 0, lambda uid: uid)
    assert comm.info() == dict(kind="rccl", rank=0, world=1, transport_ranks=1)  # transport_ranks = ncclCommCount
    for n, dens, seed, ints, thr in ((1500, 0.02, 1, 0, 0), (30000, 0.002, 4, 0, None), (2000, 0.02, 5, 3, 8)):
        loc, val = synth.gen_sparse(n, n, dens, seed=seed, integer_values=ints)
        ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
        s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8, shard=(0, 1),
                        tail_threshold=thr, shard_min_k=-1)
        sol = solve_sharded(s, comm)
        assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
        assert s.gpu["obj_f64"] == ref["extra"]["obj_f64"] and s.gpu["edges_scanned"] == ref["extra"]["edges_scanned"]
        assert s.gpu["sharded_rounds"] == s.gpu["grid_rounds"] > 0  # shard_min_k = -1: every grid round is exchanged
    # a communicator that does not match the handle's shard is refused
    s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, shard=(0, 2))
    with pytest.raises(ValueError, match="communicator is rank 0 of 1"):
        solve_sharded(s, comm)


@pytest.mark.parametrize("shape,fmt", [(0, 0), (4, 0), (7, 0), (8, 0), (9, 0), (0, 1), (8, 1), (9, 1), (0, 2), (8, 2), (9, 2),
                                       (0, 3), (8, 3), (9, 3)])
@pytest.mark.parametrize("spec,prob", [
    (dict(kind="sparse", n=6000, m=40000, density=0.001), "max"),           # ~10 edges per (person, tile) segment
    (dict(kind="sparse", n=5000, m=25000, density=0.004, ints=5), "min"),   # ~33 edges per segment, ties
    (dict(kind="sparse", n=4200, m=12000, density=0.01), "max"),            # ~60 edges per segment
])
def test_tiled_kernel_shapes_round_by_round(spec, prob, shape, fmt, gpu_lib):
    """Every lanes-per-person variant of k_bid_tiled (4 / 8 / 16 lanes: shapes 0, 7 / 8 / 9; shape 4: the column split) on short, medium and long
    (person, tile) segments -- a shape that is too short for the segments sends their tails to the overflow lists --,
    forced for every grid round: full state vs the oracle.  The three production shapes also in the record formats
    1..3 (fp64 values; stored index carried on row-shuffled input)."""
    loc, val = cases.synth_inputs(dict(spec, kind="shuffled") if fmt >= 2 else spec)
    for r in [1, 2, 3, 5, 8, 13, 30, 80]:
        o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, tail_threshold=0,
                        tiled_min_k=1, engine=1, tiled_shape=shape, force_f64=bool(fmt & 1))
        g.solve()
        assert g.gpu["tiled_active"] == 1 and g.gpu["tiled_format"] == fmt
        sg = g.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], r


def test_integration_md_sharded_binding_stub_works(gpu_lib):
    """The reference-side binding of the sharded solve printed in INTEGRATION.md, executed verbatim (world 1, RCCL)."""
    import os
    import re
    from sslap_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(# sslap/misslap_binding.py.*?)```", text, re.S)
    assert len(blocks) == 3  # single GPU, sharded, many problems at a time
    ns = {}
    for code in blocks:
        exec(compile(code.replace('C.CDLL("libmisslap.so")', f'C.CDLL({_lib.LIB_PATH!r})'), "INTEGRATION.md", "exec"), ns)
    loc, val = synth.gen_sparse(900, 900, 0.03, seed=13)
    sol = ns["solve_sharded"](loc, val.copy(), 0, 1, 0, lambda uid: uid, problem="max")
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False)
    assert np.array_equal(sol, ref["sol"])
    # ... and the binding of the batched solve (misslap_solve_batch), executed verbatim as well
    probs = [synth.gen_sparse(900, 900, 0.03, seed=40 + k) for k in range(5)]
    solvers = [ns["_from_sparse"](l, v.copy(), problem="max", cardinality_check=False) for l, v in probs]
    sols = ns["solve_many"](solvers)
    for (l, v), got in zip(probs, sols):
        assert np.array_equal(got, orc.auction_solve(loc=l, val=v.copy(), problem="max", cardinality_check=False)["sol"])


def _drive_to_phase_end(g):
    """rounds of the stepwise API until everybody is assigned (the end of an eps-phase)"""
    for _ in range(10**7):
        st = g.status()
        if st.K == 0:
            return st
        if st.K > g.tail_threshold:
            g.round_bid()
            g.round_tiebreak()
            g.round_apply()
        else:
            g.run_tail()
    raise AssertionError("the phase did not end")


@pytest.mark.parametrize("label,spec,prob,kw", [
    # the pass on the full-scan engine (tile-major copy): 4 / 8 / 16 lanes per person, several column tiles
    ("tiled4", dict(kind="sparse", n=6000, m=40000, density=0.001), "max", dict(tiled_min_k=1, engine=1)),
    ("tiled8", dict(kind="sparse", n=5000, m=25000, density=0.004, ints=5), "min", dict(tiled_min_k=1, engine=1, tiled_shape=8)),
    ("tiled16", dict(kind="sparse", n=4200, m=12000, density=0.01), "max", dict(tiled_min_k=1, engine=1, tiled_shape=9)),
    ("tiled_default", dict(kind="sparse", n=9000, m=9000, density=0.004), "max", dict()),
    # the same entry stored more than once: the LAST one is the choice (auction_.pyx:467-471)
    ("dups", dict(kind="dups", n=150, density=0.06, ints=6), "max", dict()),
    ("tiled_dups", dict(kind="dups", n=5000, density=0.004, ints=9, adjacent=True), "max", dict(tiled_min_k=1, engine=1)),
    # 12 B/edge layout (values that are not fp32-exact): the pass on the row-major CSR, and on the engine (format 1)
    ("f64", dict(kind="f64", n=4500, density=0.004), "min", dict(tiled_min_k=-1)),
    ("forced_f64", dict(kind="sparse", n=6000, m=6000, density=0.003), "max", dict(force_f64=True, tiled_min_k=-1)),
    ("tiled_f64", dict(kind="f64", n=4500, density=0.004), "min", dict(tiled_min_k=1, engine=1)),
    ("tiled16_f64", dict(kind="sparse", n=4200, m=12000, density=0.01), "max", dict(tiled_min_k=1, engine=1, tiled_shape=9, force_f64=True)),
    # rows in a random stored order: the engine's formats 2 / 3 (the LAST stored match is the choice, by stored index)
    ("tiled_shuffled", dict(kind="shuffled", n=6000, m=40000, density=0.001, ints=7), "max", dict(tiled_min_k=1, engine=1)),
    ("tiled8_shuffled_f64", dict(kind="shuffled", n=5000, m=25000, density=0.004, ints=5), "min", dict(tiled_min_k=1, engine=1, tiled_shape=8, force_f64=True)),
    # fewer rows than the sample: the sample IS the pass
    ("small", dict(kind="sparse", n=300, m=300, density=0.05), "max", dict()),
    ("tiled_rect", dict(kind="sparse", n=5000, m=7500, density=0.004), "max", dict(tail_threshold=0)),
])
def test_ece_pass_equals_the_reference_loop_at_every_phase_end(label, spec, prob, kw, gpu_lib):
    """misslap_check_ece (sample pass + full pass, on the full-scan engine where the handle has the tile-major copy)
    against eCE_satisfied of the reference (auction_.pyx:443-485, restated on arrays in the oracle) at the state the GPU
    holds at the end of every eps-phase -- states that fail the test and the final one that passes -- for a range of
    eps: the phase's own, the target, zero, negative, huge."""
    loc, val = cases.synth_inputs(spec)
    g = from_sparse(loc, val.copy(), problem=prob, max_iter=10**7, cardinality_check=False, **kw)
    seen = set()
    for phase in range(40):
        st = _drive_to_phase_end(g)
        assert st.K == 0
        s = g.state()
        for eps in (st.target_eps, st.eps, 0.0, -1.0, 1e-3, 1e-6, 3.0e38, np.float32(st.eps) * np.float32(4)):
            want = orc.ece_satisfied(loc, val, prob, s["p"], s["p2o"], eps)
            got = g.check_ece(eps)
            assert got == want, (label, phase, eps)
            seen.add(want)
        if g.phase_end():
            break
    assert seen == {True, False}
    # ... and the fused final pass: eCE, objective, validity flags from ONE scan
    sol = g.finish()
    assert g.gpu["tiled_active"] == int(label.startswith("tiled"))
    if label == "tiled_dups":  # a repeated column: the tie rule needs the stored index (formats 0 / 1 order ties by column)
        assert g.gpu["tiled_format"] == 2
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem=prob, cardinality_check=False, max_iter=10**7)
    assert np.array_equal(sol, ref["sol"]) and g.meta["eCE"] == ref["meta"]["eCE"] == 1
    assert g.meta["soln_found"] == ref["meta"]["soln_found"] and g.gpu["obj_f64"] == ref["extra"]["obj_f64"]
    n = int(loc[:, 0].max()) + 1  # benchmarking.py:56-64 with size = number of rows
    assert g.gpu["complete_assignment"] == (np.unique(sol).size == n, True, bool((sol < n).all())) and g.gpu["valid_assignment"]


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("shape", [None, 8, 9])
def test_repeated_entries_on_the_engine_round_by_round(shape, f64, gpu_lib):
    """Rows that store an entry more than once (ascending columns, not strictly; equal AND different values under the
    same column, integer costs: ties everywhere): formats 0 / 1 of the tile-major copy order equal values by column,
    which needs unique columns, so the ingest must send such input to the stored-index formats -- full state vs the
    oracle, engine forced for every grid round."""
    spec = dict(kind="dups", n=4000, density=0.004, ints=4, adjacent=True)
    loc, val = cases.synth_inputs(spec)
    kw = dict(tiled_shape=shape) if shape else {}
    for r in [1, 2, 3, 5, 8, 13, 30, 80]:
        o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=r, cardinality_check=False)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem="max", max_iter=r, cardinality_check=False, tail_threshold=0,
                        tiled_min_k=1, engine=1, force_f64=f64, **kw)
        g.solve()
        assert g.gpu["tiled_active"] == 1 and g.gpu["tiled_format"] == (3 if f64 else 2)
        sg = g.state()
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r


@pytest.mark.parametrize("rounds", [1, 7, 300])
def test_tail_launches_are_bounded_in_rounds(rounds, gpu_lib, monkeypatch):
    """No tail kernel instance runs more than MISSLAP_TAIL_LAUNCH_ROUNDS rounds (default 2^22: a degenerate instance --
    scaled integer costs against a tiny eps -- is a price war of 1e10 rounds, and ONE launch would sit on the device until
    max_iter); the host looks at the status and launches again.  Forced to 1 / 7 / 300 rounds per launch: the result is
    the reference's, bit for bit, through hundreds of returns."""
    monkeypatch.setenv("MISSLAP_TAIL_LAUNCH_ROUNDS", str(rounds))
    for spec, prob, max_iter in [(dict(kind="sparse", n=700, m=700, density=0.02, ints=4), "max", 10**8),
                                 (dict(kind="sparse", n=2500, m=3000, density=0.004), "min", 10**8),
                                 (dict(kind="sparse", n=900, m=900, density=0.01, ints=11), "max", 1234)]:
        if rounds == 1 and spec["n"] > 1000:
            continue  # (thousands of launches: the small instances are enough for the one-round budget)
        loc, val = cases.synth_inputs(spec)
        if max_iter != 10**8:
            val = np.round(val * 1e6)  # the degenerate kind: it would run for ~1e10 rounds
        o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=max_iter, cardinality_check=False)
        osol = o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem=prob, max_iter=max_iter, cardinality_check=False)
        gsol = g.solve()
        sg = g.state()
        assert np.array_equal(gsol, osol) and sg["its"] == so["its"] and sg["K"] == so["K"]
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)) and np.array_equal(sg["U"], so["U"])
        assert all(g.meta[k] == o.meta[k] for k in cases.META_KEYS)


@pytest.mark.parametrize("thr", [None, 0, 16])
def test_falling_prices_without_lines_equal_the_reference(thr, gpu_lib):
    """Costs of ~2^50 over four binades against eps down to 0.15 / N: a price update fl(fl(c - w) + eps) rounds DOWN
    now and then, i.e. prices FALL (the reference then cycles until max_iter).  The precision guard drops the candidate
    lines from the first eps-phase in which that can happen (the phases before it -- eps from 2^50 down to 2^7 -- run with
    them: the mixed regime), nothing else depends on rising prices, so the solve must neither fail (kErrPriceFell is
    raised only while lines are in use) nor differ from the reference in a single bit."""
    n, max_iter = 300, 5000
    loc, _ = synth.gen_sparse(n, n, 0.05, seed=10)
    val = 2.0 ** 47 * (1.0 + 15.0 * np.random.RandomState(10).random_sample(loc.shape[0]))
    o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=max_iter, cardinality_check=False)
    prev, falls = o.state()["p"], 0
    while not o.step():
        p = o.state()["p"]
        falls += int((p < prev).sum())
        prev = p
    assert falls > 100  # the instance does what it is here for
    so = o.state()
    g = from_sparse(loc, val.copy(), problem="max", max_iter=max_iter, cardinality_check=False, tail_threshold=thr)
    sol = g.solve()
    assert g.gpu["lines_active"] == 0 and g.meta["its"] == max_iter == so["its"]
    assert 0 < g.gpu["phases_with_lines"] < g.gpu["eps_phases"]
    sg = g.state()
    assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64))
    assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sol, so["p2o"]) and np.array_equal(sg["U"], so["U"])


_CFG_STORE = {}


def _config_arrays(cfg):
    """(loc, val) of a BASELINE config, generated once per session (C5 takes a minute) and kept on /dev/shm for the rank
    processes of the sharded tests, which load the files instead of generating the input W more times."""
    import os
    import tempfile
    if cfg not in _CFG_STORE:
        loc, val = synth.gen_config(cfg)
        d = tempfile.mkdtemp(prefix="misslap_cfg_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        paths = (os.path.join(d, cfg + "_loc.npy"), os.path.join(d, cfg + "_val.npy"))
        np.save(paths[0], loc)
        np.save(paths[1], val)
        _CFG_STORE[cfg] = (loc, val, paths)
    return _CFG_STORE[cfg]


@pytest.fixture(scope="module", autouse=True)
def _drop_config_store():
    yield
    import shutil
    import os
    for _, _, paths in _CFG_STORE.values():
        shutil.rmtree(os.path.dirname(paths[0]), ignore_errors=True)
    _CFG_STORE.clear()


def _sharded_result(s, sol, comm):
    return (synth.sol_digest(sol), s.meta["its"], s.meta["nreductions"], s.gpu["obj_f64"], s.gpu["edges_scanned"],
            s.gpu["shard_edges"], s.gpu["sharded_rounds"], s.shard_min_K, comm.info())


def _dist_cfg_worker(rank, world, port, cfgs, out):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import torch.distributed as dist
    from sslap_amd import from_sparse
    from sslap_amd.dist import Comm, solve_sharded
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = Comm.gloo_staged()
    res = {}
    for cfg, (loc_path, val_path) in cfgs.items():
        loc, val = np.load(loc_path), np.load(val_path)
        s = from_sparse(loc, val, problem="max", cardinality_check=False, shard=(rank, world), max_iter=10**8)
        sol = solve_sharded(s, comm)  # library defaults: shard_min_K = the full-scan threshold
        res[cfg] = _sharded_result(s, sol, comm)
        del s, loc, val
    out.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def _check_sharded_results(got, world, cfgs, golden_large):
    for cfg in cfgs:
        g = golden_large["cases"][cfg]
        for rank in range(world):
            sha, its, nred, obj, edges, sh, rounds, smk, info = got[rank][cfg]
            assert sha == g["sol_sha256"], (cfg, rank)
            assert (its, nred, obj) == (g["meta"]["its"], g["meta"]["nreductions"], g["obj_f64"]), (cfg, rank)
            assert info == dict(kind="custom", rank=rank, world=world, transport_ranks=world)
            assert rounds > 0 and sh > 0 and smk >= 8192
        per_rank = [got[r][cfg][4:7] for r in range(world)]
        assert len({r for _, _, r in per_rank}) == 1                 # the same rounds were sharded on every rank
        assert len({e - s for e, s, _ in per_rank}) == 1            # the replicated part is identical
        e0, s0, _ = per_rank[0]
        # unique work = the single-GPU (= the reference's) edge count: the ranks' shares of the sharded rounds add up
        assert sum(s for _, s, _ in per_rank) + (e0 - s0) == g["edges_scanned"], cfg


@pytest.mark.parametrize("world,cfgs", [(2, ("C2", "C4")), (4, ("C3", "C5"))])
def test_sharded_solve_at_baseline_sizes_rank_processes_one_gpu(world, cfgs, golden_large, gpu_lib):
    """The sharded path at BASELINE sizes with the library's default shard threshold, the ranks as PROCESSES that share
    cuda:0 and exchange through the custom communicator (gloo, staged through the host): two ranks on C2 and C4 (the
    config with the most sharded rounds per solve, 26 of 176), four ranks on C3 and C5 -- BASELINE config 5 is "C5
    sharded".  (A one-GPU box of this pool admits six processes on its card: four ranks + this one; eight ranks run as
    threads, below.)  Every rank must return the reference's assignment (sha256 of the fixture captured from the real
    reference), and the sharded rounds' shares must add up to the single-GPU count."""
    import socket
    import torch.multiprocessing as mp
    paths = {cfg: _config_arrays(cfg)[2] for cfg in cfgs}
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_cfg_worker, args=(r, world, port, paths, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=900) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    _check_sharded_results(got, world, cfgs, golden_large)
    if "C4" in cfgs:
        assert got[0]["C4"][6] >= 20  # 26 sharded rounds per C4 solve


@pytest.mark.parametrize("world,cfgs", [(8, ("C2", "C3", "C4", "C5")), (3, ("C4",))])
def test_sharded_solve_at_baseline_sizes_rank_threads_one_gpu(world, cfgs, golden_large, gpu_lib):
    """Eight ranks -- BASELINE config 5's world size -- on every BASELINE GPU config, and three (uneven shard ranges on the
    real kernels): the ranks are THREADS of this process (sslap_amd.dist.ThreadGroup / Comm.in_process: eight rank
    processes would exceed what a one-GPU box admits on its card), each with its own handle, stream and communicator;
    the library's loop issues the same exchange calls as with RCCL, the buffers are reduced on the host."""
    import threading
    from sslap_amd.dist import Comm, ThreadGroup, solve_sharded
    got, errs = {}, []
    for cfg in cfgs:
        loc, val, _ = _config_arrays(cfg)
        group = ThreadGroup(world, timeout_s=600.0)

        def rank_main(rank):
            try:
                comm = Comm.in_process(rank, group)
                s = from_sparse(loc, val, problem="max", cardinality_check=False, shard=(rank, world), max_iter=10**8)
                sol = solve_sharded(s, comm)
                got.setdefault(rank, {})[cfg] = _sharded_result(s, sol, comm)
            except Exception as e:  # noqa: BLE001
                errs.append((cfg, rank, repr(e)))
                group.abort()
        th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs[:3]
    _check_sharded_results(got, world, cfgs, golden_large)


@pytest.mark.parametrize("cand", [True, False])
@pytest.mark.parametrize("spec,prob,f64", [
    (dict(kind="sparse", n=3000, m=3000, density=0.01), "max", False),
    (dict(kind="sparse", n=2500, m=4000, density=0.01, ints=4), "max", False),  # ties at the top: the exact scan decides
    (dict(kind="single", n=1500, density=0.02, n_single=40), "min", False),      # one-entry rows: +inf bids, infinite prices
    (dict(kind="f64", n=2500, density=0.01), "min", True),                        # values that are not fp32-exact
    (dict(kind="shuffled", n=2500, m=2500, density=0.012, ints=9), "max", False),
])
def test_f32_filter_scan_round_by_round(spec, prob, f64, cand, gpu_lib, monkeypatch):
    """The wave-per-row kernel's full scans through the single-precision filter (wave_bid_filter: an fp32 mirror of the
    prices decides WHICH two edges are evaluated exactly; ties and near-ties go to the exact scan), forced on a small
    instance (the library uses it where the price table exceeds an XCD's L2 share: C5): full state vs the oracle."""
    monkeypatch.setenv("MISSLAP_F32_FILTER", "1")
    loc, val = cases.synth_inputs(spec)
    for r in [1, 2, 3, 4, 6, 9, 14, 30, 70, 160]:
        o = orc.from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False)
        o.solve()
        so = o.state()
        g = from_sparse(loc, val.copy(), problem=prob, max_iter=r, cardinality_check=False, tail_threshold=0,
                        tiled_min_k=-1, cand=cand)
        g.solve()
        sg = g.state()
        assert g.gpu["tiled_active"] == 0 and g.gpu["bytes_per_edge"] == (12 if f64 else 8)
        assert sg["its"] == so["its"] and sg["K"] == so["K"], r
        assert np.array_equal(sg["U"], so["U"]), r
        assert np.array_equal(sg["p"].view(np.uint64), so["p"].view(np.uint64)), r
        assert np.array_equal(sg["p2o"], so["p2o"]) and np.array_equal(sg["o2p"], so["o2p"]), r
        assert g.gpu["edges_scanned"] == o.extra["edges_scanned"], r


_BATCH_CASES = [
    # (label, spec, problem, number of problems, group size, options of every handle)
    ("small_ints", dict(kind="sparse", n=300, m=300, density=0.05, ints=4), "max", 7, 0, dict()),
    ("rect_grid_only", dict(kind="sparse", n=3000, m=4000, density=0.01), "min", 9, 4, dict(tail_threshold=0)),
    ("mid_default", dict(kind="sparse", n=12000, m=12000, density=0.004), "max", 13, 0, dict()),
    ("mid_tail16", dict(kind="sparse", n=5000, m=5000, density=0.01), "max", 6, 2, dict(tail_threshold=16)),
    ("engine", dict(kind="sparse", n=6000, m=40000, density=0.001), "max", 5, 0, dict(tiled_min_k=1, engine=1)),
    ("engine_f64_shuffled", dict(kind="shuffled", n=5000, m=25000, density=0.004, ints=5), "min", 4, 3,
     dict(tiled_min_k=1, engine=1, force_f64=True)),
    ("f64_values", dict(kind="f64", n=2500, density=0.01), "max", 5, 0, dict()),
    ("dense_long_rows", dict(kind="dense", n=600, m=600), "max", 4, 0, dict()),
    ("max_iter_cut", dict(kind="sparse", n=3000, m=3000, density=0.01), "max", 5, 0, dict(max_iter=57)),
    ("no_lines", dict(kind="sparse", n=3000, m=3000, density=0.01), "max", 5, 0, dict(cand=False)),
    ("one_problem", dict(kind="sparse", n=2000, m=2000, density=0.01), "max", 1, 0, dict()),
    ("many_groups", dict(kind="sparse", n=1500, m=1500, density=0.02), "max", 40, 6, dict()),
    # one group of more problems than a kernel-argument block carries (at most 16): every merged launch goes through
    # the device ring of arguments (k_batched_ptr)
    ("device_ring", dict(kind="sparse", n=300, m=300, density=0.05, ints=4), "max", 20, 20, dict()),
]


@pytest.mark.parametrize("label,spec,prob,count,group,kw", _BATCH_CASES, ids=[c[0] for c in _BATCH_CASES])
def test_batched_solve_equals_the_single_solves(label, spec, prob, count, group, kw, gpu_lib):
    """misslap_solve_batch: many problems of one shape in lockstep -- the problems of a group share a HIP stream, and every
    launch of the solve loop that several of them issue at the same point is ONE launch (csrc/host_batch.hpp).  Each handle
    must end up exactly where its own misslap_solve leaves it: assignment, every meta key, fp64 objective, edge and bid
    counts, validity flags -- for different problems (seeds) of the shape, through every engine and stage of the loop."""
    from sslap_amd import solve_batch
    kw = dict(kw)
    max_iter = kw.pop("max_iter", 10**8)
    probs = [cases.synth_inputs(dict(spec, seed=31 + 7 * k)) for k in range(count)]
    mk = lambda loc, val: from_sparse(loc, val.copy(), problem=prob, cardinality_check=False, max_iter=max_iter, **kw)  # noqa: E731
    singles = []
    for loc, val in probs:
        s = mk(loc, val)
        sol = s.solve()
        singles.append((sol, dict(s.meta), dict(s.gpu)))
    solvers = [mk(loc, val) for loc, val in probs]
    sols, info = solve_batch(solvers, group)
    assert info["groups"] == -(-count // (group or 12)) and info["launches_issued"] <= info["calls_recorded"]
    if count >= 4 and (group or 12) >= 3:
        assert info["launches_issued"] < info["calls_recorded"]  # launches WERE shared
    for k in range(count):
        sol1, meta1, gpu1 = singles[k]
        assert np.array_equal(sols[k], sol1), (label, k)
        for key in cases.META_KEYS:
            assert solvers[k].meta[key] == meta1[key], (label, k, key)
        # (not cand_hits: WHICH rounds rebuild candidate lines depends on when the host saw which K -- an upper bound by
        # design -- so the number of bids a line answers may differ from run to run; what is bid, and the row lengths counted, never do)
        for key in ("obj_f64", "edges_scanned", "bids_made", "grid_rounds", "tail_rounds", "complete_assignment",
                    "valid_assignment", "tiled_active", "tiled_format", "eps_phases", "phases_with_lines"):
            assert solvers[k].gpu[key] == gpu1[key], (label, k, key)
    ref = orc.auction_solve(loc=probs[0][0], val=probs[0][1].copy(), problem=prob, cardinality_check=False, max_iter=max_iter)
    assert np.array_equal(sols[0], ref["sol"]) and solvers[0].meta["its"] == ref["meta"]["its"]
    # a handle is an ordinary handle again afterwards (its own stream, no recording)
    assert solvers[0].status().finished == 1


def test_batched_solve_of_problems_that_differ_in_objects_entries_layout_and_engine(gpu_lib):
    """The header's promise for a batch: same number of PERSONS; objects, entries, value layout and engine may differ.
    Merged launches run on the largest grid of the calls they merge, so a handle sees grids sized for ANOTHER problem's
    objects and entries in every kernel sized by them (k_apply, k_sync_from_rec, k_reset_phase, the eCE passes): each
    handle must still end exactly where its own misslap_solve leaves it.  One group holds a square sparse problem, a
    rectangular one with three times the objects, a dense one, a 12 B/edge one, one on the full-scan engine with shuffled
    rows, one without lines, and one problem that reaches its tail long before the others (tiny, eps_start = small)."""
    from sslap_amd import solve_batch
    n = 3000
    specs = [
        (dict(kind="sparse", n=n, m=n, density=0.01, seed=11), "max", dict()),
        (dict(kind="sparse", n=n, m=3 * n, density=0.004, seed=12), "min", dict()),
        (dict(kind="sparse", n=n, m=n + 700, density=0.08, seed=13), "max", dict()),                      # 300 edges per row
        (dict(kind="f64", n=n, density=0.01, seed=14), "max", dict()),                                   # 12 B/edge layout
        (dict(kind="shuffled", n=n, m=4 * n, density=0.004, ints=5, seed=15), "min", dict(tiled_min_k=1, engine=1)),
        (dict(kind="sparse", n=n, m=n, density=0.01, seed=16), "max", dict(cand=False)),
        (dict(kind="sparse", n=n, m=2 * n, density=0.003, seed=17), "max", dict(eps_start=1e-3)),          # one phase: at its tail at once
    ]
    probs = [cases.synth_inputs(sp) for sp, _, _ in specs]
    mk = lambda k: from_sparse(probs[k][0], probs[k][1].copy(), problem=specs[k][1], cardinality_check=False,  # noqa: E731
                               max_iter=10**8, **specs[k][2])
    singles = []
    for k in range(len(specs)):
        s1 = mk(k)
        sol = s1.solve()
        singles.append((sol, dict(s1.meta), dict(s1.gpu)))
    solvers = [mk(k) for k in range(len(specs))]
    sols, info = solve_batch(solvers, 12)  # one group
    assert info["groups"] == 1 and info["launches_issued"] < info["calls_recorded"]
    for k in range(len(specs)):
        sol1, meta1, gpu1 = singles[k]
        assert np.array_equal(sols[k], sol1), k
        for key in cases.META_KEYS:
            assert solvers[k].meta[key] == meta1[key], (k, key)
        for key in ("obj_f64", "edges_scanned", "bids_made", "grid_rounds", "tail_rounds", "complete_assignment",
                    "valid_assignment", "tiled_active", "tiled_format", "eps_phases", "phases_with_lines"):
            assert solvers[k].gpu[key] == gpu1[key], (k, key)
        ref = orc.auction_solve(loc=probs[k][0], val=probs[k][1].copy(), problem=specs[k][1], cardinality_check=False,
                                max_iter=10**8, **{a: b for a, b in specs[k][2].items() if a == "eps_start"})
        assert np.array_equal(sols[k], ref["sol"]) and solvers[k].meta["its"] == ref["meta"]["its"], k


def test_batched_solve_argument_checks(gpu_lib):
    from sslap_amd import solve_batch
    a = from_sparse(*synth.gen_sparse(500, 500, 0.03, seed=1), problem="max", cardinality_check=False)
    b = from_sparse(*synth.gen_sparse(600, 600, 0.03, seed=2), problem="max", cardinality_check=False)
    with pytest.raises(ValueError, match="same number of persons"):
        solve_batch([a, b])
    with pytest.raises(ValueError, match="appears twice"):
        solve_batch([a, a])
    c = from_sparse(*synth.gen_sparse(500, 500, 0.03, seed=3), problem="max", cardinality_check=False, profile=1)
    with pytest.raises(ValueError, match="profiled"):
        solve_batch([a, c])
    sols, _ = solve_batch([a])  # (the refused calls left the handles untouched)
    o = orc.from_sparse(*synth.gen_sparse(500, 500, 0.03, seed=1), problem="max", cardinality_check=False)
    assert np.array_equal(sols[0], o.solve())


def test_batched_solve_of_sixteen_c1_equals_the_fixture(golden_large, gpu_lib):
    """BASELINE config C1 sixteen times over (the reference's harness solves its problems in a loop,
    benchmarking.py:84-142): every assignment equals the reference fixture."""
    from sslap_amd import solve_batch
    g = golden_large["cases"]["C1"]
    loc, val = _config_arrays("C1")[:2]
    solvers = [from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8) for _ in range(16)]
    sols, info = solve_batch(solvers)
    assert all(synth.sol_digest(x) == g["sol_sha256"] for x in sols)
    assert all(s.meta["its"] == g["meta"]["its"] and s.gpu["obj_f64"] == g["obj_f64"] for s in solvers)
    assert info["launches_issued"] * 4 < info["calls_recorded"]


def test_no_kernel_depends_on_what_a_device_block_held_before(gpu_lib):
    """Device blocks come back from a cache, so whatever a kernel reads without anybody having written it is the
    previous handle's data -- or, in a fresh process, zeros, which hides the bug.  A fresh interpreter with
    MISSLAP_DEBUG_POISON=0xFF (every block handed out is filled with NaN / -1 patterns first) solves instances across the
    engines: the full-scan engine in every record format with 4 / 8 / 16 lanes per person on SHORT segments (the masked-off
    lanes of a wide lane group read far past a segment's end: the copy is followed by zeroed records for them), the
    wave-per-row kernel with and without lines, the fp32 filter, the tail kernels, dense rows -- all against the oracle."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"""
import sys
for p in ({root!r}, {os.path.join(root, 'tests')!r}, {os.path.join(root, 'tests', 'golden')!r}):
    sys.path.insert(0, p)
import numpy as np
import cases
from oracle import oracle as orc
from sslap_amd import from_sparse
n = 0
def check(spec, prob, **kw):
    global n
    loc, val = cases.synth_inputs(spec)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem=prob, cardinality_check=False, max_iter=10**7)
    s = from_sparse(loc, val.copy(), problem=prob, cardinality_check=False, max_iter=10**7, **kw)
    sol = s.solve()
    assert np.array_equal(sol, ref['sol']) and s.meta['its'] == ref['meta']['its'], (spec, kw)
    assert s.gpu['obj_f64'] == ref['extra']['obj_f64'] and s.meta['eCE'] == ref['meta']['eCE'], (spec, kw)
    n += 1
short = dict(kind='sparse', n=6000, m=40000, density=0.001)
for shape in (0, 8, 9):
    for fmt in (0, 1, 2, 3):
        spec = dict(short, kind='shuffled', ints=5) if fmt >= 2 else short
        for thr in (0, None):
            check(spec, 'max', tiled_min_k=1, engine=1, tiled_shape=shape, force_f64=bool(fmt & 1), tail_threshold=thr)
check(dict(kind='sparse', n=4200, m=12000, density=0.01), 'max', tiled_min_k=1, engine=1, tiled_shape=4)
for cand in (True, False):
    check(dict(kind='sparse', n=3000, m=3000, density=0.01), 'min', tiled_min_k=-1, cand=cand)
    check(dict(kind='f64', n=2500, density=0.01), 'max', tiled_min_k=-1, cand=cand, tail_threshold=0)
check(dict(kind='dense', n=600, m=600), 'max')
check(dict(kind='single', n=1500, density=0.02, n_single=40), 'min')
print('OK', n)
"""
    env = dict(os.environ, MISSLAP_DEBUG_POISON="0xFF", MISSLAP_F32_FILTER="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0 and "OK 31" in p.stdout, (p.stdout[-300:], p.stderr[-1500:])


def test_row_shuffled_c2_keeps_the_engine_and_matches_the_oracle(gpu_lib):
    """C2 with the stored order of every row randomly permuted: the full-scan engine stays on (record format 2, stored
    index carried), the result equals the oracle's on the same arrays."""
    loc, val = _config_arrays("C2")[:2]
    loc, val = cases._shuffle_within_rows(loc, val, 5)
    ref = orc.auction_solve(loc=loc, val=val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    s = from_sparse(loc, val.copy(), problem="max", cardinality_check=False, max_iter=10**8)
    sol = s.solve()
    assert s.gpu["tiled_active"] == 1 and s.gpu["tiled_format"] == 2
    assert np.array_equal(sol, ref["sol"]) and s.meta["its"] == ref["meta"]["its"]
    assert s.gpu["obj_f64"] == ref["extra"]["obj_f64"] and s.gpu["edges_scanned"] == ref["extra"]["edges_scanned"]
    assert s.meta["eCE"] == 1 and s.meta["soln_found"] == 1


def test_final_pass_grid_fits_its_result_slots_at_any_size(gpu_lib):
    """450 000 persons on the 16-lanes-per-person shape of the full-scan engine: the final pass (eCE / objective /
    validity flags on the engine) launches ceil(N / 208) = 2164 workgroups, more than the 2048 + N / 256 result slots the
    handle used to allocate -- misslap_finish then failed AFTER a complete solve.  Three rounds are enough to reach it."""
    n = 450_000
    loc, val = synth.gen_sparse(n, n, 16.0 / n, seed=11)
    s = from_sparse(loc, val, problem="max", cardinality_check=False, max_iter=3, tiled_min_k=1, tiled_shape=9, engine=1)
    sol = s.solve()
    assert s.gpu["tiled_active"] == 1 and s.meta["its"] == 3
    o = orc.from_sparse(loc, val.copy(), problem="max", max_iter=3, cardinality_check=False)
    assert np.array_equal(sol, o.solve())
    assert s.gpu["obj_f64"] == o.extra["obj_f64"] and s.gpu["edges_scanned"] == o.extra["edges_scanned"]


def test_measured_hbm_rates_and_device_uuid(gpu_lib):
    """misslap_measure_hbm (the 'measured peak' of bench.py's roofline): the library's own read-only and copy streaming
    kernels reach a plausible share of the 8 TB/s data sheet rate; misslap_device_uuid gives 32 hex digits."""
    import ctypes as C
    from sslap_amd import _lib
    rd, cp = C.c_double(), C.c_double()
    _lib.check(gpu_lib.misslap_measure_hbm(0, 1 << 29, 5, C.byref(rd), C.byref(cp)))
    assert 3000.0 < rd.value < 8000.0 and 3000.0 < cp.value < 8000.0
    buf = C.create_string_buffer(40)
    _lib.check(gpu_lib.misslap_device_uuid(0, buf, 40))
    assert len(buf.value) == 32 and int(buf.value, 16) >= 0
    with pytest.raises(ValueError):
        _lib.check(gpu_lib.misslap_device_uuid(0, buf, 8))
