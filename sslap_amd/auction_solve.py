"""Python front-end of the MI355X auction solver: same names, arguments, return values and error
behaviour as the reference's front-end, on top of libmisslap.so (include/misslap.h).

Mirrors  sslap/auction_solve.py:6-55      -> auction_solve(...)
         sslap/auction_.pyx:528-571       -> from_matrix(...)   (reference: _from_matrix)
         sslap/auction_.pyx:575-617       -> from_sparse(...)   (reference: _from_sparse)
         sslap/auction_.pyx:164-306       -> AuctionSolver(loc, val, ...).solve() / .meta

All solver arithmetic runs on the GPU; there is no CPU fallback.  The adapters' documented quirks
 are reproduced where they are observable and well defined: the `fast` epsilon and
the "fewer than N entries" guard use the adapter's own (mis)computed N, `val` is negated in place
for problem='min' on the loc/val and coo_mat entries, float32 `val` is rejected.
"""
import ctypes as C
import os

import numpy as np

from . import _lib

# environment defaults of the keyword options (everything else is a keyword only): the device, the tail threshold
# (__graft_entry__.smoke and the parity suite switch it), the launch shape of the engine (tools/ab_shapes*.sh)
_ENV_DEVICE = "MISSLAP_DEVICE"
_ENV_TAIL = "MISSLAP_TAIL_THRESHOLD"


def _options(problem, eps_start, max_iter, device=None, tail_threshold=None, profile=None, force_f64=False,
             input_on_device=False, shard=None, rounds_per_sync=None, tiled_min_k=None, tiled_shape=None, shard_min_k=None,
             engine=None, cand=None, nnz_limit=None, cand_build_max_k=None, cand_refresh=None,
             input_stream=None):
    if problem not in ("min", "max"):
        # the reference treats every string other than 'min' as 'max' (auction_.pyx:236, :502)
        problem = "max" if problem != "min" else "min"
    o = _lib.Options()
    o.struct_size = C.sizeof(_lib.Options)
    o.device = int(os.environ.get(_ENV_DEVICE, 0)) if device is None else int(device)
    o.maximize = 1 if problem == "max" else 0
    o.eps_start = float(np.float32(eps_start))
    o.max_iter = int(max_iter)
    o.input_on_device = 1 if input_on_device else 0
    # the hipStream_t that produced device-resident inputs (None: the library waits for the whole device instead)
    o.input_stream = None if input_stream is None else C.c_void_p(int(input_stream))
    o.tail_threshold = int(os.environ.get(_ENV_TAIL, -1)) if tail_threshold is None else int(tail_threshold)
    o.force_f64_values = 1 if force_f64 else 0
    o.profile = 0 if profile is None else int(profile)
    o.rounds_per_sync = 0 if rounds_per_sync is None else int(rounds_per_sync)
    if shard is not None:
        o.shard_rank, o.shard_world = int(shard[0]), int(shard[1])
    o.tiled_min_K = 0 if tiled_min_k is None else int(tiled_min_k)  # 0 default, < 0 never the LDS-tiled engine, > 0 minimum K
    # launch shape of k_bid_tiled: None / env unset = chosen by the library; k = shape k of misslap.hip:kTiledShapes
    shape = os.environ.get("MISSLAP_TILED_SHAPE") if tiled_shape is None else tiled_shape
    o.tiled_shape = 0 if shape is None else int(shape) + 1
    o.tiled_force = 0 if engine is None else int(engine)
    o.shard_min_K = 0 if shard_min_k is None else int(shard_min_k)
    # candidate lines (per-person exact bid shortcut, csrc/device_common.hpp): on by default, 0 = off (A/B runs),
    # 2 = lines without the maintenance pass ahead of the tail kernels
    c = 1 if cand is None else int(cand)
    o.cand_mode = 1 if c == 0 else (2 if c == 2 else 0)
    o.partial_in_list_order = 0  # (ignored by the library since round 6)
    o.cand_build_max_K = 0 if cand_build_max_k is None else int(cand_build_max_k)
    # k_bid rebuilds a line that hits with fewer live candidates than this (None = library default)
    o.cand_refresh_min = 0 if cand_refresh is None else int(cand_refresh) + 1
    o.nnz_limit = 0 if nnz_limit is None else int(nnz_limit)  # tests of the int32 row-pointer guard
    return o


class AuctionSolver:
    """GPU-resident auction solver (reference: cdef class AuctionSolver, auction_.pyx:164-523).

    `loc` is int32[nnz, 2] with rows ascending and no empty row, `val` is float64[nnz].  As in the
    reference the constructor's num_rows / num_cols are ignored: N, M come from `loc` (:209-212).
    """

    def __init__(self, loc, val, num_rows=0, num_cols=0, problem="min", max_iter=1000000, eps_start=0,
                 **gpu_opts):
        lib = _lib.load()
        loc, val = self._check_buffers(loc, val)
        self._h = C.c_void_p()
        self._opts = _options(problem, eps_start, max_iter, **gpu_opts)
        self._problem = problem
        loc_c = np.ascontiguousarray(loc)
        val_c = np.ascontiguousarray(val)
        _lib.check(lib.misslap_create(C.byref(self._h), loc_c.shape[0], loc_c.ctypes.data, val_c.ctypes.data,
                                      C.byref(self._opts)))
        if problem == "min":
            # the reference negates the caller's buffer in place (mult_ndarray_by, auction_.pyx:236-237)
            np.multiply(val, -1, out=val)
        self._post_create()

    # -- alternative constructors -------------------------------------------------------------
    @classmethod
    def _from_handle(cls, handle, opts, problem):
        self = cls.__new__(cls)
        self._h, self._opts, self._problem = handle, opts, problem
        self._post_create()
        return self

    @classmethod
    def from_dense(cls, mat, problem="min", max_iter=1000000, eps_start=0, **gpu_opts):
        """Dense (N, M) float64 matrix, entries < 0 invalid: the `v >= 0` scan of auction_.pyx:546-557
        runs on the GPU.  Returns (solver, number_of_valid_entries)."""
        lib = _lib.load()
        h = C.c_void_p()
        opts = _options(problem, eps_start, max_iter, **gpu_opts)
        matc = np.ascontiguousarray(mat)
        nnz = C.c_int64(-1)
        rc = lib.misslap_create_dense(C.byref(h), matc.shape[0], matc.shape[1], matc.ctypes.data, C.byref(opts),
                                      C.byref(nnz))
        return rc, h, opts, int(nnz.value)

    @classmethod
    def from_device_pointers(cls, loc_ptr, val_ptr, nnz, problem="min", max_iter=1000000, eps_start=0,
                             **gpu_opts):
        """COO input already resident in HBM (loc int32[nnz,2], val float64[nnz] device pointers)."""
        lib = _lib.load()
        h = C.c_void_p()
        opts = _options(problem, eps_start, max_iter, input_on_device=True, **gpu_opts)
        _lib.check(lib.misslap_create(C.byref(h), int(nnz), C.c_void_p(int(loc_ptr)), C.c_void_p(int(val_ptr)),
                                      C.byref(opts)))
        return cls._from_handle(h, opts, problem)

    @staticmethod
    def _check_buffers(loc, val):
        # Cython buffer checks of auction_.pyx:202 (np.ndarray[DTYPE_int_t, ndim=2], np.ndarray[DTYPE_t, ndim=1])
        if not isinstance(loc, np.ndarray) or not isinstance(val, np.ndarray):
            raise TypeError("loc and val must be numpy arrays")
        if loc.ndim != 2:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 2, got {loc.ndim})")
        if loc.dtype != np.int32:
            raise ValueError(f"Buffer dtype mismatch, expected 'DTYPE_int_t' but got '{loc.dtype.name}'")
        if val.ndim != 1:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {val.ndim})")
        if val.dtype != np.float64:
            raise ValueError(f"Buffer dtype mismatch, expected 'DTYPE_t' but got '{_cname(val.dtype)}'")
        if loc.shape[1] != 2 or loc.shape[0] != val.shape[0]:
            raise ValueError("loc must have shape (nnz, 2) and val shape (nnz,)")
        return loc, val

    def _post_create(self):
        lib = _lib.load()
        n, m, z = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(lib.misslap_dims(self._h, C.byref(n), C.byref(m), C.byref(z)))
        self.num_rows, self.num_cols, self.nnz = n.value, m.value, z.value
        st = self.status()
        self.tail_threshold, self.rounds_per_sync = int(st.tail_threshold), int(st.rounds_per_sync)
        self.shard_min_K = int(st.shard_min_K)
        self.meta = {"start_eps": round(float(st.eps), 3)}  # auction_.pyx:264
        self.gpu = {}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.load().misslap_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- reference API ---------------------------------------------------------------------------
    def solve(self):
        """Run the auction (auction_.pyx:268-306); returns person_to_object as int32[N]."""
        lib = _lib.load()
        sol = np.empty(self.num_rows, dtype=np.int32)
        meta = _lib.new_meta()
        _lib.check(lib.misslap_solve(self._h, sol.ctypes.data, C.byref(meta)))
        self._fill_meta(meta)
        return sol

    @staticmethod
    def solve_batch(solvers, group_size=0):
        """Solve many independent problems with the same number of persons (rows) in lockstep (misslap_solve_batch: the problems of a group share a
        HIP stream and every launch of the solve loop that several of them issue at the same point is one launch).  Every
        solver ends up exactly as after its own `.solve()` -- same assignment, same meta, bit for bit.  Returns
        (list of person_to_object arrays, info dict: groups, calls_recorded, launches_issued, wall_ms)."""
        lib = _lib.load()
        n = len(solvers)
        sols = [np.empty(s.num_rows, dtype=np.int32) for s in solvers]
        handles = (C.c_void_p * n)(*[s._h for s in solvers])
        outs = (C.c_void_p * n)(*[a.ctypes.data for a in sols])
        metas = (_lib.Meta * n)()
        for m in metas:
            m.struct_size = C.sizeof(_lib.Meta)
        info = _lib.BatchInfo()
        meta_ptrs = (C.POINTER(_lib.Meta) * n)(*[C.pointer(m) for m in metas])
        _lib.check(lib.misslap_solve_batch(handles, n, outs, meta_ptrs, int(group_size), C.byref(info)))
        for s, m in zip(solvers, metas):
            s._fill_meta(m)
        return sols, dict(groups=int(info.groups), calls_recorded=int(info.calls_recorded),
                          launches_issued=int(info.launches_issued), wall_ms=float(info.wall_ms),
                          host_ms=dict(fibers=round(float(info.host_ms_fibers), 3), flush=round(float(info.host_ms_flush), 3),
                                       wait=round(float(info.host_ms_wait), 3)))

    def solve_sharded(self, comm=None):
        """The same solve over the ranks of a communicator (sslap_amd.dist.Comm): persons of the big rounds sharded,
        per-object arg-max exchanged on the solver's stream inside the library (misslap_solve_sharded)."""
        lib = _lib.load()
        sol = np.empty(self.num_rows, dtype=np.int32)
        meta = _lib.new_meta()
        _lib.check(lib.misslap_solve_sharded(self._h, comm._c if comm is not None else None, sol.ctypes.data,
                                             C.byref(meta)))
        self._fill_meta(meta)
        return sol

    def _fill_meta(self, m):
        # auction_.pyx:297-304 (and :264: the eps0 of this solve -- after update_values or resolve not that of create)
        self.meta["start_eps"] = round(float(m.start_eps), 3)
        self.meta["eCE"] = int(m.eCE)
        self.meta["its"] = int(m.its)
        self.meta["nreductions"] = int(m.nreductions)
        self.meta["soln_found"] = int(m.soln_found)
        self.meta["n_assigned"] = int(m.n_assigned)
        self.meta["obj"] = round(float(m.obj_f32), 3)
        self.meta["final_eps"] = round(float(m.final_eps), 3)
        self.meta["timer"] = {"setup": f"{m.setup_ms:.2f}ms", "solve": f"{m.solve_ms:.2f}ms"}
        g = dict(obj_f64=float(m.obj_f64), edges_scanned=int(m.edges_scanned), bids_made=int(m.bids_made),
                 grid_rounds=int(m.grid_rounds), tail_rounds=int(m.tail_rounds), bytes_per_edge=int(m.bytes_per_edge),
                 setup_ms=float(m.setup_ms), solve_ms=float(m.solve_ms), final_eps_f32=float(m.final_eps),
                 start_eps_f32=float(m.start_eps), tail_edges=int(m.tail_edges), shard_edges=int(m.shard_edges),
                 tiled_active=int(m.tiled_active), tiled_min_K=int(m.tiled_min_K),
                 cand_hits=int(m.cand_hits), cand_edges=int(m.cand_edges), lines_active=int(m.lines_active),
                 sharded_rounds=int(m.sharded_rounds), tiled_format=int(m.tiled_format),
                 phases_with_lines=int(m.phases_with_lines), eps_phases=int(m.eps_phases),
                 filter_undecided=int(m.filter_undecided),
                 # validity of the assignment as the reference's benchmark harness forms it (benchmarking.py:56-64),
                 # reduced on the device: (np.unique(sol).size == N, (sol >= 0).all(), (sol < N).all()), and
                 # (mat[arange(N), sol] >= 0).all()
                 complete_assignment=tuple(bool(m.complete_assignment >> k & 1) for k in range(3)),
                 valid_assignment=bool(m.valid_assignment))
        d = [float(x) for x in m.tail_stats]
        g["tail_modes"] = {name: dict(rounds=int(d[k]), ms=round(d[3 + k] * 1e-5, 3),
                                      us_per_round=round(d[3 + k] * 1e-2 / d[k], 3) if d[k] else None)
                           for k, name in enumerate(("solo", "team", "block"))}
        g["tail_modes"]["block"]["clean_rounds"] = int(d[10])
        g["tail_cand"] = dict(bids=int(d[6]), hits=int(d[7]), builds=int(d[8]))
        g["tail_cand_edges"] = int(d[9])
        g["tail_raw"] = d[:6]  # (diagnostic MISSLAP_TAIL_STAMP builds: cycles per segment of a solo round)
        if m.profiled:
            g.update(bid_launches=int(m.bid_launches), bid_ms=float(m.bid_ms), bid_edges=int(m.bid_edges),
                     fullscan_launches=int(m.fullscan_launches), fullscan_ms=float(m.fullscan_ms),
                     fullscan_edges=int(m.fullscan_edges), tail_launches=int(m.tail_launches),
                     tail_ms=float(m.tail_ms), tiled_launches=int(m.tiled_launches), tiled_ms=float(m.tiled_ms),
                     tiled_edges=int(m.tiled_edges), bid_edges_read=int(m.bid_edges_read),
                     fullscan_edges_read=int(m.fullscan_edges_read))
        self.gpu = g
        self.meta["gpu"] = g

    # -- warm-started re-solve (no counterpart in the reference; include/misslap.h: misslap_resolve) -------------------
    # Prices are those of the maximised problem (for problem='min' the prices of the negated costs), out and in alike.
    @property
    def prices(self):
        """The current prices, float64[num_cols]."""
        p = np.empty(self.num_cols, dtype=np.float64)
        _lib.check(_lib.load().misslap_get_prices(self._h, p.ctypes.data, 0))
        return p

    def update_values(self, val):
        """Replace the values of the handle's entries in place: a 1-D float64 array of `nnz` values in the order of the
        constructor's `loc`, or for a solver made by `from_matrix` an (N, M) float64 matrix with the same `v >= 0`
        pattern.  Values are in the caller's sign and the caller's array is not written (unlike the constructor, there is
        no reference quirk to mirror).  All or nothing: a rejected update leaves the handle unchanged.  Returns
        max |new - old| in cost units, the natural `eps_start` of the next `resolve`."""
        if not isinstance(val, np.ndarray):
            raise TypeError("val must be a numpy array")
        if val.dtype != np.float64:
            raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(val.dtype)}'")
        delta = C.c_double(0.0)
        if val.ndim == 2:
            shape = getattr(self, "_dense_shape", None)
            if shape is None:
                raise ValueError("an (N, M) matrix updates a solver made by from_matrix only; pass the nnz values instead")
            if val.shape != shape:
                raise ValueError(f"matrix of shape {val.shape}, the solver was made from one of shape {shape}")
            v = np.ascontiguousarray(val)
            if np.isposinf(v).any():  # (NaN and negative entries are invalid ones, as in from_matrix)
                raise ValueError("the matrix holds +inf")
            _lib.check(_lib.load().misslap_update_dense(self._h, v.ctypes.data, 0, None, C.byref(delta)))
            return float(delta.value)
        if val.ndim != 1:
            raise ValueError(f"Buffer has wrong number of dimensions (expected 1, got {val.ndim})")
        if val.shape[0] != self.nnz:
            raise ValueError(f"{val.shape[0]} values given, the solver holds {self.nnz} entries")
        v = np.ascontiguousarray(val)
        if not np.isfinite(v).all():
            raise ValueError("val holds a NaN or an infinity")
        _lib.check(_lib.load().misslap_update_values(self._h, v.ctypes.data, self.nnz, 0, None, C.byref(delta)))
        return float(delta.value)

    def update_values_device(self, ptr, input_stream=None, dense=False):
        """update_values on values already in HBM: `ptr` is a device pointer to nnz float64 values (or, dense=True, to the
        (N, M) matrix of a from_matrix solver), produced on the hipStream_t `input_stream` (None: the library waits for
        the whole device).  Checked on the device only."""
        delta = C.c_double(0.0)
        stream = None if input_stream is None else C.c_void_p(int(input_stream))
        lib = _lib.load()
        if dense:
            _lib.check(lib.misslap_update_dense(self._h, C.c_void_p(int(ptr)), 1, stream, C.byref(delta)))
        else:
            _lib.check(lib.misslap_update_values(self._h, C.c_void_p(int(ptr)), self.nnz, 1, stream, C.byref(delta)))
        return float(delta.value)

    def resolve(self, prices=None, eps_start=0):
        """Solve again from `prices` (float64[num_cols], a numpy array or a tensor on the device; None: the current
        prices) with every person unassigned and eps0 = eps_start if > 0, else C / 2 of the current values.  Returns
        person_to_object and refreshes self.meta like solve()."""
        e = float(eps_start)
        if e != e:
            raise ValueError("eps_start is NaN")
        ptr, on_device = None, 0
        if prices is not None:
            if isinstance(prices, np.ndarray):
                if prices.dtype != np.float64:
                    raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(prices.dtype)}'")
                p = np.ascontiguousarray(prices)
                bad_nan, bad_sign = not np.isfinite(p).all(), bool(np.signbit(p).any())
                ptr = p.ctypes.data
            elif hasattr(prices, "data_ptr") and getattr(prices, "is_cuda", False):  # a torch tensor in HBM
                import torch
                if prices.dtype != torch.float64:
                    raise ValueError(f"prices must be float64, got {prices.dtype}")
                p = prices.contiguous()
                bad_nan, bad_sign = not bool(torch.isfinite(p).all()), bool(torch.signbit(p).any())
                ptr, on_device = p.data_ptr(), 1
            else:
                raise TypeError("prices must be a numpy array or a tensor on the device")
            if p.ndim != 1 or p.shape[0] != self.num_cols:
                raise ValueError(f"prices must have shape ({self.num_cols},), got {tuple(p.shape)}")
            if bad_nan:
                raise ValueError("prices hold a NaN or an infinity")
            if bad_sign:
                raise ValueError("prices must be >= 0 (with the sign bit clear: -0.0 is rejected)")
        lib = _lib.load()
        sol = np.empty(self.num_rows, dtype=np.int32)
        meta = _lib.new_meta()
        _lib.check(lib.misslap_resolve(self._h, None if ptr is None else C.c_void_p(ptr), on_device, float(np.float32(e)),
                                       sol.ctypes.data, C.byref(meta)))
        self._fill_meta(meta)
        return sol

    # -- stepwise API (tests, multi-GPU driver) ----------------------------------------------------
    def status(self):
        st = _lib.Status()
        _lib.check(_lib.load().misslap_get_status(self._h, C.byref(st)))
        return st

    def state(self):
        """Snapshot dict(K, U[:K], p, p2o, o2p, eps, its) of the device state."""
        st = self.status()
        p = np.empty(self.num_cols, dtype=np.float64)
        U = np.empty(self.num_rows, dtype=np.int32)
        p2o = np.empty(self.num_rows, dtype=np.int32)
        o2p = np.empty(self.num_cols, dtype=np.int32)
        _lib.check(_lib.load().misslap_get_state(self._h, p.ctypes.data, U.ctypes.data, p2o.ctypes.data,
                                                 o2p.ctypes.data))
        return dict(K=int(st.K), U=U[:st.K].copy(), p=p, p2o=p2o, o2p=o2p, eps=float(st.eps), its=int(st.its),
                    nreductions=int(st.nreductions))

    def round_bid(self):
        _lib.check(_lib.load().misslap_round_bid(self._h))

    def round_tiebreak(self):
        _lib.check(_lib.load().misslap_round_tiebreak(self._h))

    def round_apply(self):
        _lib.check(_lib.load().misslap_round_apply(self._h))

    def run_tail(self):
        _lib.check(_lib.load().misslap_run_tail(self._h))

    def phase_end(self):
        fin = C.c_int32(0)
        _lib.check(_lib.load().misslap_phase_end(self._h, C.byref(fin)))
        return bool(fin.value)

    def check_ece(self, eps):
        ok = C.c_int32(0)
        _lib.check(_lib.load().misslap_check_ece(self._h, float(np.float32(eps)), C.byref(ok)))
        return bool(ok.value)

    def finish(self):
        sol = np.empty(self.num_rows, dtype=np.int32)
        meta = _lib.new_meta()
        _lib.check(_lib.load().misslap_finish(self._h, sol.ctypes.data, C.byref(meta)))
        self._fill_meta(meta)
        return sol

    def exchange_buffers(self):
        k, p, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(_lib.load().misslap_exchange_buffers(self._h, C.byref(k), C.byref(p), C.byref(n)))
        return k.value, p.value, n.value

    def matching_cardinality(self):
        """Size of a maximum matching of the handle's graph (GPU matcher on the device-resident CSR): the feasibility
        guard of the front-end (auction_.pyx:562-566, :608-612) without a host copy of the entries."""
        size = C.c_int32()
        _lib.check(_lib.load().misslap_matching_of(self._h, C.byref(size), None))
        return int(size.value)

    def set_stream(self, hip_stream):
        _lib.check(_lib.load().misslap_set_stream(self._h, C.c_void_p(int(hip_stream))))


def _cname(dt):
    return {"float32": "float", "float64": "double", "int64": "long", "int32": "int"}.get(dt.name, dt.name)


def _cardinality(loc, n_rows, n_cols):
    """Maximum-matching cardinality for the optional feasibility guard (reference: c_hopcroft_solve,
    feasibility_.pyx:95-225, called at auction_.pyx:562-566 / :608-612).  Only the cardinality reaches
    the auction path; the matching runs in the library (host C++ Hopcroft-Karp)."""
    from .check_feasible import cardinality, matching_gpu
    # large graphs: the BFS-layered GPU matcher (same cardinality); small ones are faster on the host
    if loc.shape[0] >= int(os.environ.get("MISSLAP_MATCHING_GPU_MIN_NNZ", 2_000_000)):
        return matching_gpu(loc, n_rows, n_cols)["size"]
    return cardinality(loc, n_rows, n_cols)


def from_matrix(mat, problem="min", eps_start=0, max_iter=1000000, fast=False, cardinality_check=True,
                **gpu_opts):
    """AuctionSolver from a dense (N, M) matrix where invalid entries are -1 (auction_.pyx:528-571)."""
    if not isinstance(mat, np.ndarray):
        raise TypeError("Argument 'mat' has incorrect type (expected numpy.ndarray)")
    if mat.ndim != 2:
        raise ValueError(f"Buffer has wrong number of dimensions (expected 2, got {mat.ndim})")
    if mat.dtype != np.float64:  # `cdef double[:, :] matmv = mat` (:544)
        raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(mat.dtype)}'")
    N, M = mat.shape
    if fast:
        eps_start = 1 / N  # :568-569, converted to C float by _options
    rc, h, opts, ctr = AuctionSolver.from_dense(mat, problem=problem, max_iter=max_iter, eps_start=eps_start,
                                                **gpu_opts)
    if rc != 0 and 0 <= ctr < N:  # :559-560
        raise ValueError(f"Matrix is infeasible - Fewer than {N} valid values provided for {N} rows.")
    _lib.check(rc)
    solver = AuctionSolver._from_handle(h, opts, problem)
    solver._dense_shape = (N, M)  # (update_values takes an (N, M) matrix)
    if cardinality_check:  # :562-566, on the CSR the handle already holds in device memory
        cardinality = solver.matching_cardinality()
        if cardinality < N:
            raise ValueError(f"Matrix is infeasible (Maximum matching possible only involves {cardinality} "
                             f"out of {N} rows.)")
    return solver


def from_sparse(loc, val, problem="min", eps_start=0, max_iter=1000000, fast=False, size=None,
                cardinality_check=True, **gpu_opts):
    """AuctionSolver for sparse entries (auction_.pyx:575-617).

    loc: (nnz, 2) integer (i, j) indices, rows ascending; val: (nnz,) float64.  N and M of the
    guard / `fast` epsilon are computed exactly like the reference does (:591-595), quirks included.
    """
    if size is not None:
        M, N = size  # sic, :592
    else:
        N = int(loc[:, 0].max())  # sic (no +1), :594
        M = int(loc[:, 1].max())
    num_entries = loc.shape[0]
    loc_long = loc.astype(np.int32)  # :601
    if num_entries < N:  # :604-605
        raise ValueError(f"Matrix is infeasible - Fewer than {N} valid values provided for {N} rows.")
    if fast:
        eps_start = 1 / N  # :614-615 (nothing before this line depends on it)
    if cardinality_check:  # :608-612 (on the true graph; the reference indexes out of bounds here)
        n_true, m_true = int(loc_long[:, 0].max()) + 1, int(loc_long[:, 1].max()) + 1
        failed = None
        if num_entries >= int(os.environ.get("MISSLAP_MATCHING_GPU_MIN_NNZ", 2_000_000)):
            # large graphs: the handle first, then the GPU matcher on the CSR it holds in device memory -- the entries
            # are uploaded once.  A constructor error is kept until the guard (which the reference runs first) has spoken.
            try:
                solver = AuctionSolver(loc_long, val, problem=problem, eps_start=eps_start, max_iter=max_iter, **gpu_opts)
            except ValueError as e:
                failed = e
            else:
                cardinality = solver.matching_cardinality()
                if cardinality < n_true:
                    raise ValueError(f"Matrix is infeasible (Maximum matching possible only involves {cardinality} "
                                     f"out of {n_true} rows.)")
                return solver
        cardinality = _cardinality(loc_long, n_true, m_true)
        if cardinality < n_true:
            raise ValueError(f"Matrix is infeasible (Maximum matching possible only involves {cardinality} "
                             f"out of {n_true} rows.)")
        if failed is not None:
            raise failed
    return AuctionSolver(loc_long, val, problem=problem, eps_start=eps_start, max_iter=max_iter, **gpu_opts)


# the reference's private names
_from_matrix = from_matrix
_from_sparse = from_sparse


def auction_solve(mat=None, loc=None, val=None, coo_mat=None, problem="min", eps_start=0., max_iter=1000000,
                  fast=False, size=None, cardinality_check=True):
    """Solve an Auction Algorithm problem (drop-in for sslap.auction_solve, sslap/auction_solve.py:6-55).

    Input, one of: `mat` (N x M ndarray, -1 = no edge), (`loc`, `val`) sparse triplets, or `coo_mat`
    (scipy COO matrix).  Returns dict(sol=int32[N] assignment i -> j, meta=dict).
    """
    kw = dict(problem=problem, eps_start=eps_start, max_iter=max_iter, fast=fast, cardinality_check=cardinality_check)
    if mat is not None:
        solver = from_matrix(mat=mat, **kw)
    elif loc is not None and val is not None:
        solver = from_sparse(loc=loc, val=val, size=size, **kw)
    elif coo_mat is not None:
        row, col = coo_mat.row, coo_mat.col
        loc, val, size = np.stack([row, col], axis=-1), coo_mat.data, coo_mat.shape
        solver = from_sparse(loc=loc, val=val, size=size, **kw)
    else:
        raise ValueError("One of the following formats is expected as input to auction solve: "
                         "mat OR (loc & val) OR coo_mat.")
    sol = solver.solve()
    return dict(sol=sol, meta=solver.meta)
