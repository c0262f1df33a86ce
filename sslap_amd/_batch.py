"""Plumbing shared by the one-workgroup-per-problem wrappers: dense_batch, sparse_batch, ell_batch and matching_batch.

Argument checks that raise before the library is called, the options of the call, the arrays of either side (`_empty`,
`_ptr`, `_send`), the outputs and the argument tail of a status-mode call (`_StatusCall`), the decoding of its
per-problem records, and what takes a status-mode result of any layout: batch_meta_to_host and raise_for_status.  The
library is reached through `_lib.load()` at call time, never through a name bound here; torch is imported where a
device tensor is at hand, never with the package.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from .auction_solve import _ENV_DEVICE, _cname


def _is_device_tensor(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _empty(shape, dtype, dev=None):
    """An uninitialised array of a numpy dtype: a numpy array on the host (dev None), else a tensor on dev."""
    if dev is None:
        return np.empty(shape, dtype=dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)


def _ptr(x):
    """The address of a numpy array or of a tensor; None for None."""
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def _contiguous(x):
    """x as the library reads it, row after row: a numpy array or a tensor, the same object where it already is; None
    for None."""
    if x is None:
        return None
    return np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x.contiguous()


def _send(a, dev):
    """A host array to dev from pinned memory, on the current stream of dev and without a wait (torch takes no
    read-only array: a copy then).  None and a device tensor pass through, and so does everything with host input (dev
    None)."""
    if dev is None or not isinstance(a, np.ndarray):
        return a
    import torch
    with torch.cuda.device(dev):
        return torch.from_numpy(a if a.flags.writeable else a.copy()).pin_memory().to(dev, non_blocking=True)


def _eps(eps_start):
    e = float(eps_start)
    if e != e:
        raise ValueError("eps_start is NaN")
    return e


# mat_dtype: the element types a dense stack may have (MISSLAP_DTYPE_* of include/misslap.h)
_MAT_DTYPES = {"float64": _lib.DTYPE_F64, "float32": _lib.DTYPE_F32, "float16": _lib.DTYPE_F16,
               "bfloat16": _lib.DTYPE_BF16}


def _mat_dtype_name(mat_dtype):
    """The name of a mat_dtype keyword: one of the four names, or the numpy / torch dtype object of one."""
    if isinstance(mat_dtype, str):
        name = mat_dtype
    elif type(mat_dtype).__module__.split(".")[0] == "torch":
        name = str(mat_dtype).split(".")[-1]
    elif isinstance(mat_dtype, (np.dtype, type)):  # (np.dtype(None) is float64: only a dtype or a scalar type names one)
        try:
            name = np.dtype(mat_dtype).name
        except TypeError:
            name = repr(mat_dtype)
    else:
        name = repr(mat_dtype)
    if name not in _MAT_DTYPES:
        raise ValueError(f"mat_dtype must be one of {', '.join(_MAT_DTYPES)} (or that numpy / torch dtype), got {mat_dtype!r}")
    return name


_ENTRIES = ("nonneg", "finite")


def _entries_flag(entries):
    """The entries= keyword of the dense calls as the bits it adds to mat_dtype: "nonneg" (v >= 0 is an entry, today's
    rule) adds none, "finite" (every element that is not a NaN is one) adds MISSLAP_DENSE_ENTRIES_FINITE."""
    if not isinstance(entries, str) or entries not in _ENTRIES:
        raise ValueError(f"entries must be 'nonneg' or 'finite', got {entries!r}")
    return _lib.DENSE_ENTRIES_FINITE if entries == "finite" else 0


def _check_stack(mats, mat_dtype="float64"):
    """dtype and rank of a (B, N, M) stack of mat_dtype (numpy array or device tensor); returns (B, N, M, on_device,
    the MISSLAP_DTYPE_* code).  The stack must have exactly that dtype: nothing is converted.  A device tensor may have
    any strides (_stack_strides).  The cap is the caller's check."""
    want = _mat_dtype_name(mat_dtype)
    if isinstance(mats, np.ndarray):
        on_device = False
        if mats.ndim != 3:
            raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.ndim}")
        if mats.dtype != np.float64 and want == "float64":
            raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(mats.dtype)}'")
        if mats.dtype.name != want:
            raise ValueError(f"Buffer dtype mismatch, expected '{want}' (mat_dtype) but got '{mats.dtype.name}'")
    elif _is_device_tensor(mats):
        import torch
        on_device = True
        if mats.dim() != 3:
            raise ValueError(f"mats must have 3 dimensions (B, N, M), got {mats.dim()}")
        if mats.dtype != torch.float64 and want == "float64":
            raise ValueError(f"mats must be float64, got {mats.dtype}")
        if mats.dtype != getattr(torch, want):
            raise ValueError(f"mats dtype mismatch: mat_dtype is {want}, the tensor is {mats.dtype}")
    else:
        raise TypeError("mats must be a numpy array or a tensor on the device")
    B, N, M = (int(d) for d in mats.shape)
    if B < 1 or N < 1 or M < 1:
        raise ValueError(f"empty stack of shape {(B, N, M)}")
    return B, N, M, on_device, _MAT_DTYPES[want]


def _stack_strides(mats, on_device):
    """The element strides (sB, sN, sM) of a non-contiguous device stack, which the strided entry points read in place;
    None for a contiguous tensor and for a numpy array (uploaded through np.ascontiguousarray): today's entry points."""
    if not on_device or mats.is_contiguous():
        return None
    return tuple(int(x) for x in mats.stride())  # (torch has no negative strides; expand gives 0)


def _check_shapes(shapes, B, N, M, what):
    """Optional integer (B, 2) shapes within the stack; returns them as int32 or None.  what: "problem" / "graph"."""
    if shapes is None:
        return None
    s = np.asarray(shapes)
    if s.shape != (B, 2) or not np.issubdtype(s.dtype, np.integer):
        raise ValueError(f"shapes must be an integer array of shape ({B}, 2), got {s.dtype} {s.shape}")
    bad = (s[:, 0] < 1) | (s[:, 0] > N) | (s[:, 1] < 1) | (s[:, 1] > M)
    if bad.any():
        b = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{what} {b}: shape ({int(s[b, 0])}, {int(s[b, 1])}) outside 1 .. {N} x 1 .. {M}")
    return np.ascontiguousarray(s, dtype=np.int32)


def _check_device_shapes(shp, B, dev):
    """A device shapes tensor of a status-mode call: contiguous int32 (B, 2) on the stack's device.  Its values are the
    library's to judge."""
    import torch
    if shp.dtype != torch.int32 or tuple(shp.shape) != (B, 2) or shp.device != dev or not shp.is_contiguous():
        raise ValueError(f"a device shapes tensor must be contiguous int32 of shape ({B}, 2) on {dev}, got "
                         f"{shp.dtype} {tuple(shp.shape)} on {shp.device}")
    return shp


def _scalar_outside(outside, B, dev, nonneg=False):
    """One finite float as the outside value of every row: float64 (B,) where the input lives (a fill on dev, nothing
    is sent).  nonneg: it must also be >= 0 (the dense batch, where a negative entry is an absent one)."""
    if isinstance(outside, (bool, str, bytes)) or not isinstance(outside, (int, float, np.integer, np.floating)):
        raise TypeError("outside must be a float, a float64 numpy array or a float64 tensor on the device")
    x = float(outside)
    if not np.isfinite(x):
        raise ValueError(f"outside must be finite, got {x!r}")
    if nonneg and not x >= 0:
        raise ValueError(f"outside must be >= 0 (a negative entry of a dense matrix is an absent one), got {x!r}")
    if dev is not None:
        import torch
        return torch.full((B,), x, dtype=torch.float64, device=dev)
    return np.full(B, x, dtype=np.float64)


def _check_outside(outside, B, N, dev, need="cols / vals", src="cols", nonneg=False):
    """The outside values of a dense or an ELL call: a finite float (_scalar_outside), or float64 (B,) / (B, N) on the
    host or (with device input, dev) contiguous on the input's device.  Returns (array or tensor, outside_ld); the
    values are the library's to judge.  need / src: what the input is called in the texts."""
    if _is_device_tensor(outside):
        import torch
        if dev is None:
            raise TypeError(f"outside on the device needs {need} on the device")
        if outside.dtype != torch.float64:
            raise ValueError(f"outside must be float64, got {outside.dtype}")
        if tuple(outside.shape) not in ((B,), (B, N)):
            raise ValueError(f"outside must have shape ({B},) or ({B}, {N}), got {tuple(outside.shape)}")
        if outside.device != dev:
            raise ValueError(f"outside is on {outside.device}, {src} on {dev}")
        if not outside.is_contiguous():
            raise ValueError("a device outside tensor must be contiguous (it is read in place)")
        return outside, (N if outside.dim() == 2 else 0)
    if isinstance(outside, np.ndarray):
        if outside.dtype != np.float64:
            raise ValueError(f"outside must be float64, got {outside.dtype.name}")
        if outside.shape not in ((B,), (B, N)):
            raise ValueError(f"outside must have shape ({B},) or ({B}, {N}), got {outside.shape}")
        return np.ascontiguousarray(outside), (N if outside.ndim == 2 else 0)
    return _scalar_outside(outside, B, dev, nonneg), 0


def _check_offsets(offsets, nnz, missing):
    """Host offsets of B problems over nnz packed entries; returns (B, offsets int64).  missing: the text without them."""
    if offsets is None:
        raise ValueError(missing)
    if _is_device_tensor(offsets):
        raise TypeError("offsets must be a host array")
    off = np.asarray(offsets)
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"offsets must be a 1-d integer array of length B + 1 >= 2, got {off.dtype} {off.shape}")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != nnz:
        raise ValueError(f"offsets must start at 0 and end at nnz = {nnz}, got {int(off[0])} .. {int(off[-1])}")
    if (np.diff(off) < 0).any():
        b = int(np.flatnonzero(np.diff(off) < 0)[0])
        raise ValueError(f"offsets must be non-decreasing (offsets[{b}] > offsets[{b + 1}])")
    return off.shape[0] - 1, np.ascontiguousarray(off)


def _check_device_offsets(offsets, dev):
    """Offsets that a device pipeline left on the device: a contiguous int64 tensor of shape (B + 1,) on dev, the device
    of loc / val.  Returns (B, the tensor).  Their values are the library's to judge, per problem: reading them here
    would be a wait."""
    import torch
    if (offsets.dtype != torch.int64 or offsets.dim() != 1 or int(offsets.shape[0]) < 2 or offsets.device != dev or
            not offsets.is_contiguous()):
        raise ValueError(f"device offsets must be a contiguous int64 tensor of shape (B + 1,) with B >= 1 on {dev}, got "
                         f"{offsets.dtype} {tuple(offsets.shape)} on {offsets.device}")
    return int(offsets.shape[0]) - 1, offsets


def _maxima(loc, offsets, on_device, per_problem):
    """(max row, max column) over all of loc, and per problem the max row (per_problem; empty problems: 0)."""
    B = offsets.shape[0] - 1
    nnz = int(offsets[-1])
    if nnz == 0:
        return -1, -1, np.zeros(B, dtype=np.int64)
    starts = offsets[:-1]
    nonempty = offsets[1:] > starts
    rows = np.zeros(B, dtype=np.int64)
    if on_device:
        import torch
        mx = loc.amax(dim=0).cpu().numpy()  # (ordered behind the current stream, like every read of loc)
        if per_problem:
            counts = torch.from_numpy(np.diff(offsets)).to(loc.device)
            seg = torch.repeat_interleave(torch.arange(B, device=loc.device), counts)
            r = torch.full((B,), np.iinfo(np.int32).min, dtype=torch.int32, device=loc.device)
            r = r.scatter_reduce(0, seg, loc[:, 0], reduce="amax", include_self=True)
            rows = r.cpu().numpy().astype(np.int64)
    else:
        mx = (loc[:, 0].max(), loc[:, 1].max())  # (a column at a time: 25x faster than an axis-0 reduction of (nnz, 2))
        if per_problem:
            rows[nonempty] = np.maximum.reduceat(loc[:, 0], starts[nonempty])
    rows[~nonempty] = 0
    return int(mx[0]), int(mx[1]), rows


def _starting_prices(prices, B, cols, exact, on_device, src, need):
    """Optional float64 starting prices of shape (B, cols) (exact) or (B, P) with P >= cols, on the host or, with device
    input, on the device (src: the device input, need: what it is called in the error text).  Returns (buffer to keep
    alive, pointer, leading dimension); (None, None, 0) without prices."""
    if prices is None:
        return None, None, 0
    want = f"({B}, {cols})" if exact else f"({B}, P) with P >= {cols}"

    def bad_shape(shape):
        return shape != (B, cols) if exact else len(shape) != 2 or shape[0] != B or shape[1] < cols

    if isinstance(prices, np.ndarray):
        if prices.dtype != np.float64:
            raise ValueError(f"Buffer dtype mismatch, expected 'double' but got '{_cname(prices.dtype)}'")
        if bad_shape(tuple(prices.shape)):
            raise ValueError(f"prices must have shape {want}, got {tuple(prices.shape)}")
        if on_device:
            import torch
            p = torch.from_numpy(np.ascontiguousarray(prices)).to(src.device)
            return p, p.data_ptr(), int(prices.shape[1])
        p = np.ascontiguousarray(prices)
        return p, p.ctypes.data, int(prices.shape[1])
    if _is_device_tensor(prices):
        import torch
        if not on_device:
            raise TypeError(f"prices on the device need {need} on the device")
        if prices.dtype != torch.float64:
            raise ValueError(f"prices must be float64, got {prices.dtype}")
        if bad_shape(tuple(prices.shape)):
            raise ValueError(f"prices must have shape {want}, got {tuple(prices.shape)}")
        p = prices.contiguous()
        return p, p.data_ptr(), int(prices.shape[1])
    raise TypeError("prices must be a numpy array or a tensor on the device")


def _options(on_device, src, **fields):
    """The Options of a batch call: the device (the device input's, else the environment's), the input stream (the
    current stream of the device input's device) and `fields`.  No tuning knob applies to these paths: only the fields
    the entry point reads are set."""
    opts = _lib.Options()
    opts.struct_size = C.sizeof(_lib.Options)
    opts.device = int(os.environ.get(_ENV_DEVICE, 0))
    stream = None
    if on_device:
        import torch
        if src.device.index is not None:
            opts.device = src.device.index
        stream = torch.cuda.current_stream(src.device).cuda_stream
    for name, value in fields.items():
        setattr(opts, name, value)
    opts.input_on_device = 1 if on_device else 0
    opts.input_stream = None if stream is None else C.c_void_p(int(stream))
    return opts


def _solve_options(on_device, src, problem, eps_start, max_iter, mat_dtype=_lib.DTYPE_F64):
    # (every string other than 'min' is 'max', auction_.pyx:236)
    return _options(on_device, src, maximize=1 if problem != "min" else 0, eps_start=float(np.float32(eps_start)),
                    max_iter=int(max_iter), mat_dtype=mat_dtype)


def _new_meta(B):
    """The per-problem records and the info of a solve call, struct_size set."""
    metas = (_lib.DenseBatchMeta * B)()
    metas[0].struct_size = C.sizeof(_lib.DenseBatchMeta)
    return metas, _lib.DenseBatchInfo()


def _decode_meta(metas, info):
    """misslap_dense_batch_meta records and misslap_dense_batch_info -> the meta dict of length-B arrays."""
    raw = np.ctypeslib.as_array(metas)  # structured view, one record per problem
    obj_f32 = raw["obj_f32"].astype(np.float32)
    start_f32, final_f32 = raw["start_eps"].astype(np.float32), raw["final_eps"].astype(np.float32)
    meta = dict(
        its=raw["its"].astype(np.int64), nreductions=raw["nreductions"].astype(np.int64), eCE=raw["eCE"].astype(np.int64),
        soln_found=raw["soln_found"].astype(np.int64), n_assigned=raw["n_assigned"].astype(np.int64),
        # rounded as the reference rounds them (auction_.pyx:264, :302-303: Python's round of the float)
        obj=np.array([round(float(x), 3) for x in obj_f32]), obj_f64=raw["obj_f64"].astype(np.float64),
        start_eps=np.array([round(float(x), 3) for x in start_f32]),
        final_eps=np.array([round(float(x), 3) for x in final_f32]),
        start_eps_f32=start_f32, final_eps_f32=final_f32, n_rows=raw["n_rows"].astype(np.int64),
        n_cols=raw["n_cols"].astype(np.int64), nnz=raw["nnz"].astype(np.int64), bids_made=raw["bids_made"].astype(np.int64),
    )
    meta["timer"] = {"solve": f"{info.wall_ms:.2f}ms"}
    meta["gpu"] = dict(threads=int(info.threads), lds_bytes=int(info.lds_bytes), check_ms=float(info.check_ms),
                       matching_ms=float(info.matching_ms), kernel_ms=float(info.solve_ms), wall_ms=float(info.wall_ms))
    return meta


# the meta fields a status-mode call on the device returns as views of its record buffer
_META_VIEWS = ("its", "nreductions", "eCE", "soln_found", "n_assigned", "obj_f64", "start_eps_f32", "final_eps_f32",
               "n_rows", "n_cols", "nnz", "bids_made")


def _meta_views(rec):
    """The fields of a device buffer of misslap_dense_batch_meta records as column views, one tensor of length B each."""
    import torch
    kinds = {C.c_int32: torch.int32, C.c_int64: torch.int64, C.c_uint64: torch.int64, C.c_float: torch.float32,
             C.c_double: torch.float64}
    names = dict(start_eps_f32="start_eps", final_eps_f32="final_eps")
    fields = dict(_lib.DenseBatchMeta._fields_)
    out = {}
    for key in _META_VIEWS:
        f = names.get(key, key)
        dt = kinds[fields[f]]
        out[key] = rec.view(dt)[:, getattr(_lib.DenseBatchMeta, f).offset // C.sizeof(fields[f])]
    return out


class _StatusCall:
    """The outputs of one "verdict per problem" call and the part of its argument list every such entry point shares
    (batch_stream_call, csrc/abi_batch_stream.hpp):

        head..., *way, [dims...], [outside, outside_ld], *outs

    way = (opts, stream, workspace, workspace_bytes) and outs = (sol, prices_out, [outside_prices_out], out_on_device,
    status, matching_size, meta, info).  sol is int32 (B, sol_w), prices float64 (B, prices_w), outside_prices float64
    (B, outside_w) unless outside_w is None.  dev None is the synchronous call on host arrays: the library uploads, uses
    its own scratch and waits once, and the records are _new_meta's.  On dev the call is ordered on the current stream
    of dev: every output is a tensor allocated on that stream, the records a (B, sizeof record) uint8 tensor, and the
    workspace has the bytes lib's `sizing` function names for sizing_args."""

    def __init__(self, lib, opts, B, sol_w, prices_w, outside_w, dev, sizing, sizing_args):
        self.dev, self.info = dev, _lib.DenseBatchInfo()

        def outputs():
            self.out = dict(sol=_empty((B, sol_w), np.int32, dev), prices=_empty((B, prices_w), np.float64, dev))
            if outside_w is not None:
                self.out["outside_prices"] = _empty((B, outside_w), np.float64, dev)
            self.out.update(status=_empty(B, np.int32, dev), matching_size=_empty(B, np.int32, dev))
        if dev is None:
            outputs()
            self.rec = _new_meta(B)[0]
            way, meta = (None, None, 0), C.cast(self.rec, C.c_void_p)
        else:
            import torch
            nbytes = int(getattr(lib, sizing)(*sizing_args))
            with torch.cuda.device(dev):
                self.stream = torch.cuda.current_stream(dev)
                self.work = _empty(nbytes, np.uint8, dev)
                outputs()
                self.rec = _empty((B, C.sizeof(_lib.DenseBatchMeta)), np.uint8, dev)
            way, meta = (C.c_void_p(int(self.stream.cuda_stream)), self.work.data_ptr(), nbytes), self.rec.data_ptr()
        self.way = (C.byref(opts),) + way
        arrays = [_ptr(x) for x in self.out.values()]
        self.outs = (*arrays[:-2], 0 if dev is None else 1, *arrays[-2:], meta, C.byref(self.info))

    def result(self, keep, **own):
        """The result dict after the call: the outputs, meta and the layout's `own` keys; on a device also records, info,
        stream and keep -- the workspace and `keep` (the inputs and what was sent for them) stay referenced by the result,
        so nothing of this call is recycled before it."""
        if self.dev is None:
            return dict(self.out, meta=_decode_meta(self.rec, self.info), **own)
        return dict(self.out, meta=_meta_views(self.rec), **own, records=self.rec, info=self.info, stream=self.stream,
                    keep=(self.work, *keep))


def batch_meta_to_host(res):
    """The meta of a status-mode result as the default mode returns it: a dict of length-B numpy arrays with the
    Python-rounded obj, start_eps and final_eps.  For a device result this waits for the call's stream once."""
    if "records" not in res:
        return res["meta"]
    res["stream"].synchronize()
    raw = res["records"].cpu().numpy()
    metas = (_lib.DenseBatchMeta * raw.shape[0]).from_buffer_copy(raw.tobytes())
    return _decode_meta(metas, res["info"])


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _list_finish_launch(res, name, head, entries, src, problem, max_iter, dtype, Nmax, Mmax, d_out):
    """misslap_sparse_batch_reverse_finish / misslap_ell_batch_reverse_finish (`name`) on the device result `res` of a
    status-mode list call, on the call's stream: head is the entry point's description of the input (src: one of its
    tensors), entries what its column index holds, dtype the value type, d_out the call's outside values on the device
    or None.  res's outputs are rewritten in place; res gains `reverse` and keeps the index's workspace alive."""
    import torch
    dev, B = src.device, int(res["status"].shape[0])
    lib = _lib.load()
    opts = _solve_options(True, src, problem, 0.0, max_iter, dtype)
    nbytes = int(lib.misslap_list_batch_finish_workspace_bytes(entries))
    with torch.cuda.device(dev), torch.cuda.stream(res["stream"]):
        work, its, left = _empty(nbytes, np.uint8, dev), _empty(B, np.int64, dev), _empty(B, np.int32, dev)
    out_ld = 0
    if d_out is not None and d_out.dim() == 2:
        out_ld = int(d_out.stride(0)) if B > 1 else int(d_out.shape[1])
    _lib.check(getattr(lib, name)(
        *head, _ptr(d_out), out_ld, C.byref(opts), C.c_void_p(int(res["stream"].cuda_stream)), _ptr(work), nbytes, Nmax, Mmax,
        _ptr(res["status"]), _ptr(res["sol"]), _ptr(res["prices"]), _ptr(res.get("outside_prices")), _ptr(res["records"]),
        _ptr(its), _ptr(left)))
    res["keep"] = (*res["keep"], work)
    res["reverse"] = dict(its=its, left=left)
    return its, left


def _finished_to_host(res):
    """The device result of a finished call on uploaded numpy input as numpy arrays, meta as batch_meta_to_host gives it
    (which waits for the call's stream once)."""
    meta = batch_meta_to_host(res)
    rev = res["reverse"]
    res = {k: v for k, v in res.items() if k not in ("records", "info", "stream", "keep", "reverse")}
    res = {k: _host(v) if _is_device_tensor(v) else v for k, v in res.items()}
    res.update(meta=meta, reverse=dict(its=_host(rev["its"]), left=_host(rev["left"])))
    return res


# layout -> _status_error(res, b, code, n, m, card), the exception of problem b of a result of that layout (n, m: the
# record's n_rows and n_cols; card: its matching_size).  Each layout's module enters its own when it is imported.
_STATUS_ERRORS = {}


def raise_for_status(res):
    """Raise, for the first problem of a status-mode result whose status is not 0, the ValueError the default mode
    raises for the same batch ("problem <b>: ..."); return res when every status is 0.  For a result of
    auction_solve_sparse_batch: what its default mode raises with cardinality_check=False for that check, a
    ZeroDivisionError for `fast` with N = 0 included.  For a result of auction_solve_ell_batch: the ValueError its own
    default mode raises."""
    if "stream" in res:
        res["stream"].synchronize()
    status = _host(res["status"])
    bad = np.flatnonzero(status)
    if bad.size == 0:
        return res
    b = int(bad[0])
    raise _STATUS_ERRORS[res.get("layout", "dense")](
        res, b, int(status[b]), int(_host(res["meta"]["n_rows"])[b]), int(_host(res["meta"]["n_cols"])[b]),
        int(_host(res["matching_size"])[b]))
