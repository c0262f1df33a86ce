// abi_sparse_batch_status.hpp -- C ABI: the four sparse batch calls with a verdict per problem, in stream order
// (include/misslap.h):
//   misslap_solve_sparse_batch_status, misslap_sparse_batch_workspace_bytes             the packed arrays
//   misslap_solve_sparse_batch_outside, misslap_sparse_batch_outside_workspace_bytes    ... with an outside option per row
//   misslap_solve_sparse_batch_status_view, misslap_sparse_batch_view_workspace_bytes   a view of them, fed from a device
//   misslap_solve_sparse_batch_outside_view                                             pipeline without a wait or a copy
// A packed call takes loc int32 [nnz][2], val float64 and host offsets, which it validates as misslap_solve_sparse_batch
// does (abi_sparse_batch.hpp, abi_batch_common.hpp).  A view call takes loc int32 or int64 with run-time strides, val
// float64 or float32, and offsets that exist on the device only: nnz is an argument, the slices are judged per problem
// in the check pass, and the guard's carve is sized from nnz.  Every call is described by one SparseCall; the sequence
// of launches is written once per mode (sparse_status_enqueue, sparse_outside_enqueue) and reaches the kernels of
// kernels_sparse_batch.hpp through sparse_dispatch, which names the call's entry source.  The verdict is formed in the
// solve kernel, so nothing is read back between the launches; the two modes of a call are batch_stream_call's
// (abi_batch_stream.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_ell_batch.hpp)
#pragma once

namespace {
// The workspace of a packed status call: the check records, the nnz + B row starts and the guard's cardinalities.
inline BatchCarve sparse_status_carve(int64_t B, int64_t nnz, bool guard) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * ((size_t)nnz + (size_t)B),
                        guard ? sizeof(int) * (size_t)B : 0});
}

// The workspace of a status call on a view: the check records, a block of Nmax + 1 row starts per problem and the
// guard's cardinalities.
inline BatchCarve sparse_view_carve(int64_t B, int64_t Nmax, bool guard) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * (size_t)B * (size_t)(Nmax + 1),
                        guard ? sizeof(int) * (size_t)B : 0});
}

// The workspace of an outside call, packed or view: the check records, a block of Nmax + 1 row starts per problem, and
// with starting prices the staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of Mmax + Nmax.
inline BatchCarve sparse_outside_carve(int64_t B, int64_t Nmax, int64_t Mmax, bool has_prices) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * (size_t)B * (size_t)(Nmax + 1),
                        has_prices ? sizeof(double) * (size_t)B * (size_t)(Mmax + Nmax) : 0});
}

// One sparse call.  Every pointer is a device pointer by the time the call is enqueued.
struct SparseCall {
    int64_t B, nnz, Nmax, Mmax, prices_ld;
    bool view;                  // false: SparsePacked and host-checked offsets; true: SparseView<I, V>, offsets unseen
    const void *d_loc, *d_val;  // packed: int32 [nnz][2] and float64 [nnz]; view: the first element of each
    int64_t zmax;               // packed: the largest problem's entries (sparse_batch_offsets)
    int32_t loc_int64;          // view: I is long long
    int64_t se, sc;             // view: the strides of loc
    const long long *d_off, *d_sizes;
    const double *d_p0, *d_outside;  // d_outside: the outside mode only
    int64_t outside_ld;
    int32_t fast;
    bool guard;  // (the outside mode: never)
};

// f(w) for the call's entry source w: SparsePacked, or SparseView<I, V> for the view's index and value type
template <class F>
auto sparse_dispatch(const SparseCall &c, const misslap_options &opt, F &&f) {
    if (!c.view) return f(SparsePacked{static_cast<const int *>(c.d_loc), static_cast<const double *>(c.d_val)});
    return ell_dispatch(c.loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        using I = decltype(i);
        using V = decltype(v);
        return f(SparseView<I, V>{static_cast<const I *>(c.d_loc), static_cast<const V *>(c.d_val), (long long)c.se,
                                  (long long)c.sc});
    });
}

int sparse_outside_ld_check(int64_t outside_ld, int64_t Nmax) {
    if (outside_ld != 0 && outside_ld < Nmax)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= Nmax = %lld",
                    (long long)outside_ld, (long long)Nmax);
    return MISSLAP_OK;
}

// The bounds of a call and its leading dimensions: Nmax and Mmax, outside_ld (null: a call without outside values, or
// one that checks it later), prices_ld.
int sparse_bound_checks(int64_t Nmax, int64_t Mmax, const int64_t *outside_ld, const double *prices_in,
                        int64_t prices_ld) {
    if (Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Nmax x Mmax = %lld x %lld: each 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)",
                    (long long)Nmax, (long long)Mmax, kSparseBatchMaxDim);
    if (outside_ld)
        if (int rc = sparse_outside_ld_check(*outside_ld, Nmax)) return rc;
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    return MISSLAP_OK;
}

// What both view entry points check before a device is touched.  who: the entry point.
int sparse_view_checks(const char *who, const misslap_options &opt, int64_t B, int64_t nnz, const void *loc,
                       int64_t se, int64_t sc, const void *val, const int64_t *offsets_dev, const void *sol,
                       const void *status, int64_t Nmax, int64_t Mmax, const double *prices_in, int64_t prices_ld) {
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 problems", (long long)B);
    if (nnz < 0 || nnz > (int64_t)1 << 56)
        return fail(MISSLAP_ERR_INVALID, "%s: nnz = %lld: 0 .. 2^56 entries", who, (long long)nnz);
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "%s: val is float64 or float32 (mat_dtype = MISSLAP_DTYPE_F64 / _F32), got %d", who,
                    (int)opt.mat_dtype);
    if (!opt.input_on_device)
        return fail(MISSLAP_ERR_INVALID, "%s: loc, val and offsets_dev are device arrays: set input_on_device", who);
    if (se < 0 || sc < 0)
        return fail(MISSLAP_ERR_INVALID, "%s: strides (%lld, %lld): a stride must be >= 0 (elements)", who, (long long)se,
                    (long long)sc);
    const unsigned __int128 extent =
        (unsigned __int128)(nnz > 0 ? nnz - 1 : 0) * (unsigned __int128)se + (unsigned __int128)sc;
    if (extent >> 62)
        return fail(MISSLAP_ERR_INVALID, "%s: strides (%lld, %lld) over %lld entries: the last element's offset does not "
                    "fit 62 bits", who, (long long)se, (long long)sc, (long long)nnz);
    if ((nnz > 0 && (!loc || !val)) || !offsets_dev || !sol || !status)
        return fail(MISSLAP_ERR_INVALID, "%s: null loc / val / offsets_dev / sol / status", who);
    return sparse_bound_checks(Nmax, Mmax, nullptr, prices_in, prices_ld);
}

// What the four entry points put into the call's description.  The outside calls add their second price array.
void sparse_describe(BatchStreamCall &k, int64_t B, int64_t Nmax, int64_t Mmax, int32_t *sol, double *prices_out,
                     int32_t out_on_device, int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                     misslap_dense_batch_info *info, void *stream, void *workspace, int64_t workspace_bytes) {
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)Nmax;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)B * (size_t)Mmax;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
}

// The check pass of a call on st (d_aug: the outside mode's staged prices, or null)
template <bool Out>
void sparse_check_launch(hipStream_t st, const misslap_options &opt, const SparseCall &c, int *d_rs,
                         SparseBatchCheck *d_chk, double *d_aug) {
    sparse_dispatch(c, opt, [&](auto w) {
        using Src = decltype(w);
        SparseCheckArgs<Src> k{};
        k.w = w;
        k.offsets = c.d_off;
        k.sizes = c.d_sizes;
        k.p0 = c.d_p0;
        k.p0_ld = c.prices_ld;
        k.row_start = d_rs;
        k.out = d_chk;
        k.outside = c.d_outside;
        k.outside_ld = c.outside_ld;
        k.aug = d_aug;
        k.aug_ld = (long long)(c.Mmax + c.Nmax);
        k.Nmax = (int)c.Nmax;
        k.Mmax = (int)c.Mmax;
        k.nnz = c.nnz;
        hipLaunchKernelGGL((k_sparse_batch_check<Src, Out>), dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
}

// what the solve kernels of both modes take of the call
template <class Src>
SparseBatchArgs<Src> sparse_solve_args(const Src &w, const SparseCall &c, const int *d_rs, const SparseBatchCheck *d_chk) {
    SparseBatchArgs<Src> d{};
    d.w = w;
    d.offsets = c.d_off;
    d.row_start = d_rs;
    d.chk = d_chk;
    return d;
}

// The three launches of a status call on st: the check pass, the guard, the solve with its verdict.
int sparse_status_enqueue(hipStream_t st, const misslap_options &opt, const SparseCall &c, void *ws,
                          const BatchStreamOut &d) {
    const BatchCarve carve = c.view ? sparse_view_carve(c.B, c.Nmax, c.guard) : sparse_status_carve(c.B, c.nnz, c.guard);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    int *d_card = c.guard ? carve.at<int>(ws, 2) : nullptr;

    sparse_check_launch<false>(st, opt, c, d_rs, d_chk, nullptr);
    HIP_TRY(hipGetLastError());
    if (c.guard) {  // every clean problem within the cap, on the device
        MatchBatchArgs g{};
        g.offsets = c.d_off;
        g.schk = d_chk;
        g.Ms = kSparseBatchMaxDim;
        g.size = d_card;
        if (!c.view) {  // the carve is that of misslap_solve_sparse_batch: the largest problem's entries
            g.loc = static_cast<const int *>(c.d_loc);
            g.Ns = (int)std::min<int64_t>(c.zmax, kSparseBatchMaxDim);
            hipLaunchKernelGGL(k_matching_batch<MatchSrc::Loc>, dim3((unsigned)c.B), dim3(kMatchBatchThreads),
                               matching_batch_lds_bytes(g.Ns, g.Ms, false), st, g);
        } else {
            // No host offsets, so no largest problem: a clean graph has at most as many rows as entries, and the call
            // has nnz of them.  Every clean problem within the cap is matched, as in the packed call.
            g.mat = c.d_loc;
            g.sN = c.se;
            g.sM = c.sc;
            g.Ns = (int)std::max<int64_t>(1, std::min<int64_t>(c.nnz, kSparseBatchMaxDim));
            const size_t glds = matching_batch_lds_bytes(g.Ns, g.Ms, false);
            if (c.loc_int64)
                hipLaunchKernelGGL((k_matching_batch<MatchSrc::LocView, long long>), dim3((unsigned)c.B),
                                   dim3(kMatchBatchThreads), glds, st, g);
            else
                hipLaunchKernelGGL((k_matching_batch<MatchSrc::LocView, int>), dim3((unsigned)c.B),
                                   dim3(kMatchBatchThreads), glds, st, g);
        }
        HIP_TRY(hipGetLastError());
    }
    return sparse_dispatch(c, opt, [&](auto w) {
        using Src = decltype(w);
        SparseStatusArgs<Src> a{};
        a.d = sparse_solve_args(w, c, d_rs, d_chk);
        a.sizes = c.d_sizes;
        a.card = d_card;
        a.fast = c.fast ? 1 : 0;
        a.status = d.status;
        a.matching_size = d.matching_size;
        return batch_solve_launch(k_sparse_batch_solve_status<Src>, a, a.d.s, opt, c.B, c.Nmax, c.Mmax, d.sol, c.Nmax,
                                  d.prices, c.Mmax, c.d_p0, c.prices_ld, d.meta, d.info, st);
    });
}

// The two launches of an outside call on st: the check pass and the solve with its verdict.  No guard.
int sparse_outside_enqueue(hipStream_t st, const misslap_options &opt, const SparseCall &c, void *ws,
                           const BatchStreamOut &d) {
    const BatchCarve carve = sparse_outside_carve(c.B, c.Nmax, c.Mmax, c.d_p0 != nullptr);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 2) : nullptr;

    sparse_check_launch<true>(st, opt, c, d_rs, d_chk, d_aug);
    HIP_TRY(hipGetLastError());
    return sparse_dispatch(c, opt, [&](auto w) {
        using Src = decltype(w);
        SparseOutsideArgs<Src> a{};
        a.d = sparse_solve_args(w, c, d_rs, d_chk);
        a.sizes = c.d_sizes;
        a.fast = c.fast ? 1 : 0;
        a.status = d.status;
        a.matching_size = d.matching_size;
        a.outside = c.d_outside;
        a.outside_ld = c.outside_ld;
        a.prices = d.prices;
        a.outside_prices = d.outside_prices;
        a.Mmax = (int)c.Mmax;
        a.p0_ld = c.prices_ld;
        // (the carve is Nmax x (Mmax + Nmax).  No prices array for batch_solve: k_sparse_outside_solve writes the real
        // columns itself.)
        return batch_solve_launch(k_sparse_outside_solve<Src>, a, a.d.s, opt, c.B, c.Nmax, c.Mmax + c.Nmax, d.sol,
                                  c.Nmax, nullptr, 0, d_aug, (long long)(c.Mmax + c.Nmax), d.meta, d.info, st);
    });
}
}  // namespace

MISSLAP_API int64_t misslap_sparse_batch_workspace_bytes(int64_t B, int64_t nnz, int32_t has_prices,
                                                         int32_t cardinality_check) {
    (void)has_prices;
    // (nnz + B row starts of 4 bytes: far below 2^63 for every B the call takes and every nnz a size_t of entries holds)
    if (B < 1 || B > 0x7fffffff || nnz < 0 || nnz > (int64_t)1 << 56) return -1;
    return (int64_t)sparse_status_carve(B, nnz, cardinality_check != 0).total;
}

MISSLAP_API int64_t misslap_sparse_batch_outside_workspace_bytes(int64_t B, int64_t Nmax, int64_t Mmax,
                                                                 int32_t has_prices) {
    if (B < 1 || B > 0x7fffffff || Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return -1;
    return (int64_t)sparse_outside_carve(B, Nmax, Mmax, has_prices != 0).total;
}

MISSLAP_API int64_t misslap_sparse_batch_view_workspace_bytes(int64_t B, int64_t nnz, int64_t Nmax, int32_t has_prices,
                                                              int32_t cardinality_check) {
    (void)has_prices;
    if (B < 1 || B > 0x7fffffff || nnz < 0 || nnz > (int64_t)1 << 56 || Nmax < 1 || Nmax > kSparseBatchMaxDim) return -1;
    return (int64_t)sparse_view_carve(B, Nmax, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_sparse_batch_status(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                                  const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                                  const double *prices_in, int64_t prices_ld, int32_t cardinality_check,
                                                  const misslap_options *opt_in, void *stream, void *workspace,
                                                  int64_t workspace_bytes, int64_t Nmax, int64_t Mmax, int32_t *sol,
                                                  double *prices_out, int32_t out_on_device, int32_t *status,
                                                  int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                  misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_sparse_batch_status",
                           "device, maximize, eps_start, max_iter, input_on_device and input_stream");
    if (rc) return rc;
    SparseCall c{};
    if (!offsets) return fail(MISSLAP_ERR_INVALID, "null offsets");
    if ((rc = sparse_batch_offsets(B, offsets, &c.zmax))) return rc;
    c.B = B;
    c.nnz = offsets[B];
    if ((c.nnz > 0 && (!loc || !val)) || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null loc / val / sol / status");
    if ((rc = sparse_bound_checks(Nmax, Mmax, nullptr, prices_in, prices_ld))) return rc;
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.fast = fast;
    c.guard = cardinality_check != 0;
    c.d_loc = loc;
    c.d_val = val;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    const size_t nnz = (size_t)c.nnz;
    sparse_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream, workspace,
                    workspace_bytes);
    k.carve_total = sparse_status_carve(B, c.nnz, c.guard).total;
    k.sizing = "misslap_sparse_batch_workspace_bytes";
    k.device_input_missing = !offsets_dev;
    k.device_input = "a device copy of offsets and ";

    // (with a workspace sizes is a device array and offsets_dev is read; without, offsets and sizes are host arrays
    // however input_on_device is set)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            const int32_t *dl = loc;
            const double *dv = val;
            if (!opt.input_on_device &&
                ((rc = upload(tmp, &dl, loc, 2 * nnz, st)) || (rc = upload(tmp, &dv, val, nnz, st)) ||
                 (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
                return rc;
            c.d_loc = dl;
            c.d_val = dv;
            c.d_sizes = nullptr;
            if ((rc = upload(tmp, &c.d_off, offsets, (size_t)B + 1, st))) return rc;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_status_enqueue(st, opt, c, ws, d); });
}

MISSLAP_API int misslap_solve_sparse_batch_outside(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                                   const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                                   const double *prices_in, int64_t prices_ld,
                                                   const misslap_options *opt_in, void *stream, void *workspace,
                                                   int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                                   const double *outside, int64_t outside_ld, int32_t *sol,
                                                   double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                   int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                   misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_sparse_batch_outside",
                           "device, maximize, eps_start, max_iter, input_on_device and input_stream");
    if (rc) return rc;
    SparseCall c{};
    if (!offsets) return fail(MISSLAP_ERR_INVALID, "null offsets");
    if ((rc = sparse_batch_offsets(B, offsets, &c.zmax))) return rc;
    c.B = B;
    c.nnz = offsets[B];
    if ((c.nnz > 0 && (!loc || !val)) || !sol || !status || !outside)
        return fail(MISSLAP_ERR_INVALID, "null loc / val / sol / status / outside");
    if ((rc = sparse_bound_checks(Nmax, Mmax, &outside_ld, prices_in, prices_ld))) return rc;
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.fast = fast;
    c.d_loc = loc;
    c.d_val = val;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    const size_t nnz = (size_t)c.nnz;
    sparse_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream, workspace,
                    workspace_bytes);
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)Nmax;
    k.carve_total = sparse_outside_carve(B, Nmax, Mmax, prices_in != nullptr).total;
    k.sizing = "misslap_sparse_batch_outside_workspace_bytes";
    k.device_input_missing = !offsets_dev;
    k.device_input = "a device copy of offsets and ";

    // (with a workspace sizes is a device array and offsets_dev is read; without, offsets and sizes are host arrays
    // however input_on_device is set, and outside lives where loc / val / prices_in live)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            const int32_t *dl = loc;
            const double *dv = val;
            if (!opt.input_on_device &&
                ((nnz && ((rc = upload(tmp, &dl, loc, 2 * nnz, st)) || (rc = upload(tmp, &dv, val, nnz, st)))) ||
                 (rc = upload(tmp, &c.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st)) ||
                 (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
                return rc;
            c.d_loc = dl;
            c.d_val = dv;
            c.d_sizes = nullptr;
            if ((rc = upload(tmp, &c.d_off, offsets, (size_t)B + 1, st))) return rc;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_outside_enqueue(st, opt, c, ws, d); });
}

// What both view entry points know of the call once sparse_view_checks has passed
SparseCall sparse_view_call(int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e, int64_t stride_c,
                            const void *val, const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                            const double *prices_in, int64_t prices_ld, int64_t Nmax, int64_t Mmax) {
    SparseCall c{};
    c.B = B;
    c.nnz = nnz;
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.view = true;
    c.d_loc = loc;
    c.d_val = val;
    c.loc_int64 = loc_int64 ? 1 : 0;
    c.se = stride_e;
    c.sc = stride_c;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    c.fast = fast;
    return c;
}

MISSLAP_API int misslap_solve_sparse_batch_status_view(
    int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e, int64_t stride_c, const void *val,
    const int64_t *offsets_dev, const int64_t *sizes, int32_t fast, const double *prices_in, int64_t prices_ld,
    int32_t cardinality_check, const misslap_options *opt_in, void *stream, void *workspace, int64_t workspace_bytes,
    int64_t Nmax, int64_t Mmax, int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
    int32_t *matching_size, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    const char *who = "misslap_solve_sparse_batch_status_view";
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc || (rc = sparse_view_checks(who, opt, B, nnz, loc, stride_e, stride_c, val, offsets_dev, sol, status, Nmax,
                                       Mmax, prices_in, prices_ld)))
        return rc;
    SparseCall c = sparse_view_call(B, nnz, loc, loc_int64, stride_e, stride_c, val, offsets_dev, sizes, fast, prices_in,
                                    prices_ld, Nmax, Mmax);
    c.guard = cardinality_check != 0;
    sparse_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream, workspace,
                    workspace_bytes);
    k.carve_total = sparse_view_carve(B, Nmax, c.guard).total;
    k.sizing = "misslap_sparse_batch_view_workspace_bytes";

    // (with a workspace sizes is a device array; without, a host array.  loc, val, offsets_dev and prices_in are device
    // arrays in both modes)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            c.d_sizes = nullptr;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : MISSLAP_OK;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_status_enqueue(st, opt, c, ws, d); });
}

MISSLAP_API int misslap_solve_sparse_batch_outside_view(
    int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e, int64_t stride_c, const void *val,
    const int64_t *offsets_dev, const int64_t *sizes, int32_t fast, const double *prices_in, int64_t prices_ld,
    const misslap_options *opt_in, void *stream, void *workspace, int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
    const double *outside, int64_t outside_ld, int32_t *sol, double *prices_out, double *outside_prices_out,
    int32_t out_on_device, int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
    misslap_dense_batch_info *info) {
    const char *who = "misslap_solve_sparse_batch_outside_view";
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc || (rc = sparse_view_checks(who, opt, B, nnz, loc, stride_e, stride_c, val, offsets_dev, sol, status, Nmax,
                                       Mmax, prices_in, prices_ld)))
        return rc;
    if (!outside) return fail(MISSLAP_ERR_INVALID, "%s: null outside", who);
    if ((rc = sparse_outside_ld_check(outside_ld, Nmax))) return rc;
    SparseCall c = sparse_view_call(B, nnz, loc, loc_int64, stride_e, stride_c, val, offsets_dev, sizes, fast, prices_in,
                                    prices_ld, Nmax, Mmax);
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    sparse_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream, workspace,
                    workspace_bytes);
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)Nmax;
    k.carve_total = sparse_outside_carve(B, Nmax, Mmax, prices_in != nullptr).total;
    k.sizing = "misslap_sparse_batch_outside_workspace_bytes";

    // (as above; outside lives where loc / val / prices_in live: on the device)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            c.d_sizes = nullptr;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : MISSLAP_OK;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_outside_enqueue(st, opt, c, ws, d); });
}
