// abi_sparse_view.hpp -- C ABI: the sparse batch on a view of the packed arrays, fed from a device pipeline without a
// wait or a copy (misslap_solve_sparse_batch_status_view, misslap_solve_sparse_batch_outside_view,
// misslap_sparse_batch_view_workspace_bytes; include/misslap.h).  loc is int32 or int64 with run-time strides, val
// float64 or float32, and the offsets exist on the device only: nnz is an argument, the slices are judged per problem in
// the check pass, and the guard's carve is sized from nnz.  The kernels are the family of kernels_sparse_view.hpp and
// k_matching_batch<MatchSrc::LocView>; the two modes are batch_stream_call's (abi_batch_stream.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_ell_batch_outside.hpp)
#pragma once

namespace {
// The workspace of a status call on a view: the check records, a block of Nmax + 1 row starts per problem and the
// guard's cardinalities.
inline BatchCarve sparse_view_carve(int64_t B, int64_t Nmax, bool guard) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * (size_t)B * (size_t)(Nmax + 1),
                        guard ? sizeof(int) * (size_t)B : 0});
}

struct SparseViewCall {
    int64_t B, nnz, Nmax, Mmax, prices_ld, se, sc;
    const void *d_loc, *d_val;
    int32_t loc_int64;
    const long long *d_off, *d_sizes;
    const double *d_p0, *d_outside;
    int64_t outside_ld;
    int32_t fast;
    bool guard;
};

// What both entry points check of the view before a device is touched.  who: the entry point.
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
    if (Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Nmax x Mmax = %lld x %lld: each 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)",
                    (long long)Nmax, (long long)Mmax, kSparseBatchMaxDim);
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    return MISSLAP_OK;
}

template <class I, class V>
SparseView<I, V> sparse_view_of(const SparseViewCall &c) {
    return SparseView<I, V>{static_cast<const I *>(c.d_loc), static_cast<const V *>(c.d_val), (long long)c.se,
                            (long long)c.sc};
}

template <class I, class V, bool Out>
void sparse_view_check_launch(hipStream_t st, const SparseViewCall &c, int *d_rs, SparseBatchCheck *d_chk, double *d_aug) {
    SparseViewCheckArgs<I, V> k{};
    k.w = sparse_view_of<I, V>(c);
    k.offsets = c.d_off;
    k.sizes = c.d_sizes;
    k.nnz = c.nnz;
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
    hipLaunchKernelGGL((k_sparse_view_check<I, V, Out>), dim3((unsigned)c.B), dim3(256), 0, st, k);
}

// The three launches of a status call on st: the check pass, the guard, the solve with its verdict.
int sparse_view_status_enqueue(hipStream_t st, const misslap_options &opt, const SparseViewCall &c, void *ws,
                               const BatchStreamOut &d) {
    const BatchCarve carve = sparse_view_carve(c.B, c.Nmax, c.guard);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    int *d_card = c.guard ? carve.at<int>(ws, 2) : nullptr;

    ell_dispatch(c.loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        sparse_view_check_launch<decltype(i), decltype(v), false>(st, c, d_rs, d_chk, nullptr);
    });
    HIP_TRY(hipGetLastError());
    if (c.guard) {
        // No host offsets, so no largest problem: a clean graph has at most as many rows as entries, and the call has
        // nnz of them.  Every clean problem within the cap is matched, as in misslap_solve_sparse_batch_status.
        MatchBatchArgs g{};
        g.mat = c.d_loc;
        g.sN = c.se;
        g.sM = c.sc;
        g.offsets = c.d_off;
        g.schk = d_chk;
        g.Ns = (int)std::max<int64_t>(1, std::min<int64_t>(c.nnz, kSparseBatchMaxDim));
        g.Ms = kSparseBatchMaxDim;
        g.size = d_card;
        const size_t glds = matching_batch_lds_bytes(g.Ns, g.Ms, false);
        if (c.loc_int64)
            hipLaunchKernelGGL((k_matching_batch<MatchSrc::LocView, long long>), dim3((unsigned)c.B),
                               dim3(kMatchBatchThreads), glds, st, g);
        else
            hipLaunchKernelGGL((k_matching_batch<MatchSrc::LocView, int>), dim3((unsigned)c.B), dim3(kMatchBatchThreads),
                               glds, st, g);
        HIP_TRY(hipGetLastError());
    }
    return ell_dispatch(c.loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        using I = decltype(i);
        using V = decltype(v);
        SparseViewStatusArgs<I, V> a{};
        a.d.w = sparse_view_of<I, V>(c);
        a.d.offsets = c.d_off;
        a.d.row_start = d_rs;
        a.d.chk = d_chk;
        a.sizes = c.d_sizes;
        a.card = d_card;
        a.fast = c.fast ? 1 : 0;
        a.status = d.status;
        a.matching_size = d.matching_size;
        return batch_solve_launch(k_sparse_view_solve_status<I, V>, a, a.d.s, opt, c.B, c.Nmax, c.Mmax, d.sol, c.Nmax,
                                  d.prices, c.Mmax, c.d_p0, c.prices_ld, d.meta, d.info, st);
    });
}

// The two launches of an outside call on st: the check pass and the solve with its verdict.
int sparse_view_outside_enqueue(hipStream_t st, const misslap_options &opt, const SparseViewCall &c, void *ws,
                                const BatchStreamOut &d) {
    const BatchCarve carve = sparse_outside_carve(c.B, c.Nmax, c.Mmax, c.d_p0 != nullptr);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 2) : nullptr;
    const long long aug_ld = (long long)(c.Mmax + c.Nmax);

    ell_dispatch(c.loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        sparse_view_check_launch<decltype(i), decltype(v), true>(st, c, d_rs, d_chk, d_aug);
    });
    HIP_TRY(hipGetLastError());
    return ell_dispatch(c.loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        using I = decltype(i);
        using V = decltype(v);
        SparseViewOutsideArgs<I, V> a{};
        a.d.w = sparse_view_of<I, V>(c);
        a.d.offsets = c.d_off;
        a.d.row_start = d_rs;
        a.d.chk = d_chk;
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
        return batch_solve_launch(k_sparse_view_outside_solve<I, V>, a, a.d.s, opt, c.B, c.Nmax, c.Mmax + c.Nmax, d.sol,
                                  c.Nmax, nullptr, 0, d_aug, aug_ld, d.meta, d.info, st);
    });
}

// What both entry points put into the call's description
void sparse_view_describe(BatchStreamCall &k, int64_t B, int64_t Nmax, int64_t Mmax, int32_t *sol, double *prices_out,
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
}  // namespace

MISSLAP_API int64_t misslap_sparse_batch_view_workspace_bytes(int64_t B, int64_t nnz, int64_t Nmax, int32_t has_prices,
                                                              int32_t cardinality_check) {
    (void)has_prices;
    if (B < 1 || B > 0x7fffffff || nnz < 0 || nnz > (int64_t)1 << 56 || Nmax < 1 || Nmax > kSparseBatchMaxDim) return -1;
    return (int64_t)sparse_view_carve(B, Nmax, cardinality_check != 0).total;
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
    SparseViewCall c{};
    c.B = B;
    c.nnz = nnz;
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.se = stride_e;
    c.sc = stride_c;
    c.d_loc = loc;
    c.d_val = val;
    c.loc_int64 = loc_int64 ? 1 : 0;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    c.fast = fast;
    c.guard = cardinality_check != 0;
    sparse_view_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream,
                         workspace, workspace_bytes);
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
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_view_status_enqueue(st, opt, c, ws, d); });
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
    if (outside_ld != 0 && outside_ld < Nmax)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= Nmax = %lld",
                    (long long)outside_ld, (long long)Nmax);
    SparseViewCall c{};
    c.B = B;
    c.nnz = nnz;
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.se = stride_e;
    c.sc = stride_c;
    c.d_loc = loc;
    c.d_val = val;
    c.loc_int64 = loc_int64 ? 1 : 0;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    c.fast = fast;
    c.guard = false;
    sparse_view_describe(k, B, Nmax, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info, stream,
                         workspace, workspace_bytes);
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
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_view_outside_enqueue(st, opt, c, ws, d); });
}
