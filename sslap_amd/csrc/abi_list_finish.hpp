// abi_list_finish.hpp -- C ABI: the reverse-auction finish behind a stream-ordered list batch solve (include/misslap.h):
//   misslap_sparse_batch_reverse_finish        behind misslap_solve_sparse_batch_status / _outside and their _view forms
//   misslap_ell_batch_reverse_finish           behind misslap_solve_ell_batch / _outside
//   misslap_list_batch_finish_workspace_bytes  the column index of either
// One launch of k_list_reverse_finish<Acc, Out> (kernels_list_finish.hpp) on the caller's stream.  Every pointer except
// opt is a device pointer; nothing is allocated, copied or waited for.  The packed arrays of a contiguous call are read
// as a view with their natural strides (2, 1), so the sparse family has the view's instances only.
// (part of the single translation unit misslap.hip; included last, after abi_sparse_batch_status.hpp)
#pragma once

namespace {
// The workspace of a finish: per entry of the call the column index's maximised value and its row.
inline BatchCarve list_finish_carve(int64_t entries) {
    return batch_carve({sizeof(double) * (size_t)entries, sizeof(int) * (size_t)entries});
}

// What both calls check of the arguments they share, before a device is touched.  who: the entry point.
int list_finish_checks(const char *who, const misslap_options &opt, int64_t entries, const void *workspace,
                       int64_t workspace_bytes, int64_t Nmax, const double *outside, int64_t outside_ld,
                       const void *status, const void *sol, const void *prices, const void *outside_prices,
                       const void *meta, const void *its, const void *left) {
    if (!opt.input_on_device) return fail(MISSLAP_ERR_INVALID, "%s: every array is on the device: set input_on_device", who);
    if (!status || !sol || !prices || !meta || !its || !left)
        return fail(MISSLAP_ERR_INVALID, "%s: null status / sol / prices / meta / reverse_its / reverse_left", who);
    if ((outside != nullptr) != (outside_prices != nullptr))
        return fail(MISSLAP_ERR_INVALID, "%s: outside and outside_prices go together (the outputs of the outside solve)", who);
    if (outside && outside_ld != 0 && outside_ld < Nmax)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= %lld", (long long)outside_ld,
                    (long long)Nmax);
    const int64_t need = (int64_t)list_finish_carve(entries).total;
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(MISSLAP_ERR_INVALID, "%s: the workspace holds %lld bytes, the call needs %lld "
                    "(misslap_list_batch_finish_workspace_bytes)", who, (long long)(workspace ? workspace_bytes : 0),
                    (long long)need);
    return MISSLAP_OK;
}

// The one launch: k_list_reverse_finish<Acc, outside> on st, with the dynamic-LDS opt-in above 64 KiB.
template <class Acc>
int list_finish_launch(hipStream_t st, int64_t B, ListFinishArgs<Acc> a, bool out) {
    const size_t lds = list_finish_lds_bytes(a.N, a.M, out, ListFinishSrc<Acc>::kRowStarts);
    auto launch = [&](auto kernel) -> int {
        if (lds > 65536)
            HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kListFinishThreads), lds, st, a);
        HIP_TRY(hipGetLastError());
        return MISSLAP_OK;
    };
    return out ? launch(k_list_reverse_finish<Acc, true>) : launch(k_list_reverse_finish<Acc, false>);
}

// what both families put into the kernel's arguments besides their source
template <class Acc>
void list_finish_fill(ListFinishArgs<Acc> &a, const misslap_options &opt, int64_t entries, void *workspace, int64_t Nmax,
                      int64_t Mmax, const double *outside, int64_t outside_ld, const int32_t *status, int32_t *sol,
                      double *prices, double *outside_prices, misslap_dense_batch_meta *meta, int64_t *its, int32_t *left) {
    const BatchCarve carve = list_finish_carve(entries);
    a.N = (int)Nmax;
    a.M = (int)Mmax;
    a.outside = outside;
    a.outside_ld = outside_ld;
    a.maximize = opt.maximize ? 1 : 0;
    a.max_iter = opt.max_iter;
    a.index_a = carve.at<double>(workspace, 0);
    a.index_row = carve.at<int>(workspace, 1);
    a.status = status;
    a.sol = sol;
    a.prices = prices;
    a.outside_prices = outside_prices;
    a.meta = meta;
    a.its = reinterpret_cast<long long *>(its);
    a.left = left;
}
}  // namespace

MISSLAP_API int64_t misslap_list_batch_finish_workspace_bytes(int64_t entries) {
    if (entries < 0 || entries > (int64_t)1 << 56) return -1;
    return (int64_t)list_finish_carve(entries).total;
}

MISSLAP_API int misslap_sparse_batch_reverse_finish(int64_t B, int64_t nnz, const void *loc, int32_t loc_int64,
                                                    int64_t stride_e, int64_t stride_c, const void *val,
                                                    const int64_t *offsets_dev, const double *outside, int64_t outside_ld,
                                                    const misslap_options *opt_in, void *stream, void *workspace,
                                                    int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                                    const int32_t *status, int32_t *sol, double *prices,
                                                    double *outside_prices, misslap_dense_batch_meta *meta,
                                                    int64_t *reverse_its, int32_t *reverse_left) {
    const char *who = "misslap_sparse_batch_reverse_finish";
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who, "device, maximize, max_iter, mat_dtype and input_on_device", true);
    if (rc || (rc = sparse_view_checks(who, opt, B, nnz, loc, stride_e, stride_c, val, offsets_dev, sol, status, Nmax,
                                       Mmax, nullptr, 0)) ||
        (rc = list_finish_checks(who, opt, nnz, workspace, workspace_bytes, Nmax, outside, outside_ld, status, sol, prices,
                                 outside_prices, meta, reverse_its, reverse_left)) ||
        (rc = batch_set_device(opt)))
        return rc;
    return ell_dispatch(loc_int64, opt.mat_dtype, [&](auto i, auto v) {
        using Src = SparseView<decltype(i), decltype(v)>;
        ListFinishArgs<SparseRuns<Src>> a{};
        a.src.w = Src{static_cast<const decltype(i) *>(loc), static_cast<const decltype(v) *>(val), (long long)stride_e,
                      (long long)stride_c};
        a.src.offsets = reinterpret_cast<const long long *>(offsets_dev);
        a.src.nnz = nnz;
        list_finish_fill(a, opt, nnz, workspace, Nmax, Mmax, outside, outside_ld, status, sol, prices, outside_prices, meta,
                         reverse_its, reverse_left);
        return list_finish_launch((hipStream_t)stream, B, a, outside != nullptr);
    });
}

MISSLAP_API int misslap_ell_batch_reverse_finish(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                                 const void *vals, const double *outside, int64_t outside_ld,
                                                 const misslap_options *opt_in, void *stream, void *workspace,
                                                 int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                                 const int32_t *status, int32_t *sol, double *prices,
                                                 double *outside_prices, misslap_dense_batch_meta *meta,
                                                 int64_t *reverse_its, int32_t *reverse_left) {
    const char *who = "misslap_ell_batch_reverse_finish";
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who, "device, maximize, max_iter, mat_dtype and input_on_device", true);
    if (rc || (rc = ell_batch_shape_checks(who, opt, B, N, K, Mmax))) return rc;
    if (Nmax != N) return fail(MISSLAP_ERR_INVALID, "%s: Nmax = %lld: the stack's N = %lld (sol and outside_prices have N columns)",
                               who, (long long)Nmax, (long long)N);
    if (!cols || !vals) return fail(MISSLAP_ERR_INVALID, "%s: null cols / vals", who);
    if ((rc = list_finish_checks(who, opt, B * N * K, workspace, workspace_bytes, N, outside, outside_ld, status, sol, prices,
                                 outside_prices, meta, reverse_its, reverse_left)) ||
        (rc = batch_set_device(opt)))
        return rc;
    return ell_dispatch(cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        ListFinishArgs<EllRuns<decltype(i), decltype(v)>> a{};
        a.src.cols = cols;
        a.src.vals = vals;
        a.src.N = N;
        a.src.K = K;
        list_finish_fill(a, opt, B * N * K, workspace, N, Mmax, outside, outside_ld, status, sol, prices, outside_prices,
                         meta, reverse_its, reverse_left);
        return list_finish_launch((hipStream_t)stream, B, a, outside != nullptr);
    });
}
