// abi_dense_batch_status.hpp -- C ABI: the dense batch with a verdict per problem, in stream order
// (misslap_solve_dense_batch_status and its strided form misslap_solve_dense_batch_status_strided,
// misslap_dense_batch_workspace_bytes; include/misslap.h).  The options, the shape
// checks and the launch geometry are those of misslap_solve_dense_batch (abi_dense_batch.hpp, abi_batch_common.hpp), the
// two modes of the call are batch_stream_call's (abi_batch_stream.hpp); the verdict is formed in
// k_dense_batch_solve_status (kernels_dense_batch.hpp), so nothing is read back between the launches.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the shapes the check pass sanitised and the guard's cardinalities.
inline BatchCarve dense_status_carve(int64_t B, bool guard) {
    return batch_carve({sizeof(DenseBatchCheck) * (size_t)B, sizeof(int) * 2 * (size_t)B, guard ? sizeof(int) * (size_t)B : 0});
}

// The three launches of a call on st: the check pass, the guard, the solve with its verdict.  Every pointer is a device
// pointer (d_mat: elements of opt.mat_dtype).  str: the strides of a strided stack (the strided family of
// kernels_dense_batch.hpp and the matcher's strided source), or null: the contiguous stack and its kernels.
// finite (MISSLAP_DENSE_ENTRIES_FINITE; str is then never null): the finite-mode instances of that family.
int dense_batch_status_enqueue(hipStream_t st, const misslap_options &opt, int64_t B, int64_t N, int64_t M,
                               const void *d_mat, const DenseStrides *str, const int32_t *d_shapes, int32_t fast,
                               const double *d_p0, bool guard, void *ws, const BatchStreamOut &d, bool finite) {
    const BatchCarve carve = dense_status_carve(B, guard);
    DenseBatchCheck *d_chk = carve.at<DenseBatchCheck>(ws, 0);
    int *d_san = carve.at<int>(ws, 1);
    int *d_card = guard ? carve.at<int>(ws, 2) : nullptr;

    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        using T = decltype(t);
        if (str) {
            DenseOutsideCheckArgs k{};
            k.mat = d_mat;
            k.N = N;
            k.M = M;
            k.shapes = d_shapes;
            k.p0 = d_p0;
            k.out = d_chk;
            k.shapes_out = d_san;
            if (finite)
                hipLaunchKernelGGL((k_dense_finite_check<T, false>), dim3((unsigned)B), dim3(256), 0, st, k, *str);
            else
                hipLaunchKernelGGL((k_dense_strided_check<T, false>), dim3((unsigned)B), dim3(256), 0, st, k, *str);
        } else {
            hipLaunchKernelGGL(k_dense_batch_check<T>, dim3((unsigned)B), dim3(256), 0, st, static_cast<const T *>(d_mat),
                               (long long)N, (long long)M, d_shapes, d_p0, d_chk, d_san);
        }
    });
    HIP_TRY(hipGetLastError());
    if (guard) {  // every problem's matching on the device: a shape the check pass zeroed is skipped (size -1)
        MatchBatchArgs g{};
        g.mat = d_mat;
        g.N = N;
        g.M = M;
        g.shapes = d_san;
        g.Ns = (int)N;
        g.Ms = (int)M;
        g.size = d_card;
        if (str) {
            g.sB = str->sB;
            g.sN = str->sN;
            g.sM = str->sM;
        }
        dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
            const size_t lds = matching_batch_lds_bytes(N, M, true);
            if (finite)
                hipLaunchKernelGGL((k_matching_batch<MatchSrc::DenseStridedFinite, decltype(t)>), dim3((unsigned)B),
                                   dim3(kMatchBatchThreads), lds, st, g);
            else if (str)
                hipLaunchKernelGGL((k_matching_batch<MatchSrc::DenseStrided, decltype(t)>), dim3((unsigned)B),
                                   dim3(kMatchBatchThreads), lds, st, g);
            else
                hipLaunchKernelGGL((k_matching_batch<MatchSrc::Dense, decltype(t)>), dim3((unsigned)B),
                                   dim3(kMatchBatchThreads), lds, st, g);
        });
        HIP_TRY(hipGetLastError());
    }
    DenseFiniteStatusArgs a{};  // (its bases are the strided and the contiguous kernels' arguments)
    a.d.mat = d_mat;
    a.d.N = N;
    a.d.M = M;
    a.d.shapes = d_san;
    a.d.chk = d_chk;
    a.card = d_card;
    a.fast = fast ? 1 : 0;
    a.status = d.status;
    a.matching_size = d.matching_size;
    return dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        using T = decltype(t);
        if (str) a.str = *str;
        if (finite)
            return batch_solve_launch(k_dense_batch_solve_status<T, DenseFiniteStatusArgs>, a, a.d.s, opt, B, N, M, d.sol,
                                      N, d.prices, M, d_p0, M, d.meta, d.info, st);
        if (str) {
            DenseStridedStatusArgs &s = a;
            return batch_solve_launch(k_dense_batch_solve_status<T, DenseStridedStatusArgs>, s, s.d.s, opt, B, N, M, d.sol,
                                      N, d.prices, M, d_p0, M, d.meta, d.info, st);
        }
        DenseBatchStatusArgs &c = a;
        return batch_solve_launch(k_dense_batch_solve_status<T>, c, c.d.s, opt, B, N, M, d.sol, N, d.prices, M, d_p0, M,
                                  d.meta, d.info, st);
    });
}

// misslap_solve_dense_batch_status (str null) and misslap_solve_dense_batch_status_strided (`who`)
int dense_batch_status_call(const char *who, int64_t B, int64_t N, int64_t M, const void *mat, const int64_t *strides,
                            const int32_t *shapes, int32_t fast, const double *prices_in, int32_t cardinality_check,
                            const misslap_options *opt_in, void *stream, void *workspace, int64_t workspace_bytes,
                            int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
                            int32_t *matching_size, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    const bool finite = dense_take_entries_finite(&opt);
    if (!mat || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status");
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    DenseStrides str_arg{};
    const DenseStrides *str = nullptr;
    if ((rc = dense_stack_layout(who, opt, B, N, M, strides, &str_arg, &str, finite))) return rc;
    const bool guard = cardinality_check != 0;
    const size_t cells = (size_t)B * (size_t)N * (size_t)M, pcells = (size_t)B * (size_t)M;
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)N;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = pcells;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = dense_status_carve(B, guard).total;
    k.sizing = "misslap_dense_batch_workspace_bytes";

    // (with a workspace shapes is a device array; without, a host array however input_on_device is set)
    const void *d_mat = mat;
    const double *d_p0 = prices_in;
    const int32_t *d_shapes = shapes;
    return batch_stream_call(
        opt, k, [&] { return dense_batch_host_shapes(shapes, B, N, M); },
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            if (!opt.input_on_device && ((rc = upload_stack(tmp, &d_mat, mat, cells, opt.mat_dtype, st)) ||
                                         (prices_in && (rc = upload(tmp, &d_p0, prices_in, pcells, st)))))
                return rc;
            return shapes ? upload(tmp, &d_shapes, shapes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) {
            return dense_batch_status_enqueue(st, opt, B, N, M, d_mat, str, d_shapes, fast, d_p0, guard, ws, d, finite);
        });
}
}  // namespace

MISSLAP_API int64_t misslap_dense_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                                        int32_t cardinality_check) {
    (void)has_prices;
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)dense_status_carve(B, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_dense_batch_status(int64_t B, int64_t N, int64_t M, const double *mat,
                                                 const int32_t *shapes, int32_t fast, const double *prices_in,
                                                 int32_t cardinality_check, const misslap_options *opt_in, void *stream,
                                                 void *workspace, int64_t workspace_bytes, int32_t *sol,
                                                 double *prices_out, int32_t out_on_device, int32_t *status,
                                                 int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                 misslap_dense_batch_info *info) {
    return dense_batch_status_call("misslap_solve_dense_batch_status", B, N, M, mat, nullptr, shapes, fast, prices_in,
                                   cardinality_check, opt_in, stream, workspace, workspace_bytes, sol, prices_out,
                                   out_on_device, status, matching_size, meta, info);
}

MISSLAP_API int misslap_solve_dense_batch_status_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                                         int64_t stride_m, const void *mat, const int32_t *shapes,
                                                         int32_t fast, const double *prices_in,
                                                         int32_t cardinality_check, const misslap_options *opt_in,
                                                         void *stream, void *workspace, int64_t workspace_bytes,
                                                         int32_t *sol, double *prices_out, int32_t out_on_device,
                                                         int32_t *status, int32_t *matching_size,
                                                         misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    const int64_t strides[3] = {stride_b, stride_n, stride_m};
    return dense_batch_status_call("misslap_solve_dense_batch_status_strided", B, N, M, mat, strides, shapes, fast,
                                   prices_in, cardinality_check, opt_in, stream, workspace, workspace_bytes, sol,
                                   prices_out, out_on_device, status, matching_size, meta, info);
}
