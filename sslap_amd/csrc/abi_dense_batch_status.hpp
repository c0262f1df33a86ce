// abi_dense_batch_status.hpp -- C ABI: the dense batch with a verdict per problem, in stream order
// (misslap_solve_dense_batch_status, misslap_dense_batch_workspace_bytes; include/misslap.h).  The options, the shape
// checks and the launch geometry are those of misslap_solve_dense_batch (abi_dense_batch.hpp, abi_batch_common.hpp); the
// verdict is formed in k_dense_batch_solve_status (kernels_dense_batch.hpp), so nothing is read back between the launches.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the shapes the check pass sanitised and the guard's cardinalities, each
// on a 256-byte boundary.
struct DenseStatusCarve {
    size_t chk = 0, shapes = 0, card = 0, total = 0;
    DenseStatusCarve(int64_t B, bool guard) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        shapes = chk + up(sizeof(DenseBatchCheck) * (size_t)B);
        card = shapes + up(sizeof(int) * 2 * (size_t)B);
        total = card + (guard ? up(sizeof(int) * (size_t)B) : 0);
    }
};

// The three launches of a call on st: the check pass, the guard, the solve with its verdict.  Every pointer is a device
// pointer (d_mat: elements of opt.mat_dtype); nothing here allocates, waits or copies.
int dense_batch_status_enqueue(hipStream_t st, const misslap_options &opt, int64_t B, int64_t N, int64_t M,
                               const void *d_mat, const int32_t *d_shapes, int32_t fast, const double *d_p0, bool guard,
                               void *ws, int32_t *d_sol, double *d_prices, int32_t *d_status, int32_t *d_msize,
                               misslap_dense_batch_meta *d_meta, misslap_dense_batch_info *info) {
    const DenseStatusCarve carve(B, guard);
    char *base = static_cast<char *>(ws);
    DenseBatchCheck *d_chk = reinterpret_cast<DenseBatchCheck *>(base + carve.chk);
    int *d_san = reinterpret_cast<int *>(base + carve.shapes);
    int *d_card = guard ? reinterpret_cast<int *>(base + carve.card) : nullptr;

    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_dense_batch_check<T>, dim3((unsigned)B), dim3(256), 0, st, static_cast<const T *>(d_mat),
                           (long long)N, (long long)M, d_shapes, d_p0, d_chk, d_san);
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
        dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
            hipLaunchKernelGGL((k_matching_batch<MatchSrc::Dense, decltype(t)>), dim3((unsigned)B), dim3(kMatchBatchThreads),
                               matching_batch_lds_bytes(N, M, true), st, g);
        });
        HIP_TRY(hipGetLastError());
    }
    DenseBatchStatusArgs a{};
    a.d.s.eps_b = nullptr;
    a.d.s.eps_opt = opt.eps_start;
    a.d.s.p0 = d_p0;
    a.d.s.p0_ld = M;
    a.d.s.maximize = opt.maximize ? 1 : 0;
    a.d.s.max_iter = opt.max_iter;
    a.d.s.Ns = (int)N;
    a.d.s.Ms = (int)M;
    a.d.s.sol = d_sol;
    a.d.s.sol_ld = N;
    a.d.s.prices = d_prices;
    a.d.s.prices_ld = M;
    a.d.s.meta = d_meta;
    a.d.mat = d_mat;
    a.d.N = N;
    a.d.M = M;
    a.d.shapes = d_san;
    a.d.chk = d_chk;
    a.card = d_card;
    a.fast = fast ? 1 : 0;
    a.status = d_status;
    a.matching_size = d_msize;
    const int threads = batch_solve_threads((int)N);
    const size_t lds = batch_solve_lds_bytes(N, M);  // (at most 53 248 B at the cap: no dynamic-LDS opt-in)
    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        hipLaunchKernelGGL(k_dense_batch_solve_status<decltype(t)>, dim3((unsigned)B), dim3(threads), lds, st, a);
    });
    HIP_TRY(hipGetLastError());
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->threads = threads;
        info->lds_bytes = (int32_t)lds;
    }
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int64_t misslap_dense_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                                        int32_t cardinality_check) {
    (void)has_prices;
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)DenseStatusCarve(B, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_dense_batch_status(int64_t B, int64_t N, int64_t M, const double *mat,
                                                 const int32_t *shapes, int32_t fast, const double *prices_in,
                                                 int32_t cardinality_check, const misslap_options *opt_in, void *stream,
                                                 void *workspace, int64_t workspace_bytes, int32_t *sol,
                                                 double *prices_out, int32_t out_on_device, int32_t *status,
                                                 int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                 misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_dense_batch_status",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if (!mat || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status");
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    const bool guard = cardinality_check != 0;
    const DenseStatusCarve carve(B, guard);

    if (workspace) {  // ---- stream-ordered: the caller's stream, the caller's memory, no wait
        if (!opt.input_on_device || !out_on_device || !meta)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass a device meta array");
        if (workspace_bytes < (int64_t)carve.total || ((uintptr_t)workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned "
                        "(misslap_dense_batch_workspace_bytes)", (long long)workspace_bytes, workspace, (long long)carve.total);
        if ((rc = batch_set_device(opt))) return rc;
        return dense_batch_status_enqueue((hipStream_t)stream, opt, B, N, M, mat, shapes, fast, prices_in, guard, workspace,
                                          sol, prices_out, status, matching_size, meta, info);
    }

    // ---- the library's own scratch and stream, one wait at the end
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    if ((rc = dense_batch_host_shapes(shapes, B, N, M))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    const size_t cells = (size_t)B * (size_t)N * (size_t)M, pcells = (size_t)B * (size_t)M;
    DevScratch tmp;
    const void *d_mat = mat;
    const double *d_p0 = prices_in;
    if (!opt.input_on_device && ((rc = upload_stack(tmp, &d_mat, mat, cells, opt.mat_dtype, st)) ||
                                 (prices_in && (rc = upload(tmp, &d_p0, prices_in, pcells, st)))))
        return rc;
    const int *d_shapes = nullptr;
    char *ws = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    int32_t *d_sol = sol, *d_status = status, *d_msize = matching_size;
    double *d_prices = prices_out;
    if ((shapes && (rc = upload(tmp, &d_shapes, shapes, (size_t)B * 2, st))) || (rc = tmp.alloc(&ws, carve.total)) ||
        (rc = tmp.alloc(&d_meta, (size_t)B)))
        return rc;
    if (!out_on_device &&
        ((rc = tmp.alloc(&d_sol, (size_t)B * (size_t)N)) || (rc = tmp.alloc(&d_status, (size_t)B)) ||
         (matching_size && (rc = tmp.alloc(&d_msize, (size_t)B))) || (prices_out && (rc = tmp.alloc(&d_prices, pcells)))))
        return rc;
    misslap_dense_batch_info launch{};
    if ((rc = dense_batch_status_enqueue(st, opt, B, N, M, d_mat, d_shapes, fast, d_p0, guard, ws, d_sol, d_prices,
                                         d_status, d_msize, d_meta, &launch)))
        return rc;
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * (size_t)B * (size_t)N, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (matching_size)
            HIP_TRY(hipMemcpyAsync(matching_size, d_msize, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (prices_out) HIP_TRY(hipMemcpyAsync(prices_out, d_prices, sizeof(double) * pcells, hipMemcpyDeviceToHost, st));
    }
    if (meta) {
        const size_t w = std::min((size_t)stride, sizeof(misslap_dense_batch_meta));
        HIP_TRY(hipMemcpy2DAsync(meta, (size_t)stride, d_meta, sizeof(misslap_dense_batch_meta), w, (size_t)B,
                                 hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    tmp.drained = true;
    if (meta)  // (struct_size is an input field: the caller's value stays)
        for (int64_t b = 0; b < B; ++b)
            reinterpret_cast<misslap_dense_batch_meta *>(reinterpret_cast<char *>(meta) + (size_t)b * (size_t)stride)
                ->struct_size = stride;
    if (info) {
        *info = launch;
        info->wall_ms = now_ms() - t_start;
    }
    return MISSLAP_OK;
}
