// abi_dense_batch_outside.hpp -- C ABI: the dense batch with an outside option per row, for partial assignments
// (misslap_solve_dense_batch_outside, misslap_dense_batch_outside_workspace_bytes; include/misslap.h).  The options, the
// two modes and the output conventions are those of misslap_solve_dense_batch_status (abi_dense_batch_status.hpp); the
// kernels are the <T, true> instances of kernels_dense_batch.hpp.  Two launches, no guard; the verdict is formed in
// k_dense_outside_solve, so nothing is read back between them.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch_status.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the shapes the check pass sanitised and, with starting prices, the
// staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of M + N; each on a 256-byte boundary.
struct DenseOutsideCarve {
    size_t chk = 0, shapes = 0, aug = 0, total = 0;
    DenseOutsideCarve(int64_t B, int64_t N, int64_t M, bool has_prices) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        shapes = chk + up(sizeof(DenseBatchCheck) * (size_t)B);
        aug = shapes + up(sizeof(int) * 2 * (size_t)B);
        total = aug + (has_prices ? up(sizeof(double) * (size_t)B * (size_t)(M + N)) : 0);
    }
};

struct DenseOutsideCall {
    int64_t B, N, M;
    const void *d_mat;  // elements of opt.mat_dtype
    const int32_t *d_shapes;
    const double *d_p0;
    const double *d_outside;
    int64_t outside_ld;
    int32_t fast;
};

// The two launches of a call on st: the check pass and the solve with its verdict.  Every pointer is a device pointer;
// nothing here allocates, waits or copies.
int dense_outside_enqueue(hipStream_t st, const misslap_options &opt, const DenseOutsideCall &c, void *ws, int32_t *d_sol,
                          double *d_prices, double *d_oprices, int32_t *d_status, int32_t *d_msize,
                          misslap_dense_batch_meta *d_meta, misslap_dense_batch_info *info) {
    const DenseOutsideCarve carve(c.B, c.N, c.M, c.d_p0 != nullptr);
    char *base = static_cast<char *>(ws);
    DenseBatchCheck *d_chk = reinterpret_cast<DenseBatchCheck *>(base + carve.chk);
    int *d_san = reinterpret_cast<int *>(base + carve.shapes);
    double *d_aug = c.d_p0 ? reinterpret_cast<double *>(base + carve.aug) : nullptr;

    DenseOutsideCheckArgs k{};
    k.mat = c.d_mat;
    k.N = c.N;
    k.M = c.M;
    k.shapes = c.d_shapes;
    k.p0 = c.d_p0;
    k.out = d_chk;
    k.shapes_out = d_san;
    k.outside = c.d_outside;
    k.outside_ld = c.outside_ld;
    k.aug = d_aug;
    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        hipLaunchKernelGGL(k_dense_outside_check<decltype(t)>, dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
    HIP_TRY(hipGetLastError());

    DenseOutsideArgs a{};
    BatchSolveArgs &s = a.t.d.s;
    s.eps_b = nullptr;
    s.eps_opt = opt.eps_start;
    s.p0 = d_aug;
    s.p0_ld = c.M + c.N;
    s.maximize = opt.maximize ? 1 : 0;
    s.max_iter = opt.max_iter;
    s.Ns = (int)c.N;
    s.Ms = (int)(c.M + c.N);
    s.sol = d_sol;
    s.sol_ld = c.N;
    s.prices = nullptr;  // (written by k_dense_outside_solve itself, the real columns only)
    s.prices_ld = 0;
    s.meta = d_meta;
    a.t.d.mat = c.d_mat;
    a.t.d.N = c.N;
    a.t.d.M = c.M;
    a.t.d.shapes = d_san;
    a.t.d.chk = d_chk;
    a.t.card = nullptr;
    a.t.fast = c.fast ? 1 : 0;
    a.t.status = d_status;
    a.t.matching_size = d_msize;
    a.outside = c.d_outside;
    a.outside_ld = c.outside_ld;
    a.prices = d_prices;
    a.outside_prices = d_oprices;
    const int threads = batch_solve_threads((int)c.N);
    const size_t lds = batch_solve_lds_bytes(c.N, c.M + c.N);  // (77 824 B at the cap: above 64 KB from 683 x 683 on)
    const hipError_t e = dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        auto *kernel = k_dense_outside_solve<decltype(t)>;
        // (the > 64 KB dynamic-LDS opt-in: a property of the function on the current device, set on the host without a wait)
        if (lds > 65536) {
            const hipError_t r =
                hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (r != hipSuccess) return r;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)c.B), dim3(threads), lds, st, a);
        return hipGetLastError();
    });
    HIP_TRY(e);
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->threads = threads;
        info->lds_bytes = (int32_t)lds;
    }
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int64_t misslap_dense_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices) {
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)DenseOutsideCarve(B, N, M, has_prices != 0).total;
}

MISSLAP_API int misslap_solve_dense_batch_outside(int64_t B, int64_t N, int64_t M, const void *mat, const int32_t *shapes,
                                                  int32_t fast, const double *prices_in, const misslap_options *opt_in,
                                                  void *stream, void *workspace, int64_t workspace_bytes,
                                                  const double *outside, int64_t outside_ld, int32_t *sol,
                                                  double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                  int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                  misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_dense_batch_outside",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    if (!mat || !sol || !status || !outside) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status / outside");
    if (outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    DenseOutsideCall c{};
    c.B = B;
    c.N = N;
    c.M = M;
    c.d_mat = mat;
    c.d_shapes = shapes;
    c.d_p0 = prices_in;
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    c.fast = fast;
    const DenseOutsideCarve carve(B, N, M, prices_in != nullptr);

    if (workspace) {  // ---- stream-ordered: the caller's stream, the caller's memory, no wait
        if (!opt.input_on_device || !out_on_device || !meta)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass a device meta array");
        if (workspace_bytes < (int64_t)carve.total || ((uintptr_t)workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned "
                        "(misslap_dense_batch_outside_workspace_bytes)", (long long)workspace_bytes, workspace,
                        (long long)carve.total);
        if ((rc = batch_set_device(opt))) return rc;
        return dense_outside_enqueue((hipStream_t)stream, opt, c, workspace, sol, prices_out, outside_prices_out, status,
                                     matching_size, meta, info);
    }

    // ---- the library's own scratch and stream, one wait at the end
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    if ((rc = dense_batch_host_shapes(shapes, B, N, M))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    const size_t cells = (size_t)B * (size_t)N * (size_t)M, scells = (size_t)B * (size_t)N, pcells = (size_t)B * (size_t)M;
    DevScratch tmp;
    if (!opt.input_on_device &&
        ((rc = upload_stack(tmp, &c.d_mat, mat, cells, opt.mat_dtype, st)) ||
         (rc = upload(tmp, &c.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st)) ||
         (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, pcells, st)))))
        return rc;
    char *ws = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    int32_t *d_sol = sol, *d_status = status, *d_msize = matching_size;
    double *d_prices = prices_out, *d_oprices = outside_prices_out;
    if ((shapes && (rc = upload(tmp, &c.d_shapes, shapes, (size_t)B * 2, st))) || (rc = tmp.alloc(&ws, carve.total)) ||
        (rc = tmp.alloc(&d_meta, (size_t)B)))
        return rc;
    if (!out_on_device &&
        ((rc = tmp.alloc(&d_sol, scells)) || (rc = tmp.alloc(&d_status, (size_t)B)) ||
         (matching_size && (rc = tmp.alloc(&d_msize, (size_t)B))) || (prices_out && (rc = tmp.alloc(&d_prices, pcells))) ||
         (outside_prices_out && (rc = tmp.alloc(&d_oprices, scells)))))
        return rc;
    misslap_dense_batch_info launch{};
    if ((rc = dense_outside_enqueue(st, opt, c, ws, d_sol, d_prices, d_oprices, d_status, d_msize, d_meta, &launch)))
        return rc;
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * scells, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (matching_size)
            HIP_TRY(hipMemcpyAsync(matching_size, d_msize, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (prices_out) HIP_TRY(hipMemcpyAsync(prices_out, d_prices, sizeof(double) * pcells, hipMemcpyDeviceToHost, st));
        if (outside_prices_out)
            HIP_TRY(hipMemcpyAsync(outside_prices_out, d_oprices, sizeof(double) * scells, hipMemcpyDeviceToHost, st));
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
