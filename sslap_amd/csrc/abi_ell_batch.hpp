// abi_ell_batch.hpp -- C ABI: the batch solve from padded candidate lists, cols / vals of shape (B, N, K), with a verdict
// per problem and in stream order (misslap_solve_ell_batch, misslap_ell_batch_workspace_bytes; include/misslap.h).  The
// options, the workspace rules and the output conventions are those of misslap_solve_sparse_batch_status
// (abi_sparse_batch_status.hpp); the kernels are in kernels_ell_batch.hpp, the guard is the third source of
// k_matching_batch (kernels_matching_batch.hpp).  The verdict is formed in k_ell_batch_solve, so nothing is read back
// between the launches.
// misslap_solve_ell_batch_outside is the same call with an outside option per row (partial assignments): two launches,
// no guard, and a workspace that also stages the augmented starting prices.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_matching_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records and the guard's cardinalities, each on a 256-byte boundary.
struct EllCarve {
    size_t chk = 0, card = 0, total = 0;
    EllCarve(int64_t B, bool guard) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        card = chk + up(sizeof(EllBatchCheck) * (size_t)B);
        total = card + (guard ? up(sizeof(int) * (size_t)B) : 0);
    }
};

// B, N and K of a call: 0, or the reason they are not taken
const char *ell_batch_dims(int64_t B, int64_t N, int64_t K) {
    if (B < 1 || B > 0x7fffffff) return "B must be 1 .. 2^31 - 1";
    if (N < 1 || N > kSparseBatchMaxDim) return "N must be 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM";
    if (K < 1) return "K must be >= 1";
    if (K > kMatchBatchMaxEntries / N) return "N * K must be <= INT_MAX - 128 (the guard indexes slots with an int)";
    return nullptr;
}

// f(I{}, V{}) for the index type of cols and the value type of vals
template <class F>
auto ell_dispatch(int32_t cols_int64, int32_t mat_dtype, F &&f) {
    if (cols_int64) return mat_dtype == MISSLAP_DTYPE_F32 ? f((long long)0, float{}) : f((long long)0, double{});
    return mat_dtype == MISSLAP_DTYPE_F32 ? f(int{}, float{}) : f(int{}, double{});
}

struct EllCall {
    int64_t B, N, K, Mmax, prices_ld;
    const void *d_cols, *d_vals;
    int32_t cols_int64;
    const int32_t *d_rows;
    const double *d_p0;
    int32_t fast;
    bool guard;
};

// The three launches of a call on st: the check pass, the guard, the solve with its verdict.  Every pointer is a device
// pointer; nothing here allocates, waits or copies.
int ell_batch_enqueue(hipStream_t st, const misslap_options &opt, const EllCall &c, void *ws, int32_t *d_sol,
                      double *d_prices, int32_t *d_status, int32_t *d_msize, misslap_dense_batch_meta *d_meta,
                      misslap_dense_batch_info *info) {
    const EllCarve carve(c.B, c.guard);
    char *base = static_cast<char *>(ws);
    EllBatchCheck *d_chk = reinterpret_cast<EllBatchCheck *>(base + carve.chk);
    int *d_card = c.guard ? reinterpret_cast<int *>(base + carve.card) : nullptr;

    ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        using I = decltype(i);
        using V = decltype(v);
        hipLaunchKernelGGL((k_ell_batch_check<I, V>), dim3((unsigned)c.B), dim3(256), 0, st,
                           static_cast<const I *>(c.d_cols), static_cast<const V *>(c.d_vals), (long long)c.N,
                           (long long)c.K, c.d_rows, c.d_p0, (long long)c.prices_ld, d_chk);
    });
    HIP_TRY(hipGetLastError());
    if (c.guard) {  // every problem the check pass found clean, on the device (no row starts in the carve)
        MatchBatchArgs g{};
        g.mat = c.d_cols;
        g.N = c.N;
        g.M = c.K;
        g.echk = d_chk;
        g.Ns = (int)c.N;
        g.Ms = (int)c.Mmax;
        g.size = d_card;
        const size_t glds = matching_batch_lds_bytes(g.Ns, g.Ms, true);
        if (c.cols_int64)
            hipLaunchKernelGGL((k_matching_batch<MatchSrc::Ell, long long>), dim3((unsigned)c.B), dim3(kMatchBatchThreads),
                               glds, st, g);
        else
            hipLaunchKernelGGL((k_matching_batch<MatchSrc::Ell, int>), dim3((unsigned)c.B), dim3(kMatchBatchThreads), glds,
                               st, g);
        HIP_TRY(hipGetLastError());
    }
    EllBatchArgs a{};
    a.s.eps_b = nullptr;
    a.s.eps_opt = opt.eps_start;
    a.s.p0 = c.d_p0;
    a.s.p0_ld = c.prices_ld;
    a.s.maximize = opt.maximize ? 1 : 0;
    a.s.max_iter = opt.max_iter;
    a.s.Ns = (int)c.N;
    a.s.Ms = (int)c.Mmax;
    a.s.sol = d_sol;
    a.s.sol_ld = c.N;
    a.s.prices = d_prices;
    a.s.prices_ld = c.Mmax;
    a.s.meta = d_meta;
    a.cols = c.d_cols;
    a.vals = c.d_vals;
    a.N = c.N;
    a.K = c.K;
    a.chk = d_chk;
    a.card = d_card;
    a.fast = c.fast ? 1 : 0;
    a.status = d_status;
    a.matching_size = d_msize;
    const int threads = batch_solve_threads((int)c.N);
    const size_t lds = batch_solve_lds_bytes(c.N, c.Mmax);
    const hipError_t e = ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        auto *kernel = k_ell_batch_solve<decltype(i), decltype(v)>;
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

// The workspace of an outside call: the check records, and with starting prices the staged [p0[:m_b], zeros(n_b)] of
// every problem at a leading dimension of Mmax + N.
struct EllOutsideCarve {
    size_t chk = 0, aug = 0, total = 0;
    EllOutsideCarve(int64_t B, int64_t N, int64_t Mmax, bool has_prices) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        aug = chk + up(sizeof(EllBatchCheck) * (size_t)B);
        total = aug + (has_prices ? up(sizeof(double) * (size_t)B * (size_t)(Mmax + N)) : 0);
    }
};

struct EllOutsideCall {
    EllCall c;
    const double *d_outside;
    int64_t outside_ld;
};

// The two launches of an outside call on st: the check pass and the solve with its verdict.  Every pointer is a device
// pointer; nothing here allocates, waits or copies.
int ell_outside_enqueue(hipStream_t st, const misslap_options &opt, const EllOutsideCall &oc, void *ws, int32_t *d_sol,
                        double *d_prices, double *d_oprices, int32_t *d_status, int32_t *d_msize,
                        misslap_dense_batch_meta *d_meta, misslap_dense_batch_info *info) {
    const EllCall &c = oc.c;
    const EllOutsideCarve carve(c.B, c.N, c.Mmax, c.d_p0 != nullptr);
    char *base = static_cast<char *>(ws);
    EllBatchCheck *d_chk = reinterpret_cast<EllBatchCheck *>(base + carve.chk);
    double *d_aug = c.d_p0 ? reinterpret_cast<double *>(base + carve.aug) : nullptr;
    const long long aug_ld = (long long)(c.Mmax + c.N);

    EllOutsideCheckArgs k{};
    k.cols = c.d_cols;
    k.vals = c.d_vals;
    k.N = c.N;
    k.K = c.K;
    k.rows = c.d_rows;
    k.p0 = c.d_p0;
    k.p0_ld = c.prices_ld;
    k.out = d_chk;
    k.outside = oc.d_outside;
    k.outside_ld = oc.outside_ld;
    k.aug = d_aug;
    k.aug_ld = aug_ld;
    k.Ms = (int)c.Mmax;
    ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        hipLaunchKernelGGL((k_ell_outside_check<decltype(i), decltype(v)>), dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
    HIP_TRY(hipGetLastError());

    EllOutsideArgs a{};
    a.e.s.eps_b = nullptr;
    a.e.s.eps_opt = opt.eps_start;
    a.e.s.p0 = d_aug;
    a.e.s.p0_ld = aug_ld;
    a.e.s.maximize = opt.maximize ? 1 : 0;
    a.e.s.max_iter = opt.max_iter;
    a.e.s.Ns = (int)c.N;
    a.e.s.Ms = (int)(c.Mmax + c.N);
    a.e.s.sol = d_sol;
    a.e.s.sol_ld = c.N;
    a.e.s.prices = nullptr;  // (written by k_ell_outside_solve itself, the real columns only)
    a.e.s.prices_ld = 0;
    a.e.s.meta = d_meta;
    a.e.cols = c.d_cols;
    a.e.vals = c.d_vals;
    a.e.N = c.N;
    a.e.K = c.K;
    a.e.chk = d_chk;
    a.e.card = nullptr;
    a.e.fast = c.fast ? 1 : 0;
    a.e.status = d_status;
    a.e.matching_size = d_msize;
    a.outside = oc.d_outside;
    a.outside_ld = oc.outside_ld;
    a.prices = d_prices;
    a.outside_prices = d_oprices;
    a.Mmax = (int)c.Mmax;
    a.p0_ld = c.prices_ld;
    const int threads = batch_solve_threads((int)c.N);
    const size_t lds = batch_solve_lds_bytes(c.N, c.Mmax + c.N);
    const hipError_t e = ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        auto *kernel = k_ell_outside_solve<decltype(i), decltype(v)>;
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

MISSLAP_API int64_t misslap_ell_batch_workspace_bytes(int64_t B, int64_t N, int64_t K, int32_t has_prices,
                                                      int32_t cardinality_check) {
    (void)has_prices;
    if (ell_batch_dims(B, N, K)) return -1;
    return (int64_t)EllCarve(B, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_ell_batch(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                        const void *vals, const int32_t *rows, int32_t fast, const double *prices_in,
                                        int64_t prices_ld, int32_t cardinality_check, const misslap_options *opt_in,
                                        void *stream, void *workspace, int64_t workspace_bytes, int64_t Mmax, int32_t *sol,
                                        double *prices_out, int32_t out_on_device, int32_t *status,
                                        int32_t *matching_size, misslap_dense_batch_meta *meta,
                                        misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_ell_batch",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "misslap_solve_ell_batch takes vals of MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32, "
                    "got mat_dtype = %d", (int)opt.mat_dtype);
    if (const char *why = ell_batch_dims(B, N, K))
        return fail(MISSLAP_ERR_INVALID, "B, N, K = %lld, %lld, %lld: %s", (long long)B, (long long)N, (long long)K, why);
    if (Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Mmax = %lld: 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)", (long long)Mmax,
                    kSparseBatchMaxDim);
    if (!cols || !vals || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null cols / vals / sol / status");
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    EllCall c{};
    c.B = B;
    c.N = N;
    c.K = K;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.cols_int64 = cols_int64 ? 1 : 0;
    c.fast = fast;
    c.guard = cardinality_check != 0;
    c.d_cols = cols;
    c.d_vals = vals;
    c.d_rows = rows;
    c.d_p0 = prices_in;
    const EllCarve carve(B, c.guard);

    if (workspace) {  // ---- stream-ordered: the caller's stream, the caller's memory, no wait
        if (!opt.input_on_device || !out_on_device || !meta)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass a device meta array");
        if (workspace_bytes < (int64_t)carve.total || ((uintptr_t)workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned "
                        "(misslap_ell_batch_workspace_bytes)", (long long)workspace_bytes, workspace, (long long)carve.total);
        if ((rc = batch_set_device(opt))) return rc;
        return ell_batch_enqueue((hipStream_t)stream, opt, c, workspace, sol, prices_out, status, matching_size, meta, info);
    }

    // ---- the library's own scratch and stream, one wait at the end
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    const size_t slots = (size_t)B * (size_t)N * (size_t)K, scells = (size_t)B * (size_t)N, pcells = (size_t)B * (size_t)Mmax;
    DevScratch tmp;
    if (!opt.input_on_device) {
        const char *dc = nullptr, *dv = nullptr;
        if ((rc = upload(tmp, &dc, cols, slots * (c.cols_int64 ? 8 : 4), st)) ||
            (rc = upload(tmp, &dv, vals, slots * dense_dtype_bytes(opt.mat_dtype), st)) ||
            (rows && (rc = upload(tmp, &c.d_rows, rows, (size_t)B, st))) ||
            (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st))))
            return rc;
        c.d_cols = dc;
        c.d_vals = dv;
    }
    char *ws = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    int32_t *d_sol = sol, *d_status = status, *d_msize = matching_size;
    double *d_prices = prices_out;
    if ((rc = tmp.alloc(&ws, carve.total)) || (rc = tmp.alloc(&d_meta, (size_t)B))) return rc;
    if (!out_on_device &&
        ((rc = tmp.alloc(&d_sol, scells)) || (rc = tmp.alloc(&d_status, (size_t)B)) ||
         (matching_size && (rc = tmp.alloc(&d_msize, (size_t)B))) || (prices_out && (rc = tmp.alloc(&d_prices, pcells)))))
        return rc;
    misslap_dense_batch_info launch{};
    if ((rc = ell_batch_enqueue(st, opt, c, ws, d_sol, d_prices, d_status, d_msize, d_meta, &launch))) return rc;
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * scells, hipMemcpyDeviceToHost, st));
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

MISSLAP_API int64_t misslap_ell_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t Mmax,
                                                              int32_t has_prices) {
    if (ell_batch_dims(B, N, K) || Mmax < 1 || Mmax > kSparseBatchMaxDim) return -1;
    return (int64_t)EllOutsideCarve(B, N, Mmax, has_prices != 0).total;
}

MISSLAP_API int misslap_solve_ell_batch_outside(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                                const void *vals, const int32_t *rows, int32_t fast,
                                                const double *prices_in, int64_t prices_ld, const misslap_options *opt_in,
                                                void *stream, void *workspace, int64_t workspace_bytes, int64_t Mmax,
                                                const double *outside, int64_t outside_ld, int32_t *sol,
                                                double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_ell_batch_outside",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "misslap_solve_ell_batch_outside takes vals of MISSLAP_DTYPE_F64 or "
                    "MISSLAP_DTYPE_F32, got mat_dtype = %d", (int)opt.mat_dtype);
    if (const char *why = ell_batch_dims(B, N, K))
        return fail(MISSLAP_ERR_INVALID, "B, N, K = %lld, %lld, %lld: %s", (long long)B, (long long)N, (long long)K, why);
    if (Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Mmax = %lld: 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)", (long long)Mmax,
                    kSparseBatchMaxDim);
    if (!cols || !vals || !sol || !status || !outside)
        return fail(MISSLAP_ERR_INVALID, "null cols / vals / sol / status / outside");
    if (outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    EllOutsideCall oc{};
    EllCall &c = oc.c;
    c.B = B;
    c.N = N;
    c.K = K;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.cols_int64 = cols_int64 ? 1 : 0;
    c.fast = fast;
    c.guard = false;
    c.d_cols = cols;
    c.d_vals = vals;
    c.d_rows = rows;
    c.d_p0 = prices_in;
    oc.d_outside = outside;
    oc.outside_ld = outside_ld;
    const EllOutsideCarve carve(B, N, Mmax, prices_in != nullptr);

    if (workspace) {  // ---- stream-ordered: the caller's stream, the caller's memory, no wait
        if (!opt.input_on_device || !out_on_device || !meta)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass a device meta array");
        if (workspace_bytes < (int64_t)carve.total || ((uintptr_t)workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned "
                        "(misslap_ell_batch_outside_workspace_bytes)", (long long)workspace_bytes, workspace,
                        (long long)carve.total);
        if ((rc = batch_set_device(opt))) return rc;
        return ell_outside_enqueue((hipStream_t)stream, opt, oc, workspace, sol, prices_out, outside_prices_out, status,
                                   matching_size, meta, info);
    }

    // ---- the library's own scratch and stream, one wait at the end
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    const size_t slots = (size_t)B * (size_t)N * (size_t)K, scells = (size_t)B * (size_t)N, pcells = (size_t)B * (size_t)Mmax;
    DevScratch tmp;
    if (!opt.input_on_device) {
        const char *dc = nullptr, *dv = nullptr;
        if ((rc = upload(tmp, &dc, cols, slots * (c.cols_int64 ? 8 : 4), st)) ||
            (rc = upload(tmp, &dv, vals, slots * dense_dtype_bytes(opt.mat_dtype), st)) ||
            (rc = upload(tmp, &oc.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st)) ||
            (rows && (rc = upload(tmp, &c.d_rows, rows, (size_t)B, st))) ||
            (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st))))
            return rc;
        c.d_cols = dc;
        c.d_vals = dv;
    }
    char *ws = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    int32_t *d_sol = sol, *d_status = status, *d_msize = matching_size;
    double *d_prices = prices_out, *d_oprices = outside_prices_out;
    if ((rc = tmp.alloc(&ws, carve.total)) || (rc = tmp.alloc(&d_meta, (size_t)B))) return rc;
    if (!out_on_device &&
        ((rc = tmp.alloc(&d_sol, scells)) || (rc = tmp.alloc(&d_status, (size_t)B)) ||
         (matching_size && (rc = tmp.alloc(&d_msize, (size_t)B))) || (prices_out && (rc = tmp.alloc(&d_prices, pcells))) ||
         (outside_prices_out && (rc = tmp.alloc(&d_oprices, scells)))))
        return rc;
    misslap_dense_batch_info launch{};
    if ((rc = ell_outside_enqueue(st, opt, oc, ws, d_sol, d_prices, d_oprices, d_status, d_msize, d_meta, &launch)))
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
