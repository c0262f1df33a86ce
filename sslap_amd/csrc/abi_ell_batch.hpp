// abi_ell_batch.hpp -- C ABI: the batch solve from padded candidate lists, cols / vals of shape (B, N, K), with a verdict
// per problem and in stream order (include/misslap.h):
//   misslap_solve_ell_batch, misslap_ell_batch_workspace_bytes
//   misslap_solve_ell_batch_outside, misslap_ell_batch_outside_workspace_bytes    ... with an outside option per row
// Both calls are described by one EllCall, filled by ell_describe, and enqueued by ell_enqueue: the check pass, the guard
// (the plain mode only; the third source of k_matching_batch, kernels_matching_batch.hpp) and the solve, whose kernels
// are in kernels_ell_batch.hpp.  The verdict is formed in the solve kernel, so nothing is read back between the
// launches; the two modes of a call are batch_stream_call's (abi_batch_stream.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_matching_batch.hpp)
#pragma once

namespace {
// The workspace of a plain call: the check records and the guard's cardinalities.
inline BatchCarve ell_carve(int64_t B, bool guard) {
    return batch_carve({sizeof(EllBatchCheck) * (size_t)B, guard ? sizeof(int) * (size_t)B : 0});
}

// The workspace of an outside call: the check records, and with starting prices the staged [p0[:m_b], zeros(n_b)] of
// every problem at a leading dimension of Mmax + N.
inline BatchCarve ell_outside_carve(int64_t B, int64_t N, int64_t Mmax, bool has_prices) {
    return batch_carve({sizeof(EllBatchCheck) * (size_t)B, has_prices ? sizeof(double) * (size_t)B * (size_t)(Mmax + N) : 0});
}

// B, N and K of a call: 0, or the reason they are not taken
const char *ell_batch_dims(int64_t B, int64_t N, int64_t K) {
    if (B < 1 || B > 0x7fffffff) return "B must be 1 .. 2^31 - 1";
    if (N < 1 || N > kSparseBatchMaxDim) return "N must be 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM";
    if (K < 1) return "K must be >= 1";
    if (K > kMatchBatchMaxEntries / N) return "N * K must be <= INT_MAX - 128 (the guard indexes slots with an int)";
    return nullptr;
}

// the checks of mat_dtype, B, N, K and Mmax that both ELL calls make first, in this order (`who`: the call's name)
int ell_batch_shape_checks(const char *who, const misslap_options &opt, int64_t B, int64_t N, int64_t K, int64_t Mmax) {
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "%s takes vals of MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32, got mat_dtype = %d", who,
                    (int)opt.mat_dtype);
    if (const char *why = ell_batch_dims(B, N, K))
        return fail(MISSLAP_ERR_INVALID, "B, N, K = %lld, %lld, %lld: %s", (long long)B, (long long)N, (long long)K, why);
    if (Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Mmax = %lld: 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)", (long long)Mmax,
                    kSparseBatchMaxDim);
    return MISSLAP_OK;
}

// f(I{}, V{}) for the index type of cols and the value type of vals
template <class F>
auto ell_dispatch(int32_t cols_int64, int32_t mat_dtype, F &&f) {
    if (cols_int64) return mat_dtype == MISSLAP_DTYPE_F32 ? f((long long)0, float{}) : f((long long)0, double{});
    return mat_dtype == MISSLAP_DTYPE_F32 ? f(int{}, float{}) : f(int{}, double{});
}

// One ELL call.  Every pointer is a device pointer by the time the call is enqueued.
struct EllCall {
    int64_t B, N, K, Mmax, prices_ld;
    const void *d_cols, *d_vals;
    int32_t cols_int64;
    const int32_t *d_rows;
    const double *d_p0, *d_outside;  // d_outside: the outside mode only
    int64_t outside_ld;
    int32_t fast;
    bool guard;  // (the outside mode: never)
};

// What both entry points put into the call and its description once their checks have passed.  The outside call adds
// its values, its second price array and its own carve.
void ell_describe(EllCall &c, BatchStreamCall &k, int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                  const void *vals, const int32_t *rows, int32_t fast, const double *prices_in, int64_t prices_ld,
                  void *stream, void *workspace, int64_t workspace_bytes, int64_t Mmax, int32_t *sol, double *prices_out,
                  int32_t out_on_device, int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                  misslap_dense_batch_info *info) {
    c.B = B;
    c.N = N;
    c.K = K;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.cols_int64 = cols_int64 ? 1 : 0;
    c.fast = fast;
    c.d_cols = cols;
    c.d_vals = vals;
    c.d_rows = rows;
    c.d_p0 = prices_in;
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)N;
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

// Without a workspace and with host inputs: c's cols, vals, rows, starting prices and outside values, which the entry
// point set to the caller's arrays, replaced by copies on the device.
int ell_upload(DevScratch &tmp, hipStream_t st, const misslap_options &opt, EllCall &c) {
    const size_t slots = (size_t)c.B * (size_t)c.N * (size_t)c.K;
    const char *dc = nullptr, *dv = nullptr;
    int rc = 0;
    if ((rc = upload(tmp, &dc, c.d_cols, slots * (c.cols_int64 ? 8 : 4), st)) ||
        (rc = upload(tmp, &dv, c.d_vals, slots * dense_dtype_bytes(opt.mat_dtype), st)) ||
        (c.d_rows && (rc = upload(tmp, &c.d_rows, c.d_rows, (size_t)c.B, st))) ||
        (c.d_p0 && (rc = upload(tmp, &c.d_p0, c.d_p0, (size_t)c.B * (size_t)c.prices_ld, st))))
        return rc;
    c.d_cols = dc;
    c.d_vals = dv;
    if (!c.d_outside) return MISSLAP_OK;
    return upload(tmp, &c.d_outside, c.d_outside, c.outside_ld ? (size_t)c.B * (size_t)c.outside_ld : (size_t)c.B, st);
}

// The launches of a call on st: the check pass, in the plain mode the guard, the solve with its verdict.
template <bool Out>
int ell_enqueue(hipStream_t st, const misslap_options &opt, const EllCall &c, void *ws, const BatchStreamOut &d) {
    const BatchCarve carve = Out ? ell_outside_carve(c.B, c.N, c.Mmax, c.d_p0 != nullptr) : ell_carve(c.B, c.guard);
    EllBatchCheck *d_chk = carve.at<EllBatchCheck>(ws, 0);
    int *d_card = !Out && c.guard ? carve.at<int>(ws, 1) : nullptr;
    double *d_aug = Out && c.d_p0 ? carve.at<double>(ws, 1) : nullptr;
    const long long aug_ld = (long long)(c.Mmax + c.N);

    EllCheckArgs k{};
    k.cols = c.d_cols;
    k.vals = c.d_vals;
    k.N = c.N;
    k.K = c.K;
    k.rows = c.d_rows;
    k.p0 = c.d_p0;
    k.p0_ld = c.prices_ld;
    k.out = d_chk;
    k.outside = c.d_outside;
    k.outside_ld = c.outside_ld;
    k.aug = d_aug;
    k.aug_ld = aug_ld;
    k.Ms = (int)c.Mmax;
    ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        hipLaunchKernelGGL((k_ell_batch_check<decltype(i), decltype(v), Out>), dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
    HIP_TRY(hipGetLastError());
    if (d_card) {  // every problem the check pass found clean, on the device (no row starts in the carve)
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
    EllBatchArgs e{};
    e.cols = c.d_cols;
    e.vals = c.d_vals;
    e.N = c.N;
    e.K = c.K;
    e.chk = d_chk;
    e.card = d_card;
    e.fast = c.fast ? 1 : 0;
    e.status = d.status;
    e.matching_size = d.matching_size;
    return ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        if constexpr (Out) {
            EllOutsideArgs a{};
            a.e = e;
            a.outside = c.d_outside;
            a.outside_ld = c.outside_ld;
            a.prices = d.prices;
            a.outside_prices = d.outside_prices;
            a.Mmax = (int)c.Mmax;
            a.p0_ld = c.prices_ld;
            // (the carve is N x (Mmax + N).  No prices array for batch_solve: k_ell_outside_solve writes the real
            // columns itself.)
            return batch_solve_launch(k_ell_outside_solve<decltype(i), decltype(v)>, a, a.e.s, opt, c.B, c.N,
                                      c.Mmax + c.N, d.sol, c.N, nullptr, 0, d_aug, aug_ld, d.meta, d.info, st);
        } else {
            EllBatchArgs a = e;
            return batch_solve_launch(k_ell_batch_solve<decltype(i), decltype(v)>, a, a.s, opt, c.B, c.N, c.Mmax, d.sol,
                                      c.N, d.prices, c.Mmax, c.d_p0, c.prices_ld, d.meta, d.info, st);
        }
    });
}
}  // namespace

MISSLAP_API int64_t misslap_ell_batch_workspace_bytes(int64_t B, int64_t N, int64_t K, int32_t has_prices,
                                                      int32_t cardinality_check) {
    (void)has_prices;
    if (ell_batch_dims(B, N, K)) return -1;
    return (int64_t)ell_carve(B, cardinality_check != 0).total;
}

MISSLAP_API int64_t misslap_ell_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t Mmax,
                                                              int32_t has_prices) {
    if (ell_batch_dims(B, N, K) || Mmax < 1 || Mmax > kSparseBatchMaxDim) return -1;
    return (int64_t)ell_outside_carve(B, N, Mmax, has_prices != 0).total;
}

MISSLAP_API int misslap_solve_ell_batch(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                        const void *vals, const int32_t *rows, int32_t fast, const double *prices_in,
                                        int64_t prices_ld, int32_t cardinality_check, const misslap_options *opt_in,
                                        void *stream, void *workspace, int64_t workspace_bytes, int64_t Mmax, int32_t *sol,
                                        double *prices_out, int32_t out_on_device, int32_t *status,
                                        int32_t *matching_size, misslap_dense_batch_meta *meta,
                                        misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_ell_batch",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc || (rc = ell_batch_shape_checks("misslap_solve_ell_batch", opt, B, N, K, Mmax))) return rc;
    if (!cols || !vals || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null cols / vals / sol / status");
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    EllCall c{};
    ell_describe(c, k, B, N, K, cols, cols_int64, vals, rows, fast, prices_in, prices_ld, stream, workspace,
                 workspace_bytes, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info);
    c.guard = cardinality_check != 0;
    k.carve_total = ell_carve(B, c.guard).total;
    k.sizing = "misslap_ell_batch_workspace_bytes";
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) { return opt.input_on_device ? MISSLAP_OK : ell_upload(tmp, st, opt, c); },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return ell_enqueue<false>(st, opt, c, ws, d); });
}

MISSLAP_API int misslap_solve_ell_batch_outside(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                                const void *vals, const int32_t *rows, int32_t fast,
                                                const double *prices_in, int64_t prices_ld, const misslap_options *opt_in,
                                                void *stream, void *workspace, int64_t workspace_bytes, int64_t Mmax,
                                                const double *outside, int64_t outside_ld, int32_t *sol,
                                                double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_ell_batch_outside",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc || (rc = ell_batch_shape_checks("misslap_solve_ell_batch_outside", opt, B, N, K, Mmax))) return rc;
    if (!cols || !vals || !sol || !status || !outside)
        return fail(MISSLAP_ERR_INVALID, "null cols / vals / sol / status / outside");
    if (outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    EllCall c{};
    ell_describe(c, k, B, N, K, cols, cols_int64, vals, rows, fast, prices_in, prices_ld, stream, workspace,
                 workspace_bytes, Mmax, sol, prices_out, out_on_device, status, matching_size, meta, info);
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)N;
    k.carve_total = ell_outside_carve(B, N, Mmax, prices_in != nullptr).total;
    k.sizing = "misslap_ell_batch_outside_workspace_bytes";
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) { return opt.input_on_device ? MISSLAP_OK : ell_upload(tmp, st, opt, c); },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return ell_enqueue<true>(st, opt, c, ws, d); });
}
