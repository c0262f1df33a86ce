// abi_ell_batch_outside.hpp -- C ABI: the ELL batch with an outside option per row, for partial assignments
// (misslap_solve_ell_batch_outside, misslap_ell_batch_outside_workspace_bytes; include/misslap.h).  The arguments are
// those of misslap_solve_ell_batch (abi_ell_batch.hpp) plus the outside values, the two modes are batch_stream_call's
// (abi_batch_stream.hpp); the kernels are k_ell_outside_check and k_ell_outside_solve (kernels_ell_batch.hpp).  Two
// launches, no guard; the verdict is formed in k_ell_outside_solve, so nothing is read back between them.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_ell_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, and with starting prices the staged [p0[:m_b], zeros(n_b)] of every
// problem at a leading dimension of Mmax + N.
inline BatchCarve ell_outside_carve(int64_t B, int64_t N, int64_t Mmax, bool has_prices) {
    return batch_carve({sizeof(EllBatchCheck) * (size_t)B, has_prices ? sizeof(double) * (size_t)B * (size_t)(Mmax + N) : 0});
}

struct EllOutsideCall {
    EllCall c;
    const double *d_outside;
    int64_t outside_ld;
};

// The two launches of a call on st: the check pass and the solve with its verdict.  Every pointer is a device pointer.
int ell_outside_enqueue(hipStream_t st, const misslap_options &opt, const EllOutsideCall &oc, void *ws,
                        const BatchStreamOut &d) {
    const EllCall &c = oc.c;
    const BatchCarve carve = ell_outside_carve(c.B, c.N, c.Mmax, c.d_p0 != nullptr);
    EllBatchCheck *d_chk = carve.at<EllBatchCheck>(ws, 0);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 1) : nullptr;
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
    a.e.cols = c.d_cols;
    a.e.vals = c.d_vals;
    a.e.N = c.N;
    a.e.K = c.K;
    a.e.chk = d_chk;
    a.e.card = nullptr;
    a.e.fast = c.fast ? 1 : 0;
    a.e.status = d.status;
    a.e.matching_size = d.matching_size;
    a.outside = oc.d_outside;
    a.outside_ld = oc.outside_ld;
    a.prices = d.prices;
    a.outside_prices = d.outside_prices;
    a.Mmax = (int)c.Mmax;
    a.p0_ld = c.prices_ld;
    // (the carve is N x (Mmax + N).  No prices array for batch_solve: k_ell_outside_solve writes the real columns itself.)
    return ell_dispatch(c.cols_int64, opt.mat_dtype, [&](auto i, auto v) {
        return batch_solve_launch(k_ell_outside_solve<decltype(i), decltype(v)>, a, a.e.s, opt, c.B, c.N, c.Mmax + c.N,
                                  d.sol, c.N, nullptr, 0, d_aug, aug_ld, d.meta, d.info, st);
    });
}
}  // namespace

MISSLAP_API int64_t misslap_ell_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t Mmax,
                                                              int32_t has_prices) {
    if (ell_batch_dims(B, N, K) || Mmax < 1 || Mmax > kSparseBatchMaxDim) return -1;
    return (int64_t)ell_outside_carve(B, N, Mmax, has_prices != 0).total;
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
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)N;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)B * (size_t)Mmax;
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)N;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = ell_outside_carve(B, N, Mmax, prices_in != nullptr).total;
    k.sizing = "misslap_ell_batch_outside_workspace_bytes";
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            if (opt.input_on_device) return (int)MISSLAP_OK;
            const int rc = ell_upload(tmp, st, opt, c);
            return rc ? rc : upload(tmp, &oc.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st);
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return ell_outside_enqueue(st, opt, oc, ws, d); });
}
