// abi_dense_batch_outside.hpp -- C ABI: the dense batch with an outside option per row, for partial assignments
// (misslap_solve_dense_batch_outside, its strided form misslap_solve_dense_batch_outside_strided,
// misslap_dense_batch_outside_workspace_bytes; include/misslap.h).  The options and
// the output conventions are those of misslap_solve_dense_batch_status (abi_dense_batch_status.hpp), the two modes of the
// call are batch_stream_call's (abi_batch_stream.hpp); the kernels are the <T, true> instances of kernels_dense_batch.hpp.  Two launches, no guard; the verdict is formed in
// k_dense_outside_solve, so nothing is read back between them.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch_status.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the shapes the check pass sanitised and, with starting prices, the
// staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of M + N.
inline BatchCarve dense_outside_carve(int64_t B, int64_t N, int64_t M, bool has_prices) {
    return batch_carve({sizeof(DenseBatchCheck) * (size_t)B, sizeof(int) * 2 * (size_t)B,
                        has_prices ? sizeof(double) * (size_t)B * (size_t)(M + N) : 0});
}

struct DenseOutsideCall {
    int64_t B, N, M;
    const void *d_mat;  // elements of opt.mat_dtype
    const DenseStrides *str;  // the strides of a strided stack and its kernels, or null: the contiguous stack
    bool finite;  // MISSLAP_DENSE_ENTRIES_FINITE: the finite-mode instances of the strided family (str is not null)
    const int32_t *d_shapes;
    const double *d_p0;
    const double *d_outside;
    int64_t outside_ld;
    int32_t fast;
};

// The two launches of a call on st: the check pass and the solve with its verdict.  Every pointer is a device pointer.
int dense_outside_enqueue(hipStream_t st, const misslap_options &opt, const DenseOutsideCall &c, void *ws,
                          const BatchStreamOut &d) {
    const BatchCarve carve = dense_outside_carve(c.B, c.N, c.M, c.d_p0 != nullptr);
    DenseBatchCheck *d_chk = carve.at<DenseBatchCheck>(ws, 0);
    int *d_san = carve.at<int>(ws, 1);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 2) : nullptr;

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
        if (c.finite)
            hipLaunchKernelGGL((k_dense_finite_check<decltype(t), true>), dim3((unsigned)c.B), dim3(256), 0, st, k, *c.str);
        else if (c.str)
            hipLaunchKernelGGL((k_dense_strided_check<decltype(t), true>), dim3((unsigned)c.B), dim3(256), 0, st, k, *c.str);
        else
            hipLaunchKernelGGL(k_dense_outside_check<decltype(t)>, dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
    HIP_TRY(hipGetLastError());

    DenseFiniteOutsideArgs a{};  // (its bases are the strided and the contiguous kernels' arguments)
    a.t.d.mat = c.d_mat;
    a.t.d.N = c.N;
    a.t.d.M = c.M;
    a.t.d.shapes = d_san;
    a.t.d.chk = d_chk;
    a.t.card = nullptr;
    a.t.fast = c.fast ? 1 : 0;
    a.t.status = d.status;
    a.t.matching_size = d.matching_size;
    a.outside = c.d_outside;
    a.outside_ld = c.outside_ld;
    a.prices = d.prices;
    a.outside_prices = d.outside_prices;
    // (the carve is N x (M + N): 77 824 B at the cap, above 64 KB from 683 x 683 on.  No prices array for batch_solve:
    // k_dense_outside_solve writes the real columns itself.)
    return dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        using T = decltype(t);
        if (c.str) a.str = *c.str;
        if (c.finite)
            return batch_solve_launch(k_dense_outside_solve<T, DenseFiniteOutsideArgs>, a, a.t.d.s, opt, c.B, c.N,
                                      c.M + c.N, d.sol, c.N, nullptr, 0, d_aug, c.M + c.N, d.meta, d.info, st);
        if (c.str) {
            DenseStridedOutsideArgs &s = a;
            return batch_solve_launch(k_dense_outside_solve<T, DenseStridedOutsideArgs>, s, s.t.d.s, opt, c.B, c.N,
                                      c.M + c.N, d.sol, c.N, nullptr, 0, d_aug, c.M + c.N, d.meta, d.info, st);
        }
        DenseOutsideArgs &p = a;
        return batch_solve_launch(k_dense_outside_solve<T>, p, p.t.d.s, opt, c.B, c.N, c.M + c.N, d.sol, c.N, nullptr, 0,
                                  d_aug, c.M + c.N, d.meta, d.info, st);
    });
}
}  // namespace

MISSLAP_API int64_t misslap_dense_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices) {
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)dense_outside_carve(B, N, M, has_prices != 0).total;
}

namespace {
// misslap_solve_dense_batch_outside (strides null) and misslap_solve_dense_batch_outside_strided (`who`)
int dense_outside_call(const char *who, int64_t B, int64_t N, int64_t M, const void *mat, const int64_t *strides,
                       const int32_t *shapes, int32_t fast, const double *prices_in, const misslap_options *opt_in,
                       void *stream, void *workspace, int64_t workspace_bytes, const double *outside, int64_t outside_ld,
                       int32_t *sol, double *prices_out, double *outside_prices_out, int32_t out_on_device,
                       int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                       misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    const bool finite = dense_take_entries_finite(&opt);
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    if (!mat || !sol || !status || !outside) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status / outside");
    if (outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    DenseStrides str_arg{};
    DenseOutsideCall c{};
    if ((rc = dense_stack_layout(who, opt, B, N, M, strides, &str_arg, &c.str, finite))) return rc;
    c.finite = finite;
    c.B = B;
    c.N = N;
    c.M = M;
    c.d_mat = mat;
    c.d_shapes = shapes;
    c.d_p0 = prices_in;
    c.d_outside = outside;
    c.outside_ld = outside_ld;
    c.fast = fast;
    const size_t cells = (size_t)B * (size_t)N * (size_t)M, scells = (size_t)B * (size_t)N, pcells = (size_t)B * (size_t)M;
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = scells;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = pcells;
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = scells;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = dense_outside_carve(B, N, M, prices_in != nullptr).total;
    k.sizing = "misslap_dense_batch_outside_workspace_bytes";

    // (with a workspace shapes is a device array; without, a host array however input_on_device is set)
    return batch_stream_call(
        opt, k, [&] { return dense_batch_host_shapes(shapes, B, N, M); },
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            if (!opt.input_on_device &&
                ((rc = upload_stack(tmp, &c.d_mat, mat, cells, opt.mat_dtype, st)) ||
                 (rc = upload(tmp, &c.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st)) ||
                 (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, pcells, st)))))
                return rc;
            return shapes ? upload(tmp, &c.d_shapes, shapes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return dense_outside_enqueue(st, opt, c, ws, d); });
}
}  // namespace

MISSLAP_API int misslap_solve_dense_batch_outside(int64_t B, int64_t N, int64_t M, const void *mat, const int32_t *shapes,
                                                  int32_t fast, const double *prices_in, const misslap_options *opt_in,
                                                  void *stream, void *workspace, int64_t workspace_bytes,
                                                  const double *outside, int64_t outside_ld, int32_t *sol,
                                                  double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                  int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                  misslap_dense_batch_info *info) {
    return dense_outside_call("misslap_solve_dense_batch_outside", B, N, M, mat, nullptr, shapes, fast, prices_in, opt_in,
                              stream, workspace, workspace_bytes, outside, outside_ld, sol, prices_out, outside_prices_out,
                              out_on_device, status, matching_size, meta, info);
}

MISSLAP_API int misslap_solve_dense_batch_outside_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                                          int64_t stride_m, const void *mat, const int32_t *shapes,
                                                          int32_t fast, const double *prices_in,
                                                          const misslap_options *opt_in, void *stream, void *workspace,
                                                          int64_t workspace_bytes, const double *outside,
                                                          int64_t outside_ld, int32_t *sol, double *prices_out,
                                                          double *outside_prices_out, int32_t out_on_device,
                                                          int32_t *status, int32_t *matching_size,
                                                          misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    const int64_t strides[3] = {stride_b, stride_n, stride_m};
    return dense_outside_call("misslap_solve_dense_batch_outside_strided", B, N, M, mat, strides, shapes, fast, prices_in,
                              opt_in, stream, workspace, workspace_bytes, outside, outside_ld, sol, prices_out,
                              outside_prices_out, out_on_device, status, matching_size, meta, info);
}
