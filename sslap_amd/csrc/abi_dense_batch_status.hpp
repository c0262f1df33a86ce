// abi_dense_batch_status.hpp -- C ABI: the dense batch calls with a verdict per problem, in stream order
// (include/misslap.h):
//   misslap_solve_dense_batch_status, misslap_dense_batch_workspace_bytes             the contiguous stack
//   misslap_solve_dense_batch_status_strided                                          ... as a strided view
//   misslap_solve_dense_batch_outside, misslap_dense_batch_outside_workspace_bytes    with an outside option per row
//   misslap_solve_dense_batch_outside_strided                                         ... as a strided view
//   misslap_dense_batch_reverse_finish                                                one more launch behind any of them
// The options, the shape checks and the launch geometry are those of misslap_solve_dense_batch (abi_dense_batch.hpp,
// abi_batch_common.hpp), the two modes of a call are batch_stream_call's (abi_batch_stream.hpp).  Every call is
// described by one DenseCall; the sequence of launches is written once per mode (dense_batch_status_enqueue,
// dense_outside_enqueue) and reaches the kernels of kernels_dense_batch.hpp through dense_dispatch, which names the
// call's element type and layout.  The verdict is formed in the solve kernel, so nothing is read back between the
// launches.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch.hpp)
#pragma once

namespace {
// The workspace of a status call: the check records, the shapes the check pass sanitised and the guard's cardinalities.
inline BatchCarve dense_status_carve(int64_t B, bool guard) {
    return batch_carve({sizeof(DenseBatchCheck) * (size_t)B, sizeof(int) * 2 * (size_t)B, guard ? sizeof(int) * (size_t)B : 0});
}

// The workspace of an outside call: the check records, the shapes the check pass sanitised and, with starting prices,
// the staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of M + N.
inline BatchCarve dense_outside_carve(int64_t B, int64_t N, int64_t M, bool has_prices) {
    return batch_carve({sizeof(DenseBatchCheck) * (size_t)B, sizeof(int) * 2 * (size_t)B,
                        has_prices ? sizeof(double) * (size_t)B * (size_t)(M + N) : 0});
}

// One dense call.  Every pointer is a device pointer by the time the call is enqueued.
struct DenseCall {
    int64_t B, N, M;
    const void *d_mat;        // elements of opt.mat_dtype
    const DenseStrides *str;  // the layout (dense_stack_layout): null, or &str_store
    bool finite;              // ... and MISSLAP_DENSE_ENTRIES_FINITE (str is then not null)
    DenseStrides str_store;
    const int32_t *d_shapes;
    const double *d_p0, *d_outside;  // d_outside: the outside mode only
    int64_t outside_ld;
    int32_t fast;
    bool guard;  // (the outside mode: never)
};

// The check pass of a call on st (d_aug: the outside mode's staged prices, or null)
template <bool Out>
void dense_check_launch(hipStream_t st, const misslap_options &opt, const DenseCall &c, DenseBatchCheck *d_chk, int *d_san,
                        double *d_aug) {
    dense_dispatch(opt.mat_dtype, c.str, c.finite, [&](auto t, auto lay) {
        using Lay = decltype(lay);
        DenseCheckArgs<Lay> k{};
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
        k.lay = lay;
        hipLaunchKernelGGL((k_dense_batch_check<decltype(t), Lay, Out>), dim3((unsigned)c.B), dim3(256), 0, st, k);
    });
}

// what the solve kernels of both modes take of the call
DenseVerdictArgs dense_verdict_args(const DenseCall &c, const DenseBatchCheck *d_chk, const int *d_san, const int *d_card,
                                    const BatchStreamOut &d) {
    DenseVerdictArgs t{};
    t.d.mat = c.d_mat;
    t.d.N = c.N;
    t.d.M = c.M;
    t.d.shapes = d_san;
    t.d.chk = d_chk;
    t.card = d_card;
    t.fast = c.fast ? 1 : 0;
    t.status = d.status;
    t.matching_size = d.matching_size;
    return t;
}

// The three launches of a status call on st: the check pass, the guard, the solve with its verdict.
int dense_batch_status_enqueue(hipStream_t st, const misslap_options &opt, const DenseCall &c, void *ws,
                               const BatchStreamOut &d) {
    const BatchCarve carve = dense_status_carve(c.B, c.guard);
    DenseBatchCheck *d_chk = carve.at<DenseBatchCheck>(ws, 0);
    int *d_san = carve.at<int>(ws, 1);
    int *d_card = c.guard ? carve.at<int>(ws, 2) : nullptr;

    dense_check_launch<false>(st, opt, c, d_chk, d_san, nullptr);
    HIP_TRY(hipGetLastError());
    if (c.guard) {  // every problem's matching on the device: a shape the check pass zeroed is skipped (size -1)
        MatchBatchArgs g{};
        g.mat = c.d_mat;
        g.N = c.N;
        g.M = c.M;
        g.shapes = d_san;
        g.Ns = (int)c.N;
        g.Ms = (int)c.M;
        g.size = d_card;
        dense_dispatch(opt.mat_dtype, c.str, c.finite, [&](auto t, auto lay) {
            dense_guard_launch<decltype(t)>(st, c.B, g, lay, matching_batch_lds_bytes(c.N, c.M, true));
        });
        HIP_TRY(hipGetLastError());
    }
    return dense_dispatch(opt.mat_dtype, c.str, c.finite, [&](auto t, auto lay) {
        using Lay = decltype(lay);
        DenseStatusArgs<Lay> a{};
        a.t = dense_verdict_args(c, d_chk, d_san, d_card, d);
        a.lay = lay;
        return batch_solve_launch(k_dense_batch_solve_status<decltype(t), Lay>, a, a.t.d.s, opt, c.B, c.N, c.M, d.sol, c.N,
                                  d.prices, c.M, c.d_p0, c.M, d.meta, d.info, st);
    });
}

// The two launches of an outside call on st: the check pass and the solve with its verdict.  No guard.
int dense_outside_enqueue(hipStream_t st, const misslap_options &opt, const DenseCall &c, void *ws,
                          const BatchStreamOut &d) {
    const BatchCarve carve = dense_outside_carve(c.B, c.N, c.M, c.d_p0 != nullptr);
    DenseBatchCheck *d_chk = carve.at<DenseBatchCheck>(ws, 0);
    int *d_san = carve.at<int>(ws, 1);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 2) : nullptr;

    dense_check_launch<true>(st, opt, c, d_chk, d_san, d_aug);
    HIP_TRY(hipGetLastError());
    return dense_dispatch(opt.mat_dtype, c.str, c.finite, [&](auto t, auto lay) {
        using Lay = decltype(lay);
        DenseOutsideArgs<Lay> a{};
        a.t = dense_verdict_args(c, d_chk, d_san, nullptr, d);
        a.outside = c.d_outside;
        a.outside_ld = c.outside_ld;
        a.prices = d.prices;
        a.outside_prices = d.outside_prices;
        a.lay = lay;
        // (the carve is N x (M + N): 77 824 B at the cap, above 64 KB from 683 x 683 on.  No prices array for
        // batch_solve: k_dense_outside_solve writes the real columns itself.)
        return batch_solve_launch(k_dense_outside_solve<decltype(t), Lay>, a, a.t.d.s, opt, c.B, c.N, c.M + c.N, d.sol, c.N,
                                  nullptr, 0, d_aug, c.M + c.N, d.meta, d.info, st);
    });
}

// How both calls begin: the clock, the options (`who`: the entry point) and the entry rule they ask for.
int dense_call_options(const char *who, const misslap_options *opt_in, misslap_options *opt, DenseCall *c,
                       BatchStreamCall *k) {
    k->t_start = now_ms();
    if (int rc = batch_options(opt_in, opt, who,
                               "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true))
        return rc;
    c->finite = dense_take_entries_finite(opt);
    return MISSLAP_OK;
}

// ... and what follows a call's own argument checks: the layout of the stack (c.B / N / M and c.finite are set) and
// what both put into the call's description.  The outside call adds its second price array.
int dense_call_describe(const char *who, const misslap_options &opt, const int64_t *strides, DenseCall &c,
                        BatchStreamCall &k, int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
                        int32_t *matching_size, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info,
                        void *stream, void *workspace, int64_t workspace_bytes) {
    if (int rc = dense_stack_layout(who, opt, c.B, c.N, c.M, strides, &c.str_store, &c.str, c.finite)) return rc;
    k.B = c.B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)c.B * (size_t)c.N;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)c.B * (size_t)c.M;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    return MISSLAP_OK;
}

// Without a workspace: every input of the call that is not on the device yet (c holds the caller's pointers) into
// scratch, copied on st.  shapes is then a host array however input_on_device is set; with a workspace it is a
// device array.
int dense_call_upload(DevScratch &tmp, hipStream_t st, const misslap_options &opt, DenseCall &c) {
    const size_t cells = (size_t)c.B * (size_t)c.N * (size_t)c.M, pcells = (size_t)c.B * (size_t)c.M;
    const size_t ocells = c.outside_ld ? (size_t)c.B * (size_t)c.outside_ld : (size_t)c.B;
    int rc = 0;
    if (!opt.input_on_device && ((rc = upload_stack(tmp, &c.d_mat, c.d_mat, cells, opt.mat_dtype, st)) ||
                                 (c.d_outside && (rc = upload(tmp, &c.d_outside, c.d_outside, ocells, st))) ||
                                 (c.d_p0 && (rc = upload(tmp, &c.d_p0, c.d_p0, pcells, st)))))
        return rc;
    return c.d_shapes ? upload(tmp, &c.d_shapes, c.d_shapes, (size_t)c.B * 2, st) : rc;
}

// misslap_solve_dense_batch_status (strides null) and misslap_solve_dense_batch_status_strided (`who`)
int dense_batch_status_call(const char *who, int64_t B, int64_t N, int64_t M, const void *mat, const int64_t *strides,
                            const int32_t *shapes, int32_t fast, const double *prices_in, int32_t cardinality_check,
                            const misslap_options *opt_in, void *stream, void *workspace, int64_t workspace_bytes,
                            int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
                            int32_t *matching_size, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    BatchStreamCall k;
    misslap_options opt;
    DenseCall c{B, N, M, mat, nullptr, false, {}, shapes, prices_in, nullptr, 0, fast, cardinality_check != 0};
    int rc = dense_call_options(who, opt_in, &opt, &c, &k);
    if (rc) return rc;
    if (!mat || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status");
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    if ((rc = dense_call_describe(who, opt, strides, c, k, sol, prices_out, out_on_device, status, matching_size, meta, info,
                                  stream, workspace, workspace_bytes)))
        return rc;
    k.carve_total = dense_status_carve(B, c.guard).total;
    k.sizing = "misslap_dense_batch_workspace_bytes";
    return batch_stream_call(
        opt, k, [&] { return dense_batch_host_shapes(shapes, B, N, M); },
        [&](DevScratch &tmp, hipStream_t st) { return dense_call_upload(tmp, st, opt, c); },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return dense_batch_status_enqueue(st, opt, c, ws, d); });
}

// misslap_solve_dense_batch_outside (strides null) and misslap_solve_dense_batch_outside_strided (`who`)
int dense_outside_call(const char *who, int64_t B, int64_t N, int64_t M, const void *mat, const int64_t *strides,
                       const int32_t *shapes, int32_t fast, const double *prices_in, const misslap_options *opt_in,
                       void *stream, void *workspace, int64_t workspace_bytes, const double *outside, int64_t outside_ld,
                       int32_t *sol, double *prices_out, double *outside_prices_out, int32_t out_on_device,
                       int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                       misslap_dense_batch_info *info) {
    BatchStreamCall k;
    misslap_options opt;
    DenseCall c{B, N, M, mat, nullptr, false, {}, shapes, prices_in, outside, outside_ld, fast, false};
    int rc = dense_call_options(who, opt_in, &opt, &c, &k);
    if (rc) return rc;
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    if (!mat || !sol || !status || !outside) return fail(MISSLAP_ERR_INVALID, "null mat / sol / status / outside");
    if (outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if ((rc = dense_call_describe(who, opt, strides, c, k, sol, prices_out, out_on_device, status, matching_size, meta, info,
                                  stream, workspace, workspace_bytes)))
        return rc;
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)N;
    k.carve_total = dense_outside_carve(B, N, M, prices_in != nullptr).total;
    k.sizing = "misslap_dense_batch_outside_workspace_bytes";
    return batch_stream_call(
        opt, k, [&] { return dense_batch_host_shapes(shapes, B, N, M); },
        [&](DevScratch &tmp, hipStream_t st) { return dense_call_upload(tmp, st, opt, c); },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return dense_outside_enqueue(st, opt, c, ws, d); });
}

// The one launch of misslap_dense_batch_reverse_finish on st: k_dense_reverse_finish<T, DenseView<finite>, outside>.
template <class T, bool Fin>
void dense_finish_launch(hipStream_t st, int64_t B, int64_t Mo, DenseFinishArgs<DenseView<Fin>> a, bool out) {
    const size_t lds = dense_finish_lds_bytes(a.N, Mo);
    if (out)
        hipLaunchKernelGGL((k_dense_reverse_finish<T, DenseView<Fin>, true>), dim3((unsigned)B), dim3(kDenseFinishThreads),
                           lds, st, a);
    else
        hipLaunchKernelGGL((k_dense_reverse_finish<T, DenseView<Fin>, false>), dim3((unsigned)B),
                           dim3(kDenseFinishThreads), lds, st, a);
}
}  // namespace

MISSLAP_API int misslap_dense_batch_reverse_finish(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                                   int64_t stride_m, const void *mat, const int32_t *shapes,
                                                   const double *outside, int64_t outside_ld,
                                                   const misslap_options *opt_in, void *stream, const int32_t *status,
                                                   int32_t *sol, double *prices, double *outside_prices,
                                                   misslap_dense_batch_meta *meta, int64_t *reverse_its,
                                                   int32_t *reverse_left) {
    const char *who = "misslap_dense_batch_reverse_finish";
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who, "device, maximize, max_iter, mat_dtype and input_on_device", true);
    if (rc) return rc;
    const bool finite = dense_take_entries_finite(&opt);
    if (!opt.input_on_device) return fail(MISSLAP_ERR_INVALID, "%s: every array is on the device: set input_on_device", who);
    if (!mat || !status || !sol || !prices || !meta || !reverse_its || !reverse_left)
        return fail(MISSLAP_ERR_INVALID, "null mat / status / sol / prices / meta / reverse_its / reverse_left");
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    if ((outside != nullptr) != (outside_prices != nullptr))
        return fail(MISSLAP_ERR_INVALID, "%s: outside and outside_prices go together (the outputs of the outside solve)", who);
    if (outside && outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if ((rc = dense_strides_check(B, N, M, stride_b, stride_n, stride_m, who))) return rc;
    if ((rc = batch_set_device(opt))) return rc;
    const DenseStrides str{(long long)stride_b, (long long)stride_n, (long long)stride_m, 0x7fffffff};
    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        auto fill = [&](auto lay) {
            DenseFinishArgs<decltype(lay)> a{};
            a.mat = mat;
            a.N = N;
            a.M = M;
            a.shapes = shapes;
            a.outside = outside;
            a.outside_ld = outside_ld;
            a.maximize = opt.maximize ? 1 : 0;
            a.max_iter = opt.max_iter;
            a.status = status;
            a.sol = sol;
            a.prices = prices;
            a.outside_prices = outside_prices;
            a.meta = meta;
            a.its = reinterpret_cast<long long *>(reverse_its);
            a.left = reverse_left;
            a.lay = lay;
            return a;
        };
        const int64_t Mo = outside ? M + N : M;
        if (finite) dense_finish_launch<decltype(t), true>((hipStream_t)stream, B, Mo, fill(DenseView<true>{str}), outside != nullptr);
        else dense_finish_launch<decltype(t), false>((hipStream_t)stream, B, Mo, fill(DenseView<false>{str}), outside != nullptr);
    });
    HIP_TRY(hipGetLastError());
    return MISSLAP_OK;
}

MISSLAP_API int64_t misslap_dense_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                                        int32_t cardinality_check) {
    (void)has_prices;
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)dense_status_carve(B, cardinality_check != 0).total;
}

MISSLAP_API int64_t misslap_dense_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices) {
    if (dense_batch_dims(B, N, M)) return -1;
    return (int64_t)dense_outside_carve(B, N, M, has_prices != 0).total;
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
