// abi_points_batch.hpp -- C ABI: the batch solve from two point sets, costs |x_i - y_j|^2 formed from the coordinates and
// never stored, with a verdict per problem and in stream order (include/misslap.h):
//   misslap_solve_points_batch, misslap_points_batch_workspace_bytes
// One entry point serves the plain problem (outside == NULL) and the one with an outside option per row.  The call is
// described by one PointsCall and enqueued by points_enqueue: the check pass and the solve, whose kernels are in
// kernels_points_batch.hpp.  No guard: every pair is an edge, so the verdict knows the maximum matching.  The verdict is
// formed in the solve kernel, so nothing is read back between the launches; the two modes of a call are
// batch_stream_call's (abi_batch_stream.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, behind everything else)
#pragma once

namespace {
// The workspace of a call: the check records, the shapes the check pass sanitised and, with an outside option and
// starting prices, the staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of M + N.
inline BatchCarve points_carve(int64_t B, int64_t N, int64_t M, bool has_prices, bool has_outside) {
    return batch_carve({sizeof(PointsBatchCheck) * (size_t)B, sizeof(int) * 2 * (size_t)B,
                        has_prices && has_outside ? sizeof(double) * (size_t)B * (size_t)(M + N) : 0});
}

// B, N, M of a call: 0, or the reason they are not taken
const char *points_batch_dims(int64_t B, int64_t N, int64_t M) {
    if (B < 1 || B > 0x7fffffff) return "B must be 1 .. 2^31 - 1";
    if (N < 1 || N > kPointsBatchMaxDim || M < 1 || M > kPointsBatchMaxDim)
        return "N and M must be 1 .. MISSLAP_POINTS_BATCH_MAX_DIM";
    return nullptr;
}

// One points call.  Every pointer is a device pointer by the time the call is enqueued.
struct PointsCall {
    int64_t B, N, M, D;
    PointsView x, y;
    const int32_t *d_shapes;
    const double *d_p0, *d_outside;
    int64_t outside_ld;
    int32_t fast;
};

// Without a workspace: every input of the call that is not on the device yet (c holds the caller's pointers) into
// scratch, copied on st.  Host point sets are compact (the entry point has checked it).  shapes is then a host array
// however input_on_device is set; with a workspace it is a device array.
int points_upload(DevScratch &tmp, hipStream_t st, const misslap_options &opt, PointsCall &c) {
    const size_t ocells = c.outside_ld ? (size_t)c.B * (size_t)c.outside_ld : (size_t)c.B;
    int rc = 0;
    if (!opt.input_on_device &&
        ((rc = upload_stack(tmp, &c.x.p, c.x.p, (size_t)c.B * (size_t)c.N * (size_t)c.D, opt.mat_dtype, st)) ||
         (rc = upload_stack(tmp, &c.y.p, c.y.p, (size_t)c.B * (size_t)c.M * (size_t)c.D, opt.mat_dtype, st)) ||
         (c.d_outside && (rc = upload(tmp, &c.d_outside, c.d_outside, ocells, st))) ||
         (c.d_p0 && (rc = upload(tmp, &c.d_p0, c.d_p0, (size_t)c.B * (size_t)c.M, st)))))
        return rc;
    return c.d_shapes ? upload(tmp, &c.d_shapes, c.d_shapes, (size_t)c.B * 2, st) : rc;
}

// The two launches of a call on st: the check pass and the solve with its verdict.
template <class T, bool Out>
int points_enqueue_as(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    const BatchCarve carve = points_carve(c.B, c.N, c.M, c.d_p0 != nullptr, Out);
    PointsBatchCheck *d_chk = carve.at<PointsBatchCheck>(ws, 0);
    int *d_san = carve.at<int>(ws, 1);
    double *d_aug = Out && c.d_p0 ? carve.at<double>(ws, 2) : nullptr;

    PointsCheckArgs k{};
    k.x = c.x;
    k.y = c.y;
    k.N = c.N;
    k.M = c.M;
    k.D = (int)c.D;
    k.shapes = c.d_shapes;
    k.p0 = c.d_p0;
    k.out = d_chk;
    k.shapes_out = d_san;
    k.outside = c.d_outside;
    k.outside_ld = c.outside_ld;
    k.aug = d_aug;
    hipLaunchKernelGGL((k_points_batch_check<T, Out>), dim3((unsigned)c.B), dim3(256), 0, st, k);
    HIP_TRY(hipGetLastError());

    PointsBatchArgs a{};
    a.x = c.x;
    a.y = c.y;
    a.N = c.N;
    a.M = c.M;
    a.D = (int)c.D;
    a.shapes = d_san;
    a.chk = d_chk;
    a.fast = c.fast ? 1 : 0;
    a.status = d.status;
    a.matching_size = d.matching_size;
    a.outside = c.d_outside;
    a.outside_ld = c.outside_ld;
    if constexpr (Out) {
        a.prices = d.prices;
        a.outside_prices = d.outside_prices;
        // (the carve is N x (M + N): 155 648 B at the cap.  No prices array for batch_solve: k_points_batch_solve writes
        // the real columns itself.)
        return batch_solve_launch(k_points_batch_solve<T, true>, a, a.s, opt, c.B, c.N, c.M + c.N, d.sol, c.N, nullptr, 0,
                                  d_aug, c.M + c.N, d.meta, d.info, st);
    } else {
        return batch_solve_launch(k_points_batch_solve<T, false>, a, a.s, opt, c.B, c.N, c.M, d.sol, c.N, d.prices, c.M,
                                  c.d_p0, c.M, d.meta, d.info, st);
    }
}

int points_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    const bool f32 = opt.mat_dtype == MISSLAP_DTYPE_F32;
    if (c.d_outside) return f32 ? points_enqueue_as<float, true>(st, opt, c, ws, d) : points_enqueue_as<double, true>(st, opt, c, ws, d);
    return f32 ? points_enqueue_as<float, false>(st, opt, c, ws, d) : points_enqueue_as<double, false>(st, opt, c, ws, d);
}
}  // namespace

MISSLAP_API int64_t misslap_points_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                                         int32_t has_outside) {
    if (points_batch_dims(B, N, M)) return -1;
    return (int64_t)points_carve(B, N, M, has_prices != 0, has_outside != 0).total;
}

MISSLAP_API int misslap_solve_points_batch(int64_t B, int64_t N, int64_t M, int64_t D, const void *x, int64_t x_stride_b,
                                           int64_t x_stride_n, int64_t x_stride_d, const void *y, int64_t y_stride_b,
                                           int64_t y_stride_m, int64_t y_stride_d, const int32_t *shapes, int32_t fast,
                                           const double *prices_in, const misslap_options *opt_in, void *stream,
                                           void *workspace, int64_t workspace_bytes, const double *outside,
                                           int64_t outside_ld, int32_t *sol, double *prices_out,
                                           double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                           int32_t *matching_size, misslap_dense_batch_meta *meta,
                                           misslap_dense_batch_info *info) {
    const char *who = "misslap_solve_points_batch";
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "%s takes coordinates of MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32, got mat_dtype = %d",
                    who, (int)opt.mat_dtype);
    if (const char *why = points_batch_dims(B, N, M))
        return fail(MISSLAP_ERR_INVALID, "B, N, M = %lld, %lld, %lld: %s (%d)", (long long)B, (long long)N, (long long)M, why,
                    kPointsBatchMaxDim);
    if (D < 1 || D > kPointsBatchMaxCoords)
        return fail(MISSLAP_ERR_INVALID, "D = %lld: 1 .. MISSLAP_POINTS_BATCH_MAX_COORDS (%d) coordinates", (long long)D,
                    kPointsBatchMaxCoords);
    if (!x || !y || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null x / y / sol / status");
    if (outside && outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if ((rc = dense_strides_check(B, N, D, x_stride_b, x_stride_n, x_stride_d, who)) ||
        (rc = dense_strides_check(B, M, D, y_stride_b, y_stride_m, y_stride_d, who)))
        return rc;
    if (!opt.input_on_device && (!dense_strides_compact(N, D, x_stride_b, x_stride_n, x_stride_d) ||
                                 !dense_strides_compact(M, D, y_stride_b, y_stride_m, y_stride_d)))
        return fail(MISSLAP_ERR_INVALID, "%s: a strided point set is a device array: set input_on_device (host arrays are "
                    "compact: strides (N * D, D, 1) and (M * D, D, 1))", who);
    PointsCall c{B, N, M, D, {x, (long long)x_stride_b, (long long)x_stride_n, (long long)x_stride_d},
                 {y, (long long)y_stride_b, (long long)y_stride_m, (long long)y_stride_d}, shapes, prices_in, outside,
                 outside ? outside_ld : 0, fast};
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)N;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)B * (size_t)M;
    if (outside) {
        k.out.outside_prices = outside_prices_out;
        k.out.outside_cells = (size_t)B * (size_t)N;
    }
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = points_carve(B, N, M, prices_in != nullptr, outside != nullptr).total;
    k.sizing = "misslap_points_batch_workspace_bytes";
    return batch_stream_call(
        opt, k, [&] { return dense_batch_host_shapes(shapes, B, N, M); },
        [&](DevScratch &tmp, hipStream_t st) { return points_upload(tmp, st, opt, c); },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return points_enqueue(st, opt, c, ws, d); });
}
