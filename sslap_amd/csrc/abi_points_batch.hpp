// abi_points_batch.hpp -- C ABI: the batch solve from two point sets, costs |x_i - y_j|^2 formed from the coordinates and
// never stored, with a verdict per problem and in stream order (include/misslap.h):
//   misslap_solve_points_batch, misslap_solve_points_batch_whitened, misslap_points_batch_workspace_bytes
// (and, through points_batch_call, misslap_solve_boxes_batch of abi_boxes_batch.hpp: a box set is a point set of D = 4)
// One entry point serves the plain problem (outside == NULL) and the one with an outside option per row; the whitened
// entry point is the same call with a lower-triangular matrix per row, costs |W_i (x_i - y_j)|^2.  The call is
// described by one PointsCall and enqueued by points_enqueue: the check pass and the solve, whose kernels are in
// kernels_points_batch.hpp and, with a matrix, kernels_points_whiten.hpp (enqueued by abi_points_whiten.hpp).  No guard: every pair is an edge, so the verdict knows the maximum matching.  The verdict is
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
    WhitenView w;  // p null: the plain call
    int32_t boxes;  // 0, or MISSLAP_BOXES_METRIC_*: x and y are box sets (D = 4) and the cost is that metric's
};

// Without a workspace: every input of the call that is not on the device yet (c holds the caller's pointers) into
// scratch, copied on st.  Host point sets and matrices are compact (the entry point has checked it).  shapes is then a host array
// however input_on_device is set; with a workspace it is a device array.
int points_upload(DevScratch &tmp, hipStream_t st, const misslap_options &opt, PointsCall &c) {
    const size_t ocells = c.outside_ld ? (size_t)c.B * (size_t)c.outside_ld : (size_t)c.B;
    int rc = 0;
    if (!opt.input_on_device &&
        ((rc = upload_stack(tmp, &c.x.p, c.x.p, (size_t)c.B * (size_t)c.N * (size_t)c.D, opt.mat_dtype, st)) ||
         (rc = upload_stack(tmp, &c.y.p, c.y.p, (size_t)c.B * (size_t)c.M * (size_t)c.D, opt.mat_dtype, st)) ||
         (c.w.p && (rc = upload_stack(tmp, &c.w.p, c.w.p, (size_t)c.B * (size_t)c.N * (size_t)(c.D * c.D), opt.mat_dtype, st))) ||
         (c.d_outside && (rc = upload(tmp, &c.d_outside, c.d_outside, ocells, st))) ||
         (c.d_p0 && (rc = upload(tmp, &c.d_p0, c.d_p0, (size_t)c.B * (size_t)c.M, st)))))
        return rc;
    return c.d_shapes ? upload(tmp, &c.d_shapes, c.d_shapes, (size_t)c.B * 2, st) : rc;
}

// The two kernels of a call: the plain pair takes its argument struct as it is, the whitened pair the struct and the
// matrices (the specialisation for Wh = 1 is in abi_points_whiten.hpp, next to its kernels; Wh = 2 and 3 are the box
// metrics of abi_boxes_batch.hpp, which take the plain structs).
template <class T, bool Out, int Wh>
struct PointsKernels {
    static PointsCheckArgs check_args(const PointsCheckArgs &k, const WhitenView &) { return k; }
    static PointsBatchArgs solve_args(const WhitenView &) { return PointsBatchArgs{}; }
    static PointsBatchArgs &inner(PointsBatchArgs &a) { return a; }
    static constexpr auto check = k_points_batch_check<T, Out>;
    static constexpr auto solve = k_points_batch_solve<T, Out>;
};

// The two launches of a call on st: the check pass and the solve with its verdict.
template <class T, bool Out, int Wh>
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
    using Kernels = PointsKernels<T, Out, Wh>;
    hipLaunchKernelGGL(Kernels::check, dim3((unsigned)c.B), dim3(256), 0, st, Kernels::check_args(k, c.w));
    HIP_TRY(hipGetLastError());

    auto args = Kernels::solve_args(c.w);
    PointsBatchArgs &a = Kernels::inner(args);
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
        return batch_solve_launch(Kernels::solve, args, a.s, opt, c.B, c.N, c.M + c.N, d.sol, c.N, nullptr, 0, d_aug,
                                  c.M + c.N, d.meta, d.info, st);
    } else {
        return batch_solve_launch(Kernels::solve, args, a.s, opt, c.B, c.N, c.M, d.sol, c.N, d.prices, c.M, c.d_p0, c.M,
                                  d.meta, d.info, st);
    }
}

template <int Wh>
int points_enqueue_wh(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    const bool f32 = opt.mat_dtype == MISSLAP_DTYPE_F32;
    if (c.d_outside)
        return f32 ? points_enqueue_as<float, true, Wh>(st, opt, c, ws, d) : points_enqueue_as<double, true, Wh>(st, opt, c, ws, d);
    return f32 ? points_enqueue_as<float, false, Wh>(st, opt, c, ws, d) : points_enqueue_as<double, false, Wh>(st, opt, c, ws, d);
}
// (abi_points_whiten.hpp: points_enqueue_wh<1>, behind the whitened kernels; abi_boxes_batch.hpp: <2> and <3>, behind
// the box kernels)
int points_whiten_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d);
int boxes_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d);
int points_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    if (c.boxes) return boxes_enqueue(st, opt, c, ws, d);
    return c.w.p ? points_whiten_enqueue(st, opt, c, ws, d) : points_enqueue_wh<0>(st, opt, c, ws, d);
}

// The matrices of a whitened call (`who`): D within the whitened cap, w not null, element strides >= 0 whose extent
// fits 62 bits, and a host array compact.  Made before any device is touched.
int points_whiten_check(const char *who, int64_t B, int64_t N, int64_t D, const void *w, int64_t sB, int64_t sN, int64_t sK,
                        int64_t sL, bool on_device) {
    if (!w) return fail(MISSLAP_ERR_INVALID, "%s: null w (the call without a matrix is the plain entry point)", who);
    if (D < 1 || D > MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS)
        return fail(MISSLAP_ERR_INVALID, "D = %lld: 1 .. MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS (%d) coordinates with a "
                    "whitening matrix", (long long)D, MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS);
    if (sB < 0 || sN < 0 || sK < 0 || sL < 0)
        return fail(MISSLAP_ERR_INVALID, "%s: w strides (%lld, %lld, %lld, %lld): a stride must be >= 0 (elements)", who,
                    (long long)sB, (long long)sN, (long long)sK, (long long)sL);
    const unsigned __int128 extent = (unsigned __int128)(B - 1) * (unsigned __int128)sB +
                                     (unsigned __int128)(N - 1) * (unsigned __int128)sN +
                                     (unsigned __int128)(D - 1) * (unsigned __int128)sK +
                                     (unsigned __int128)(D - 1) * (unsigned __int128)sL;
    if (extent >> 62)
        return fail(MISSLAP_ERR_INVALID, "%s: w strides (%lld, %lld, %lld, %lld): the last element's offset does not fit 62 "
                    "bits", who, (long long)sB, (long long)sN, (long long)sK, (long long)sL);
    if (!on_device && !(sL == 1 && sK == D && sN == D * D && sB == N * D * D))
        return fail(MISSLAP_ERR_INVALID, "%s: a strided w is a device array: set input_on_device (a host array is compact: "
                    "strides (N * D * D, D * D, D, 1))", who);
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int64_t misslap_points_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                                         int32_t has_outside) {
    if (points_batch_dims(B, N, M)) return -1;
    return (int64_t)points_carve(B, N, M, has_prices != 0, has_outside != 0).total;
}

namespace {
// misslap_solve_points_batch (whiten null), misslap_solve_points_batch_whitened (`who`; whiten: w and its strides) and
// misslap_solve_boxes_batch (boxes: its metric, D = 4)
int points_batch_call(const char *who, const WhitenView *whiten, int32_t boxes, int64_t B, int64_t N, int64_t M, int64_t D, const void *x,
                      int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d, const void *y, int64_t y_stride_b,
                      int64_t y_stride_m, int64_t y_stride_d, const int32_t *shapes, int32_t fast, const double *prices_in,
                      const misslap_options *opt_in, void *stream, void *workspace, int64_t workspace_bytes,
                      const double *outside, int64_t outside_ld, int32_t *sol, double *prices_out,
                      double *outside_prices_out, int32_t out_on_device, int32_t *status, int32_t *matching_size,
                      misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
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
    if (whiten && (rc = points_whiten_check(who, B, N, D, whiten->p, whiten->sB, whiten->sN, whiten->sK, whiten->sL,
                                            opt.input_on_device != 0)))
        return rc;
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
                 outside ? outside_ld : 0, fast, whiten ? *whiten : WhitenView{}, boxes};
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
}  // namespace

MISSLAP_API int misslap_solve_points_batch(int64_t B, int64_t N, int64_t M, int64_t D, const void *x, int64_t x_stride_b,
                                           int64_t x_stride_n, int64_t x_stride_d, const void *y, int64_t y_stride_b,
                                           int64_t y_stride_m, int64_t y_stride_d, const int32_t *shapes, int32_t fast,
                                           const double *prices_in, const misslap_options *opt_in, void *stream,
                                           void *workspace, int64_t workspace_bytes, const double *outside,
                                           int64_t outside_ld, int32_t *sol, double *prices_out,
                                           double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                           int32_t *matching_size, misslap_dense_batch_meta *meta,
                                           misslap_dense_batch_info *info) {
    return points_batch_call("misslap_solve_points_batch", nullptr, 0, B, N, M, D, x, x_stride_b, x_stride_n, x_stride_d, y,
                             y_stride_b, y_stride_m, y_stride_d, shapes, fast, prices_in, opt_in, stream, workspace,
                             workspace_bytes, outside, outside_ld, sol, prices_out, outside_prices_out, out_on_device, status,
                             matching_size, meta, info);
}

MISSLAP_API int misslap_solve_points_batch_whitened(int64_t B, int64_t N, int64_t M, int64_t D, const void *x,
                                                    int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d, const void *y,
                                                    int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d, const void *w,
                                                    int64_t w_stride_b, int64_t w_stride_n, int64_t w_stride_k,
                                                    int64_t w_stride_l, const int32_t *shapes, int32_t fast,
                                                    const double *prices_in, const misslap_options *opt_in, void *stream,
                                                    void *workspace, int64_t workspace_bytes, const double *outside,
                                                    int64_t outside_ld, int32_t *sol, double *prices_out,
                                                    double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                                    int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                    misslap_dense_batch_info *info) {
    const WhitenView wv{w, (long long)w_stride_b, (long long)w_stride_n, (long long)w_stride_k, (long long)w_stride_l};
    return points_batch_call("misslap_solve_points_batch_whitened", &wv, 0, B, N, M, D, x, x_stride_b, x_stride_n, x_stride_d, y,
                             y_stride_b, y_stride_m, y_stride_d, shapes, fast, prices_in, opt_in, stream, workspace,
                             workspace_bytes, outside, outside_ld, sol, prices_out, outside_prices_out, out_on_device, status,
                             matching_size, meta, info);
}
