// abi_points_candidates.hpp -- C ABI: two point sets into padded candidate lists for misslap_solve_ell_batch
// (include/misslap.h):
//   misslap_points_batch_candidates, misslap_points_batch_candidates_whitened
// One launch of k_points_candidates<T> (kernels_points_candidates.hpp) or, with a whitening matrix per row, of
// k_points_whiten_candidates<T> (kernels_points_whiten.hpp, launched by abi_points_whiten.hpp) on the caller's stream: device pointers only, no
// workspace, nothing waited for or read back.  The host-side argument checks are the points solve's (the caps, D, the
// strides) and 1 <= K <= MISSLAP_POINTS_CANDIDATES_MAX_K.
// (part of the single translation unit misslap.hip; included in the order given there, behind everything else)
#pragma once

namespace {
// The one launch on st: a wavefront per row, four rows per workgroup, the problems along y (a workgroup strides over
// them where B exceeds what the grid's y takes).
inline dim3 points_candidates_grid(const PointsCandidatesArgs &a) {
    const unsigned gx = (unsigned)((a.N + 3) / 4);
    const long long cap = std::max<long long>(1, std::min<long long>(65535, (1ll << 22) / gx));
    return dim3(gx, (unsigned)std::min<long long>(a.B, cap));
}
template <class T>
int points_candidates_launch(hipStream_t st, const PointsCandidatesArgs &a) {
    hipLaunchKernelGGL(k_points_candidates<T>, points_candidates_grid(a), dim3(kPointsCandidatesThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return MISSLAP_OK;
}
// (abi_points_whiten.hpp: the same launch of k_points_whiten_candidates<float or double>)
int points_whiten_candidates_launch(hipStream_t st, const PointsCandidatesArgs &a, const WhitenView &w, bool f32);
// (abi_boxes_batch.hpp: the same launch of k_boxes_batch_candidates<float or double, the metric>)
int boxes_candidates_launch(hipStream_t st, const PointsCandidatesArgs &a, int32_t metric, bool f32);

// misslap_points_batch_candidates (whiten null), misslap_points_batch_candidates_whitened (`who`) and
// misslap_boxes_batch_candidates (boxes: its metric, D = 4)
int points_candidates_call(const char *who, const WhitenView *whiten, int32_t boxes, int64_t B, int64_t N, int64_t M, int64_t D,
                           const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d, const void *y,
                           int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d, int64_t K, const int32_t *shapes,
                           const double *limit, int64_t limit_ld, const misslap_options *opt_in, void *stream, int32_t *cols,
                           double *vals, int32_t *counts, int32_t *rows) {
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who, "device, mat_dtype and input_on_device", true);
    if (rc) return rc;
    if (opt.mat_dtype != MISSLAP_DTYPE_F64 && opt.mat_dtype != MISSLAP_DTYPE_F32)
        return fail(MISSLAP_ERR_INVALID, "%s takes coordinates of MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32, got mat_dtype = %d",
                    who, (int)opt.mat_dtype);
    if (!opt.input_on_device) return fail(MISSLAP_ERR_INVALID, "%s: every array is on the device: set input_on_device", who);
    if (const char *why = points_batch_dims(B, N, M))
        return fail(MISSLAP_ERR_INVALID, "B, N, M = %lld, %lld, %lld: %s (%d)", (long long)B, (long long)N, (long long)M, why,
                    kPointsBatchMaxDim);
    if (D < 1 || D > kPointsBatchMaxCoords)
        return fail(MISSLAP_ERR_INVALID, "D = %lld: 1 .. MISSLAP_POINTS_BATCH_MAX_COORDS (%d) coordinates", (long long)D,
                    kPointsBatchMaxCoords);
    if (K < 1 || K > kPointsCandidatesMaxK)
        return fail(MISSLAP_ERR_INVALID, "K = %lld: 1 .. MISSLAP_POINTS_CANDIDATES_MAX_K (%d) candidates per row",
                    (long long)K, kPointsCandidatesMaxK);
    if (!x || !y || !cols || !vals || !counts || !rows)
        return fail(MISSLAP_ERR_INVALID, "null x / y / cols / vals / counts / rows");
    if (whiten && (rc = points_whiten_check(who, B, N, D, whiten->p, whiten->sB, whiten->sN, whiten->sK, whiten->sL, true)))
        return rc;
    if (limit && limit_ld != 0 && limit_ld < N)
        return fail(MISSLAP_ERR_INVALID, "limit_ld = %lld: 0 (one value per problem) or >= N = %lld", (long long)limit_ld,
                    (long long)N);
    if ((rc = dense_strides_check(B, N, D, x_stride_b, x_stride_n, x_stride_d, who)) ||
        (rc = dense_strides_check(B, M, D, y_stride_b, y_stride_m, y_stride_d, who)))
        return rc;
    if ((rc = batch_set_device(opt))) return rc;
    PointsCandidatesArgs a{};
    a.x = {x, (long long)x_stride_b, (long long)x_stride_n, (long long)x_stride_d};
    a.y = {y, (long long)y_stride_b, (long long)y_stride_m, (long long)y_stride_d};
    a.N = N;
    a.M = M;
    a.B = (int)B;
    a.D = (int)D;
    a.K = (int)K;
    a.shapes = shapes;
    a.limit = limit;
    a.limit_ld = limit ? limit_ld : 0;
    a.cols = cols;
    a.vals = vals;
    a.counts = counts;
    a.rows = rows;
    if (boxes) return boxes_candidates_launch((hipStream_t)stream, a, boxes, opt.mat_dtype == MISSLAP_DTYPE_F32);
    if (whiten) return points_whiten_candidates_launch((hipStream_t)stream, a, *whiten, opt.mat_dtype == MISSLAP_DTYPE_F32);
    return opt.mat_dtype == MISSLAP_DTYPE_F32 ? points_candidates_launch<float>((hipStream_t)stream, a)
                                              : points_candidates_launch<double>((hipStream_t)stream, a);
}
}  // namespace

MISSLAP_API int misslap_points_batch_candidates(int64_t B, int64_t N, int64_t M, int64_t D, const void *x,
                                                int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d, const void *y,
                                                int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d, int64_t K,
                                                const int32_t *shapes, const double *limit, int64_t limit_ld,
                                                const misslap_options *opt_in, void *stream, int32_t *cols, double *vals,
                                                int32_t *counts, int32_t *rows) {
    return points_candidates_call("misslap_points_batch_candidates", nullptr, 0, B, N, M, D, x, x_stride_b, x_stride_n,
                                  x_stride_d, y, y_stride_b, y_stride_m, y_stride_d, K, shapes, limit, limit_ld, opt_in, stream,
                                  cols, vals, counts, rows);
}

MISSLAP_API int misslap_points_batch_candidates_whitened(int64_t B, int64_t N, int64_t M, int64_t D, const void *x,
                                                         int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                                         const void *y, int64_t y_stride_b, int64_t y_stride_m,
                                                         int64_t y_stride_d, const void *w, int64_t w_stride_b,
                                                         int64_t w_stride_n, int64_t w_stride_k, int64_t w_stride_l, int64_t K,
                                                         const int32_t *shapes, const double *limit, int64_t limit_ld,
                                                         const misslap_options *opt_in, void *stream, int32_t *cols,
                                                         double *vals, int32_t *counts, int32_t *rows) {
    const WhitenView wv{w, (long long)w_stride_b, (long long)w_stride_n, (long long)w_stride_k, (long long)w_stride_l};
    return points_candidates_call("misslap_points_batch_candidates_whitened", &wv, 0, B, N, M, D, x, x_stride_b, x_stride_n,
                                  x_stride_d, y, y_stride_b, y_stride_m, y_stride_d, K, shapes, limit, limit_ld, opt_in, stream,
                                  cols, vals, counts, rows);
}
