// abi_boxes_batch.hpp -- C ABI: the batch solve and the candidate lists from two box sets, costs 1 - IoU or 1 - GIoU
// formed from the coordinates and never stored (include/misslap.h):
//   misslap_solve_boxes_batch, misslap_boxes_batch_candidates
// A box set is a point set of D = 4 coordinates (x1, y1, x2, y2), so the entry points share the call paths of the
// points ones (points_batch_call in abi_points_batch.hpp, points_candidates_call in abi_points_candidates.hpp: the same
// argument checks, modes, workspace -- misslap_points_batch_workspace_bytes -- and uploads); what differs is the check
// of the metric, made here before anything else, and which kernels are launched, behind the kernels of
// kernels_boxes_batch.hpp.
// (part of the single translation unit misslap.hip; included in the order given there, behind everything else)
#pragma once

namespace {
template <class T, bool Out>
struct PointsKernels<T, Out, 1 + MISSLAP_BOXES_METRIC_IOU> {
    static PointsCheckArgs check_args(const PointsCheckArgs &k, const WhitenView &) { return k; }
    static PointsBatchArgs solve_args(const WhitenView &) { return PointsBatchArgs{}; }
    static PointsBatchArgs &inner(PointsBatchArgs &a) { return a; }
    static constexpr auto check = k_boxes_batch_check<T, Out, false>;
    static constexpr auto solve = k_boxes_batch_solve<T, Out, false>;
};
template <class T, bool Out>
struct PointsKernels<T, Out, 1 + MISSLAP_BOXES_METRIC_GIOU> {
    static PointsCheckArgs check_args(const PointsCheckArgs &k, const WhitenView &) { return k; }
    static PointsBatchArgs solve_args(const WhitenView &) { return PointsBatchArgs{}; }
    static PointsBatchArgs &inner(PointsBatchArgs &a) { return a; }
    static constexpr auto check = k_boxes_batch_check<T, Out, true>;
    static constexpr auto solve = k_boxes_batch_solve<T, Out, true>;
};

int boxes_enqueue(hipStream_t st, const misslap_options &opt, const PointsCall &c, void *ws, const BatchStreamOut &d) {
    return c.boxes == MISSLAP_BOXES_METRIC_GIOU ? points_enqueue_wh<1 + MISSLAP_BOXES_METRIC_GIOU>(st, opt, c, ws, d)
                                                : points_enqueue_wh<1 + MISSLAP_BOXES_METRIC_IOU>(st, opt, c, ws, d);
}

template <class T, bool Giou>
int boxes_candidates_launch_as(hipStream_t st, const PointsCandidatesArgs &a) {
    hipLaunchKernelGGL((k_boxes_batch_candidates<T, Giou>), points_candidates_grid(a), dim3(kPointsCandidatesThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return MISSLAP_OK;
}
int boxes_candidates_launch(hipStream_t st, const PointsCandidatesArgs &a, int32_t metric, bool f32) {
    if (metric == MISSLAP_BOXES_METRIC_GIOU)
        return f32 ? boxes_candidates_launch_as<float, true>(st, a) : boxes_candidates_launch_as<double, true>(st, a);
    return f32 ? boxes_candidates_launch_as<float, false>(st, a) : boxes_candidates_launch_as<double, false>(st, a);
}

int boxes_metric_check(const char *who, int32_t metric) {
    if (metric != MISSLAP_BOXES_METRIC_IOU && metric != MISSLAP_BOXES_METRIC_GIOU)
        return fail(MISSLAP_ERR_INVALID, "%s: metric = %d: MISSLAP_BOXES_METRIC_IOU (%d) or MISSLAP_BOXES_METRIC_GIOU (%d)", who,
                    (int)metric, MISSLAP_BOXES_METRIC_IOU, MISSLAP_BOXES_METRIC_GIOU);
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int misslap_solve_boxes_batch(int64_t B, int64_t N, int64_t M, const void *a, int64_t a_stride_b,
                                          int64_t a_stride_n, int64_t a_stride_d, const void *b, int64_t b_stride_b,
                                          int64_t b_stride_m, int64_t b_stride_d, int32_t metric, const int32_t *shapes,
                                          int32_t fast, const double *prices_in, const misslap_options *opt_in, void *stream,
                                          void *workspace, int64_t workspace_bytes, const double *outside,
                                          int64_t outside_ld, int32_t *sol, double *prices_out, double *outside_prices_out,
                                          int32_t out_on_device, int32_t *status, int32_t *matching_size,
                                          misslap_dense_batch_meta *meta, misslap_dense_batch_info *info) {
    if (int rc = boxes_metric_check("misslap_solve_boxes_batch", metric)) return rc;
    return points_batch_call("misslap_solve_boxes_batch", nullptr, metric, B, N, M, 4, a, a_stride_b, a_stride_n, a_stride_d,
                             b, b_stride_b, b_stride_m, b_stride_d, shapes, fast, prices_in, opt_in, stream, workspace,
                             workspace_bytes, outside, outside_ld, sol, prices_out, outside_prices_out, out_on_device, status,
                             matching_size, meta, info);
}

MISSLAP_API int misslap_boxes_batch_candidates(int64_t B, int64_t N, int64_t M, const void *a, int64_t a_stride_b,
                                               int64_t a_stride_n, int64_t a_stride_d, const void *b, int64_t b_stride_b,
                                               int64_t b_stride_m, int64_t b_stride_d, int32_t metric, int64_t K,
                                               const int32_t *shapes, const double *limit, int64_t limit_ld,
                                               const misslap_options *opt_in, void *stream, int32_t *cols, double *vals,
                                               int32_t *counts, int32_t *rows) {
    if (int rc = boxes_metric_check("misslap_boxes_batch_candidates", metric)) return rc;
    return points_candidates_call("misslap_boxes_batch_candidates", nullptr, metric, B, N, M, 4, a, a_stride_b, a_stride_n,
                                  a_stride_d, b, b_stride_b, b_stride_m, b_stride_d, K, shapes, limit, limit_ld, opt_in,
                                  stream, cols, vals, counts, rows);
}
