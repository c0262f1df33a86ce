// abi_points_finish.hpp -- C ABI: the reverse-auction finish behind misslap_solve_points_batch (include/misslap.h):
//   misslap_points_batch_reverse_finish
// One launch of k_points_reverse_finish<T, outside> (kernels_points_finish.hpp) on the caller's stream, on the solve's
// device outputs; no workspace.  The host-side argument checks are the solve's: the caps, D and the strides.
// (part of the single translation unit misslap.hip; included in the order given there, behind everything else)
#pragma once

namespace {
// The one launch on st, with the dynamic-LDS opt-in above 64 KiB.
template <class T>
int points_finish_launch(hipStream_t st, int64_t B, const PointsFinishArgs &a, bool out) {
    const size_t lds = dense_finish_lds_bytes(a.N, out ? a.M + a.N : a.M);
    auto launch = [&](auto kernel) -> int {
        if (lds > 65536)
            HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(kPointsFinishThreads), lds, st, a);
        HIP_TRY(hipGetLastError());
        return MISSLAP_OK;
    };
    return out ? launch(k_points_reverse_finish<T, true>) : launch(k_points_reverse_finish<T, false>);
}
}  // namespace

MISSLAP_API int misslap_points_batch_reverse_finish(int64_t B, int64_t N, int64_t M, int64_t D, const void *x,
                                                    int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                                    const void *y, int64_t y_stride_b, int64_t y_stride_m,
                                                    int64_t y_stride_d, const int32_t *shapes, const double *outside,
                                                    int64_t outside_ld, const misslap_options *opt_in, void *stream,
                                                    const int32_t *status, int32_t *sol, double *prices,
                                                    double *outside_prices, misslap_dense_batch_meta *meta,
                                                    int64_t *reverse_its, int32_t *reverse_left) {
    const char *who = "misslap_points_batch_reverse_finish";
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who, "device, maximize, max_iter, mat_dtype and input_on_device", true);
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
    if (!x || !y || !status || !sol || !prices || !meta || !reverse_its || !reverse_left)
        return fail(MISSLAP_ERR_INVALID, "null x / y / status / sol / prices / meta / reverse_its / reverse_left");
    if ((outside != nullptr) != (outside_prices != nullptr))
        return fail(MISSLAP_ERR_INVALID, "%s: outside and outside_prices go together (the outputs of the outside solve)", who);
    if (outside && outside_ld != 0 && outside_ld < N)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= N = %lld",
                    (long long)outside_ld, (long long)N);
    if ((rc = dense_strides_check(B, N, D, x_stride_b, x_stride_n, x_stride_d, who)) ||
        (rc = dense_strides_check(B, M, D, y_stride_b, y_stride_m, y_stride_d, who)))
        return rc;
    if ((rc = batch_set_device(opt))) return rc;
    PointsFinishArgs a{};
    a.x = {x, (long long)x_stride_b, (long long)x_stride_n, (long long)x_stride_d};
    a.y = {y, (long long)y_stride_b, (long long)y_stride_m, (long long)y_stride_d};
    a.N = N;
    a.M = M;
    a.D = (int)D;
    a.shapes = shapes;
    a.outside = outside;
    a.outside_ld = outside ? outside_ld : 0;
    a.maximize = opt.maximize ? 1 : 0;
    a.max_iter = opt.max_iter;
    a.status = status;
    a.sol = sol;
    a.prices = prices;
    a.outside_prices = outside_prices;
    a.meta = meta;
    a.its = reinterpret_cast<long long *>(reverse_its);
    a.left = reverse_left;
    return opt.mat_dtype == MISSLAP_DTYPE_F32 ? points_finish_launch<float>((hipStream_t)stream, B, a, outside != nullptr)
                                              : points_finish_launch<double>((hipStream_t)stream, B, a, outside != nullptr);
}
