// abi_matching_batch.hpp -- C ABI: the reference's Hopcroft-Karp on many small graphs in one call, one workgroup per
// graph (misslap_matching_batch / misslap_matching_dense_batch / misslap_matching_dense_batch_strided; the kernels are in kernels_matching_batch.hpp, the shared
// host helpers in abi_batch_common.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_sparse_batch.hpp)
#pragma once

namespace {
// The part both entry points share once every graph is accepted: the launch, the outputs, the info.
// launch(a, lds) starts the matcher of the caller's source on st with an LDS carve of lds bytes (Ns x Ms; the > 64 KB
// opt-in is never needed: 48 KB at the cap).
template <bool kDense, class Launch>
int matching_batch_run(hipStream_t st, DevScratch &tmp, int64_t B, MatchBatchArgs a, int32_t *size, int32_t *left,
                       int64_t left_ld, int32_t *right, int64_t right_ld, int32_t out_on_device,
                       misslap_matching_batch_info *info, double t_start, double t_checked, const Launch &launch) {
    int rc = 0;
    int *d_size = nullptr;
    if ((rc = tmp.alloc(&d_size, (size_t)B))) return rc;
    a.size = d_size;
    a.left = left;
    a.left_ld = left ? left_ld : 0;
    a.right = right;
    a.right_ld = right ? right_ld : 0;
    if (!out_on_device) {
        if (left && (rc = tmp.alloc(&a.left, (size_t)B * (size_t)left_ld))) return rc;
        if (right && (rc = tmp.alloc(&a.right, (size_t)B * (size_t)right_ld))) return rc;
    }
    EventPair ev;
    if ((rc = ev.create())) return rc;
    const size_t lds = matching_batch_lds_bytes(a.Ns, a.Ms, kDense);
    HIP_TRY(hipEventRecord(ev.e[0], st));
    launch(a, lds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(hipMemcpyAsync(size, d_size, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (!out_on_device) {
        if (left)
            HIP_TRY(hipMemcpyAsync(left, a.left, sizeof(int32_t) * (size_t)B * (size_t)left_ld, hipMemcpyDeviceToHost, st));
        if (right)
            HIP_TRY(hipMemcpyAsync(right, a.right, sizeof(int32_t) * (size_t)B * (size_t)right_ld, hipMemcpyDeviceToHost,
                                   st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    tmp.drained = true;
    if (info) {
        double ms = 0;
        if ((rc = ev.elapsed(&ms))) return rc;
        info->threads = kMatchBatchThreads;
        info->lds_bytes = (int32_t)lds;
        info->check_ms = t_checked - t_start;
        info->kernel_ms = ms;
        info->wall_ms = now_ms() - t_start;
    }
    return MISSLAP_OK;
}

int matching_batch_info_size(const misslap_matching_batch_info *info) {
    if (info && (info->struct_size < (int32_t)sizeof(misslap_matching_batch_info) || info->struct_size > 4096))
        return fail(MISSLAP_ERR_INVALID, "misslap_matching_batch_info.struct_size = %d: set it to sizeof (%d)",
                    info->struct_size, (int)sizeof(misslap_matching_batch_info));
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int misslap_matching_batch(int64_t B, const int32_t *loc, const int64_t *offsets, const misslap_options *opt_in,
                                       int32_t *size, int32_t *n_rows, int32_t *n_cols, int32_t *left_pairings,
                                       int64_t left_ld, int32_t *right_pairings, int64_t right_ld, int32_t out_on_device,
                                       misslap_matching_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_matching_batch", "device, input_on_device and input_stream");
    if (rc) return rc;
    if ((rc = matching_batch_info_size(info))) return rc;
    if (!loc || !offsets || !size || !n_rows || !n_cols) return fail(MISSLAP_ERR_INVALID, "null loc / offsets / size / n_rows / n_cols");
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 graphs", (long long)B);
    if ((left_pairings && left_ld < 1) || (right_pairings && right_ld < 1))
        return fail(MISSLAP_ERR_INVALID, "left_ld / right_ld must be >= 1");
    if (offsets[0] != 0) return fail(MISSLAP_ERR_INVALID, "offsets[0] = %lld: must be 0", (long long)offsets[0]);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t z = offsets[b + 1] - offsets[b];
        if (z < 0) return fail(MISSLAP_ERR_INVALID, "offsets must be non-decreasing (offsets[%lld] > offsets[%lld])",
                               (long long)b, (long long)b + 1);
        if (z > kMatchBatchMaxEntries)
            return fail(MISSLAP_ERR_INVALID, "graph %lld: %lld entries; a graph takes at most %d", (long long)b,
                        (long long)z, kMatchBatchMaxEntries);
    }
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;

    const size_t nnz = (size_t)offsets[B];
    DevScratch tmp;
    const int32_t *d_loc = loc;
    const long long *d_off = nullptr;
    MatchBatchCheck *d_chk = nullptr;
    if ((!opt.input_on_device && (rc = upload(tmp, &d_loc, loc, 2 * nnz, st))) ||
        (rc = upload(tmp, &d_off, offsets, (size_t)B + 1, st)) || (rc = tmp.alloc(&d_chk, (size_t)B)))
        return rc;
    hipLaunchKernelGGL(k_matching_batch_check, dim3((unsigned)B), dim3(256), 0, st, d_loc, d_off, d_chk);
    HIP_TRY(hipGetLastError());
    std::vector<MatchBatchCheck> chk((size_t)B);
    HIP_TRY(hipMemcpyAsync(chk.data(), d_chk, sizeof(MatchBatchCheck) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double t_checked = now_ms();

    // misslap_hopcroft_karp's checks on each graph with n = max row + 1, m = max column + 1 (feasibility_.pyx:245-246)
    int Ns = 1, Ms = 1;
    for (int64_t b = 0; b < B; ++b) {
        const MatchBatchCheck &c = chk[(size_t)b];
        if (offsets[b + 1] == offsets[b]) return fail(MISSLAP_ERR_INVALID, "graph %lld: no entries", (long long)b);
        const int64_t n = (int64_t)c.max_row + 1, m = (int64_t)c.max_col + 1;
        if (n < 0 || m < 0) return fail(MISSLAP_ERR_INVALID, "graph %lld: bad argument", (long long)b);
        if (c.first_bad >= 0) {
            if (c.bad_i < 0 || c.bad_j < 0)  // (i >= n and j >= m cannot happen: n and m are the maxima + 1)
                return fail(MISSLAP_ERR_INVALID, "graph %lld: loc entry %d = (%d, %d) outside %lld x %lld", (long long)b,
                            c.first_bad, c.bad_i, c.bad_j, (long long)n, (long long)m);
            return fail(MISSLAP_ERR_INVALID, "graph %lld: loc rows must be sorted in ascending order", (long long)b);
        }
        if (n > kMatchBatchMaxDim || m > kMatchBatchMaxDim)
            return fail(MISSLAP_ERR_INVALID, "graph %lld: %lld x %lld exceeds MISSLAP_MATCHING_BATCH_MAX_DIM (%d)",
                        (long long)b, (long long)n, (long long)m, kMatchBatchMaxDim);
        if ((left_pairings && n > left_ld) || (right_pairings && m > right_ld))
            return fail(MISSLAP_ERR_INVALID, "graph %lld: %lld x %lld does not fit left_ld = %lld / right_ld = %lld",
                        (long long)b, (long long)n, (long long)m, (long long)left_ld, (long long)right_ld);
        Ns = std::max(Ns, (int)n);
        Ms = std::max(Ms, (int)m);
    }
    for (int64_t b = 0; b < B; ++b) {
        n_rows[b] = chk[(size_t)b].max_row + 1;
        n_cols[b] = chk[(size_t)b].max_col + 1;
    }
    MatchBatchArgs a{};
    a.loc = d_loc;
    a.offsets = d_off;
    a.mchk = d_chk;
    a.Ns = Ns;
    a.Ms = Ms;
    return matching_batch_run<false>(st, tmp, B, a, size, left_pairings, left_ld, right_pairings, right_ld, out_on_device,
                                     info, t_start, t_checked, [&](const MatchBatchArgs &g, size_t lds) {
                                         hipLaunchKernelGGL(k_matching_batch<MatchSrc::Loc>, dim3((unsigned)B),
                                                            dim3(kMatchBatchThreads), lds, st, g);
                                     });
}

namespace {
// misslap_matching_dense_batch (strides null) and misslap_matching_dense_batch_strided (`who`)
int matching_dense_batch_call(const char *who, int64_t B, int64_t N, int64_t M, const void *mat, const int64_t *strides,
                              const int32_t *shapes, const misslap_options *opt_in, int32_t *size, int32_t *n_rows,
                              int32_t *n_cols, int32_t *left_pairings, int64_t left_ld, int32_t *right_pairings,
                              int64_t right_ld, int32_t out_on_device, misslap_matching_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, who,
                           "device, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    const bool finite = dense_take_entries_finite(&opt);
    if ((rc = matching_batch_info_size(info))) return rc;
    if (!mat || !size || !n_rows || !n_cols) return fail(MISSLAP_ERR_INVALID, "null mat / size / n_rows / n_cols");
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 graphs", (long long)B);
    if (N < 1 || M < 1 || N > 0x7fffffff || M > 0x7fffffff)
        return fail(MISSLAP_ERR_INVALID, "a %lld x %lld stack: N and M must be 1 .. 2^31 - 1", (long long)N, (long long)M);
    if ((left_pairings && left_ld < 1) || (right_pairings && right_ld < 1))
        return fail(MISSLAP_ERR_INVALID, "left_ld / right_ld must be >= 1");
    DenseStrides str_arg{};
    const DenseStrides *str = nullptr;
    if ((rc = dense_stack_layout(who, opt, B, N, M, strides, &str_arg, &str, finite))) return rc;
    // each graph is its slice (feasibility_.pyx:250-251)
    int Ns = 1, Ms = 1;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = shapes ? shapes[2 * b] : N, m = shapes ? shapes[2 * b + 1] : M;
        if (shapes && (n < 1 || n > N || m < 1 || m > M))
            return fail(MISSLAP_ERR_INVALID, "graph %lld: shape (%lld, %lld) outside 1 .. %lld x 1 .. %lld", (long long)b,
                        (long long)n, (long long)m, (long long)N, (long long)M);
        if (n > kMatchBatchMaxDim || m > kMatchBatchMaxDim)
            return fail(MISSLAP_ERR_INVALID, "graph %lld: %lld x %lld exceeds MISSLAP_MATCHING_BATCH_MAX_DIM (%d)",
                        (long long)b, (long long)n, (long long)m, kMatchBatchMaxDim);
        if ((left_pairings && n > left_ld) || (right_pairings && m > right_ld))
            return fail(MISSLAP_ERR_INVALID, "graph %lld: %lld x %lld does not fit left_ld = %lld / right_ld = %lld",
                        (long long)b, (long long)n, (long long)m, (long long)left_ld, (long long)right_ld);
        Ns = std::max(Ns, (int)n);
        Ms = std::max(Ms, (int)m);
    }
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    DevScratch tmp;
    const void *d_mat = mat;  // elements of opt.mat_dtype
    const int *d_shapes = nullptr;
    if ((!opt.input_on_device &&
         (rc = upload_stack(tmp, &d_mat, mat, (size_t)B * (size_t)N * (size_t)M, opt.mat_dtype, st))) ||
        (shapes && (rc = upload(tmp, &d_shapes, shapes, (size_t)B * 2, st))))
        return rc;
    for (int64_t b = 0; b < B; ++b) {
        n_rows[b] = shapes ? shapes[2 * b] : (int32_t)N;
        n_cols[b] = shapes ? shapes[2 * b + 1] : (int32_t)M;
    }
    MatchBatchArgs a{};
    a.mat = d_mat;
    a.N = N;
    a.M = M;
    a.shapes = d_shapes;
    a.Ns = Ns;
    a.Ms = Ms;
    return matching_batch_run<true>(st, tmp, B, a, size, left_pairings, left_ld, right_pairings, right_ld, out_on_device,
                                    info, t_start, now_ms(), [&](const MatchBatchArgs &g, size_t lds) {
                                        dense_dispatch(opt.mat_dtype, str, finite, [&](auto t, auto lay) {
                                            dense_guard_launch<decltype(t)>(st, B, g, lay, lds);
                                        });
                                    });
}
}  // namespace

MISSLAP_API int misslap_matching_dense_batch(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                                             const misslap_options *opt_in, int32_t *size, int32_t *n_rows,
                                             int32_t *n_cols, int32_t *left_pairings, int64_t left_ld,
                                             int32_t *right_pairings, int64_t right_ld, int32_t out_on_device,
                                             misslap_matching_batch_info *info) {
    return matching_dense_batch_call("misslap_matching_dense_batch", B, N, M, mat, nullptr, shapes, opt_in, size, n_rows,
                                     n_cols, left_pairings, left_ld, right_pairings, right_ld, out_on_device, info);
}

MISSLAP_API int misslap_matching_dense_batch_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                                     int64_t stride_m, const void *mat, const int32_t *shapes,
                                                     const misslap_options *opt_in, int32_t *size, int32_t *n_rows,
                                                     int32_t *n_cols, int32_t *left_pairings, int64_t left_ld,
                                                     int32_t *right_pairings, int64_t right_ld, int32_t out_on_device,
                                                     misslap_matching_batch_info *info) {
    const int64_t strides[3] = {stride_b, stride_n, stride_m};
    return matching_dense_batch_call("misslap_matching_dense_batch_strided", B, N, M, mat, strides, shapes, opt_in, size,
                                     n_rows, n_cols, left_pairings, left_ld, right_pairings, right_ld, out_on_device, info);
}
