// abi_sparse_batch_status.hpp -- C ABI: the sparse batch with a verdict per problem, in stream order
// (misslap_solve_sparse_batch_status, misslap_sparse_batch_workspace_bytes; include/misslap.h).  The options and the
// offsets checks are those of misslap_solve_sparse_batch (abi_sparse_batch.hpp, abi_batch_common.hpp); the verdict is
// formed in k_sparse_batch_solve_status (kernels_sparse_batch.hpp), so nothing is read back between the launches.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_sparse_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the nnz + B row starts and the guard's cardinalities, each on a
// 256-byte boundary.
struct SparseStatusCarve {
    size_t chk = 0, rs = 0, card = 0, total = 0;
    SparseStatusCarve(int64_t B, int64_t nnz, bool guard) {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        rs = chk + up(sizeof(SparseBatchCheck) * (size_t)B);
        card = rs + up(sizeof(int) * ((size_t)nnz + (size_t)B));
        total = card + (guard ? up(sizeof(int) * (size_t)B) : 0);
    }
};

struct SparseStatusCall {
    int64_t B, nnz, zmax, Nmax, Mmax, prices_ld;
    const int32_t *d_loc;
    const double *d_val;
    const long long *d_off, *d_sizes;
    const double *d_p0;
    int32_t fast;
    bool guard;
};

// The three launches of a call on st: the check pass, the guard, the solve with its verdict.  Every pointer is a device
// pointer; nothing here allocates, waits or copies.
int sparse_batch_status_enqueue(hipStream_t st, const misslap_options &opt, const SparseStatusCall &c, void *ws,
                                int32_t *d_sol, double *d_prices, int32_t *d_status, int32_t *d_msize,
                                misslap_dense_batch_meta *d_meta, misslap_dense_batch_info *info) {
    const SparseStatusCarve carve(c.B, c.nnz, c.guard);
    char *base = static_cast<char *>(ws);
    SparseBatchCheck *d_chk = reinterpret_cast<SparseBatchCheck *>(base + carve.chk);
    int *d_rs = reinterpret_cast<int *>(base + carve.rs);
    int *d_card = c.guard ? reinterpret_cast<int *>(base + carve.card) : nullptr;

    hipLaunchKernelGGL(k_sparse_batch_check, dim3((unsigned)c.B), dim3(256), 0, st, c.d_loc, c.d_val, c.d_off, c.d_p0,
                       (long long)c.prices_ld, d_rs, d_chk);
    HIP_TRY(hipGetLastError());
    if (c.guard) {  // every clean problem within the cap on the device; the carve is that of misslap_solve_sparse_batch
        MatchBatchArgs g{};
        g.loc = c.d_loc;
        g.offsets = c.d_off;
        g.schk = d_chk;
        g.Ns = (int)std::min<int64_t>(c.zmax, kSparseBatchMaxDim);
        g.Ms = kSparseBatchMaxDim;
        g.size = d_card;
        hipLaunchKernelGGL(k_matching_batch<MatchSrc::Loc>, dim3((unsigned)c.B), dim3(kMatchBatchThreads),
                           matching_batch_lds_bytes(g.Ns, g.Ms, false), st, g);
        HIP_TRY(hipGetLastError());
    }
    SparseBatchStatusArgs a{};
    a.d.s.eps_b = nullptr;
    a.d.s.eps_opt = opt.eps_start;
    a.d.s.p0 = c.d_p0;
    a.d.s.p0_ld = c.prices_ld;
    a.d.s.maximize = opt.maximize ? 1 : 0;
    a.d.s.max_iter = opt.max_iter;
    a.d.s.Ns = (int)c.Nmax;
    a.d.s.Ms = (int)c.Mmax;
    a.d.s.sol = d_sol;
    a.d.s.sol_ld = c.Nmax;
    a.d.s.prices = d_prices;
    a.d.s.prices_ld = c.Mmax;
    a.d.s.meta = d_meta;
    a.d.loc = c.d_loc;
    a.d.val = c.d_val;
    a.d.offsets = c.d_off;
    a.d.row_start = d_rs;
    a.d.chk = d_chk;
    a.sizes = c.d_sizes;
    a.card = d_card;
    a.fast = c.fast ? 1 : 0;
    a.status = d_status;
    a.matching_size = d_msize;
    const int threads = batch_solve_threads((int)c.Nmax);
    const size_t lds = batch_solve_lds_bytes(c.Nmax, c.Mmax);
    // (the > 64 KB dynamic-LDS opt-in: a property of the function on the current device, set on the host without a wait)
    if (lds > 65536)
        HIP_TRY(hipFuncSetAttribute((const void *)k_sparse_batch_solve_status, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    hipLaunchKernelGGL(k_sparse_batch_solve_status, dim3((unsigned)c.B), dim3(threads), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->threads = threads;
        info->lds_bytes = (int32_t)lds;
    }
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int64_t misslap_sparse_batch_workspace_bytes(int64_t B, int64_t nnz, int32_t has_prices,
                                                         int32_t cardinality_check) {
    (void)has_prices;
    // (nnz + B row starts of 4 bytes: far below 2^63 for every B the call takes and every nnz a size_t of entries holds)
    if (B < 1 || B > 0x7fffffff || nnz < 0 || nnz > (int64_t)1 << 56) return -1;
    return (int64_t)SparseStatusCarve(B, nnz, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_sparse_batch_status(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                                  const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                                  const double *prices_in, int64_t prices_ld, int32_t cardinality_check,
                                                  const misslap_options *opt_in, void *stream, void *workspace,
                                                  int64_t workspace_bytes, int64_t Nmax, int64_t Mmax, int32_t *sol,
                                                  double *prices_out, int32_t out_on_device, int32_t *status,
                                                  int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                  misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_sparse_batch_status",
                           "device, maximize, eps_start, max_iter, input_on_device and input_stream");
    if (rc) return rc;
    SparseStatusCall c{};
    if (!offsets) return fail(MISSLAP_ERR_INVALID, "null offsets");
    if ((rc = sparse_batch_offsets(B, offsets, &c.zmax))) return rc;
    c.B = B;
    c.nnz = offsets[B];
    if ((c.nnz > 0 && (!loc || !val)) || !sol || !status) return fail(MISSLAP_ERR_INVALID, "null loc / val / sol / status");
    if (Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Nmax x Mmax = %lld x %lld: each 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)",
                    (long long)Nmax, (long long)Mmax, kSparseBatchMaxDim);
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.fast = fast;
    c.guard = cardinality_check != 0;
    const SparseStatusCarve carve(B, c.nnz, c.guard);

    if (workspace) {  // ---- stream-ordered: the caller's stream, the caller's memory, no wait
        if (!opt.input_on_device || !out_on_device || !meta || !offsets_dev)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass a device copy of offsets and a device meta array");
        if (workspace_bytes < (int64_t)carve.total || ((uintptr_t)workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned "
                        "(misslap_sparse_batch_workspace_bytes)", (long long)workspace_bytes, workspace, (long long)carve.total);
        if ((rc = batch_set_device(opt))) return rc;
        c.d_loc = loc;
        c.d_val = val;
        c.d_off = reinterpret_cast<const long long *>(offsets_dev);
        c.d_sizes = reinterpret_cast<const long long *>(sizes);
        c.d_p0 = prices_in;
        return sparse_batch_status_enqueue((hipStream_t)stream, opt, c, workspace, sol, prices_out, status, matching_size,
                                           meta, info);
    }

    // ---- the library's own scratch and stream, one wait at the end
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    const size_t nnz = (size_t)c.nnz, scells = (size_t)B * (size_t)Nmax, pcells = (size_t)B * (size_t)Mmax;
    DevScratch tmp;
    c.d_loc = loc;
    c.d_val = val;
    c.d_p0 = prices_in;
    if (!opt.input_on_device &&
        ((rc = upload(tmp, &c.d_loc, loc, 2 * nnz, st)) || (rc = upload(tmp, &c.d_val, val, nnz, st)) ||
         (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
        return rc;
    char *ws = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    int32_t *d_sol = sol, *d_status = status, *d_msize = matching_size;
    double *d_prices = prices_out;
    if ((rc = upload(tmp, &c.d_off, offsets, (size_t)B + 1, st)) ||
        (sizes && (rc = upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st))) || (rc = tmp.alloc(&ws, carve.total)) ||
        (rc = tmp.alloc(&d_meta, (size_t)B)))
        return rc;
    if (!out_on_device &&
        ((rc = tmp.alloc(&d_sol, scells)) || (rc = tmp.alloc(&d_status, (size_t)B)) ||
         (matching_size && (rc = tmp.alloc(&d_msize, (size_t)B))) || (prices_out && (rc = tmp.alloc(&d_prices, pcells)))))
        return rc;
    misslap_dense_batch_info launch{};
    if ((rc = sparse_batch_status_enqueue(st, opt, c, ws, d_sol, d_prices, d_status, d_msize, d_meta, &launch))) return rc;
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * scells, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (matching_size)
            HIP_TRY(hipMemcpyAsync(matching_size, d_msize, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
        if (prices_out) HIP_TRY(hipMemcpyAsync(prices_out, d_prices, sizeof(double) * pcells, hipMemcpyDeviceToHost, st));
    }
    if (meta) {
        const size_t w = std::min((size_t)stride, sizeof(misslap_dense_batch_meta));
        HIP_TRY(hipMemcpy2DAsync(meta, (size_t)stride, d_meta, sizeof(misslap_dense_batch_meta), w, (size_t)B,
                                 hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    tmp.drained = true;
    if (meta)  // (struct_size is an input field: the caller's value stays)
        for (int64_t b = 0; b < B; ++b)
            reinterpret_cast<misslap_dense_batch_meta *>(reinterpret_cast<char *>(meta) + (size_t)b * (size_t)stride)
                ->struct_size = stride;
    if (info) {
        *info = launch;
        info->wall_ms = now_ms() - t_start;
    }
    return MISSLAP_OK;
}
