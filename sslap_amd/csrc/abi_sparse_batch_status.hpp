// abi_sparse_batch_status.hpp -- C ABI: the sparse batch with a verdict per problem, in stream order
// (misslap_solve_sparse_batch_status, misslap_sparse_batch_workspace_bytes; include/misslap.h).  The options and the
// offsets checks are those of misslap_solve_sparse_batch (abi_sparse_batch.hpp, abi_batch_common.hpp), the two modes of
// the call are batch_stream_call's (abi_batch_stream.hpp); the verdict is formed in k_sparse_batch_solve_status
// (kernels_sparse_batch.hpp), so nothing is read back between the launches.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_sparse_batch.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, the nnz + B row starts and the guard's cardinalities.
inline BatchCarve sparse_status_carve(int64_t B, int64_t nnz, bool guard) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * ((size_t)nnz + (size_t)B),
                        guard ? sizeof(int) * (size_t)B : 0});
}

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
// pointer.
int sparse_batch_status_enqueue(hipStream_t st, const misslap_options &opt, const SparseStatusCall &c, void *ws,
                                const BatchStreamOut &d) {
    const BatchCarve carve = sparse_status_carve(c.B, c.nnz, c.guard);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    int *d_card = c.guard ? carve.at<int>(ws, 2) : nullptr;

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
    a.d.loc = c.d_loc;
    a.d.val = c.d_val;
    a.d.offsets = c.d_off;
    a.d.row_start = d_rs;
    a.d.chk = d_chk;
    a.sizes = c.d_sizes;
    a.card = d_card;
    a.fast = c.fast ? 1 : 0;
    a.status = d.status;
    a.matching_size = d.matching_size;
    return batch_solve_launch(k_sparse_batch_solve_status, a, a.d.s, opt, c.B, c.Nmax, c.Mmax, d.sol, c.Nmax, d.prices,
                              c.Mmax, c.d_p0, c.prices_ld, d.meta, d.info, st);
}
}  // namespace

MISSLAP_API int64_t misslap_sparse_batch_workspace_bytes(int64_t B, int64_t nnz, int32_t has_prices,
                                                         int32_t cardinality_check) {
    (void)has_prices;
    // (nnz + B row starts of 4 bytes: far below 2^63 for every B the call takes and every nnz a size_t of entries holds)
    if (B < 1 || B > 0x7fffffff || nnz < 0 || nnz > (int64_t)1 << 56) return -1;
    return (int64_t)sparse_status_carve(B, nnz, cardinality_check != 0).total;
}

MISSLAP_API int misslap_solve_sparse_batch_status(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                                  const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                                  const double *prices_in, int64_t prices_ld, int32_t cardinality_check,
                                                  const misslap_options *opt_in, void *stream, void *workspace,
                                                  int64_t workspace_bytes, int64_t Nmax, int64_t Mmax, int32_t *sol,
                                                  double *prices_out, int32_t out_on_device, int32_t *status,
                                                  int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                  misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
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
    c.d_loc = loc;
    c.d_val = val;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    const size_t nnz = (size_t)c.nnz;
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)Nmax;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)B * (size_t)Mmax;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = sparse_status_carve(B, c.nnz, c.guard).total;
    k.sizing = "misslap_sparse_batch_workspace_bytes";
    k.device_input_missing = !offsets_dev;
    k.device_input = "a device copy of offsets and ";

    // (with a workspace sizes is a device array and offsets_dev is read; without, offsets and sizes are host arrays
    // however input_on_device is set)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            if (!opt.input_on_device &&
                ((rc = upload(tmp, &c.d_loc, loc, 2 * nnz, st)) || (rc = upload(tmp, &c.d_val, val, nnz, st)) ||
                 (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
                return rc;
            c.d_sizes = nullptr;
            if ((rc = upload(tmp, &c.d_off, offsets, (size_t)B + 1, st))) return rc;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_batch_status_enqueue(st, opt, c, ws, d); });
}
