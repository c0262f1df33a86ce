// abi_sparse_batch_outside.hpp -- C ABI: the sparse batch with an outside option per row, for partial assignments
// (misslap_solve_sparse_batch_outside, misslap_sparse_batch_outside_workspace_bytes; include/misslap.h).  The arguments
// are those of misslap_solve_sparse_batch_status (abi_sparse_batch_status.hpp) without the guard, plus the outside values;
// the two modes are batch_stream_call's (abi_batch_stream.hpp); the kernels are k_sparse_outside_check and
// k_sparse_outside_solve (kernels_sparse_batch.hpp).  Two launches, no guard; the verdict is formed in
// k_sparse_outside_solve, so nothing is read back between them.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_sparse_batch_status.hpp)
#pragma once

namespace {
// The workspace of one call: the check records, a block of Nmax + 1 row starts per problem, and with starting prices the
// staged [p0[:m_b], zeros(n_b)] of every problem at a leading dimension of Mmax + Nmax.
inline BatchCarve sparse_outside_carve(int64_t B, int64_t Nmax, int64_t Mmax, bool has_prices) {
    return batch_carve({sizeof(SparseBatchCheck) * (size_t)B, sizeof(int) * (size_t)B * (size_t)(Nmax + 1),
                        has_prices ? sizeof(double) * (size_t)B * (size_t)(Mmax + Nmax) : 0});
}

struct SparseOutsideCall {
    SparseStatusCall c;  // (guard: never)
    const double *d_outside;
    int64_t outside_ld;
};

// The two launches of a call on st: the check pass and the solve with its verdict.  Every pointer is a device pointer.
int sparse_outside_enqueue(hipStream_t st, const misslap_options &opt, const SparseOutsideCall &oc, void *ws,
                           const BatchStreamOut &d) {
    const SparseStatusCall &c = oc.c;
    const BatchCarve carve = sparse_outside_carve(c.B, c.Nmax, c.Mmax, c.d_p0 != nullptr);
    SparseBatchCheck *d_chk = carve.at<SparseBatchCheck>(ws, 0);
    int *d_rs = carve.at<int>(ws, 1);
    double *d_aug = c.d_p0 ? carve.at<double>(ws, 2) : nullptr;
    const long long aug_ld = (long long)(c.Mmax + c.Nmax);

    SparseOutsideCheckArgs k{};
    k.loc = c.d_loc;
    k.val = c.d_val;
    k.offsets = c.d_off;
    k.sizes = c.d_sizes;
    k.p0 = c.d_p0;
    k.p0_ld = c.prices_ld;
    k.row_start = d_rs;
    k.out = d_chk;
    k.outside = oc.d_outside;
    k.outside_ld = oc.outside_ld;
    k.aug = d_aug;
    k.aug_ld = aug_ld;
    k.Nmax = (int)c.Nmax;
    k.Mmax = (int)c.Mmax;
    hipLaunchKernelGGL(k_sparse_outside_check, dim3((unsigned)c.B), dim3(256), 0, st, k);
    HIP_TRY(hipGetLastError());

    SparseOutsideArgs a{};
    a.d.loc = c.d_loc;
    a.d.val = c.d_val;
    a.d.offsets = c.d_off;
    a.d.row_start = d_rs;
    a.d.chk = d_chk;
    a.sizes = c.d_sizes;
    a.fast = c.fast ? 1 : 0;
    a.status = d.status;
    a.matching_size = d.matching_size;
    a.outside = oc.d_outside;
    a.outside_ld = oc.outside_ld;
    a.prices = d.prices;
    a.outside_prices = d.outside_prices;
    a.Mmax = (int)c.Mmax;
    a.p0_ld = c.prices_ld;
    // (the carve is Nmax x (Mmax + Nmax).  No prices array for batch_solve: k_sparse_outside_solve writes the real
    // columns itself.)
    return batch_solve_launch(k_sparse_outside_solve, a, a.d.s, opt, c.B, c.Nmax, c.Mmax + c.Nmax, d.sol, c.Nmax, nullptr, 0,
                              d_aug, aug_ld, d.meta, d.info, st);
}
}  // namespace

MISSLAP_API int64_t misslap_sparse_batch_outside_workspace_bytes(int64_t B, int64_t Nmax, int64_t Mmax,
                                                                 int32_t has_prices) {
    if (B < 1 || B > 0x7fffffff || Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return -1;
    return (int64_t)sparse_outside_carve(B, Nmax, Mmax, has_prices != 0).total;
}

MISSLAP_API int misslap_solve_sparse_batch_outside(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                                   const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                                   const double *prices_in, int64_t prices_ld,
                                                   const misslap_options *opt_in, void *stream, void *workspace,
                                                   int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                                   const double *outside, int64_t outside_ld, int32_t *sol,
                                                   double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                                   int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                                   misslap_dense_batch_info *info) {
    BatchStreamCall k;
    k.t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_sparse_batch_outside",
                           "device, maximize, eps_start, max_iter, input_on_device and input_stream");
    if (rc) return rc;
    SparseOutsideCall oc{};
    SparseStatusCall &c = oc.c;
    if (!offsets) return fail(MISSLAP_ERR_INVALID, "null offsets");
    if ((rc = sparse_batch_offsets(B, offsets, &c.zmax))) return rc;
    c.B = B;
    c.nnz = offsets[B];
    if ((c.nnz > 0 && (!loc || !val)) || !sol || !status || !outside)
        return fail(MISSLAP_ERR_INVALID, "null loc / val / sol / status / outside");
    if (Nmax < 1 || Nmax > kSparseBatchMaxDim || Mmax < 1 || Mmax > kSparseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID, "Nmax x Mmax = %lld x %lld: each 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM (%d)",
                    (long long)Nmax, (long long)Mmax, kSparseBatchMaxDim);
    if (outside_ld != 0 && outside_ld < Nmax)
        return fail(MISSLAP_ERR_INVALID, "outside_ld = %lld: 0 (one value per problem) or >= Nmax = %lld",
                    (long long)outside_ld, (long long)Nmax);
    if (prices_in && prices_ld < 1) return fail(MISSLAP_ERR_INVALID, "prices_ld must be >= 1");
    c.Nmax = Nmax;
    c.Mmax = Mmax;
    c.prices_ld = prices_in ? prices_ld : 0;
    c.fast = fast;
    c.guard = false;
    c.d_loc = loc;
    c.d_val = val;
    c.d_off = reinterpret_cast<const long long *>(offsets_dev);
    c.d_sizes = reinterpret_cast<const long long *>(sizes);
    c.d_p0 = prices_in;
    oc.d_outside = outside;
    oc.outside_ld = outside_ld;
    const size_t nnz = (size_t)c.nnz;
    k.B = B;
    k.out.sol = sol;
    k.out.sol_cells = (size_t)B * (size_t)Nmax;
    k.out.status = status;
    k.out.matching_size = matching_size;
    k.out.prices = prices_out;
    k.out.prices_cells = (size_t)B * (size_t)Mmax;
    k.out.outside_prices = outside_prices_out;
    k.out.outside_cells = (size_t)B * (size_t)Nmax;
    k.out.meta = meta;
    k.out.info = info;
    k.out_on_device = out_on_device;
    k.stream = stream;
    k.workspace = workspace;
    k.workspace_bytes = workspace_bytes;
    k.carve_total = sparse_outside_carve(B, Nmax, Mmax, prices_in != nullptr).total;
    k.sizing = "misslap_sparse_batch_outside_workspace_bytes";
    k.device_input_missing = !offsets_dev;
    k.device_input = "a device copy of offsets and ";

    // (with a workspace sizes is a device array and offsets_dev is read; without, offsets and sizes are host arrays
    // however input_on_device is set, and outside lives where loc / val / prices_in live)
    return batch_stream_call(
        opt, k, batch_no_host_check,
        [&](DevScratch &tmp, hipStream_t st) {
            int rc = 0;
            if (!opt.input_on_device &&
                ((nnz && ((rc = upload(tmp, &c.d_loc, loc, 2 * nnz, st)) || (rc = upload(tmp, &c.d_val, val, nnz, st)))) ||
                 (rc = upload(tmp, &oc.d_outside, outside, outside_ld ? (size_t)B * (size_t)outside_ld : (size_t)B, st)) ||
                 (prices_in && (rc = upload(tmp, &c.d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
                return rc;
            c.d_sizes = nullptr;
            if ((rc = upload(tmp, &c.d_off, offsets, (size_t)B + 1, st))) return rc;
            return sizes ? upload(tmp, &c.d_sizes, sizes, (size_t)B * 2, st) : rc;
        },
        [&](hipStream_t st, void *ws, const BatchStreamOut &d) { return sparse_outside_enqueue(st, opt, oc, ws, d); });
}
