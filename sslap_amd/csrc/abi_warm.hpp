// abi_warm.hpp -- C ABI: warm-started re-solves (prices out and in, values replaced in place, solve again).
// (part of the single translation unit misslap.hip; included in the order given there)
#pragma once

namespace {
// Both phases of a value update on device-resident values in entry order (the caller's sign): phase 1 checks and reduces
// and writes nothing, so a rejected update leaves the handle as it was; phase 2 rewrites every layout that carries a value.
int update_values_device(misslap_solver *h, const double *d_val, double *max_abs_change) {
    const long long nnz = h->nnz;
    const int flip = h->maximize ? 0 : 1;
    int rc;
    DevScratch tmp;
    WarmStats *d_st = nullptr;
    if ((rc = tmp.alloc(&d_st, 1))) return rc;
    HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(WarmStats), h->stream));
    const int grid = blocks_for(nnz, 256 * 8);
    if (h->f32) {
        hipLaunchKernelGGL(k_update_check<EdgesF32>, dim3(grid), dim3(256), 0, h->stream, EdgesF32{h->edges32}, d_val, nnz,
                           flip, 1, d_st);
    } else {
        hipLaunchKernelGGL(k_update_check<EdgesF64>, dim3(grid), dim3(256), 0, h->stream, EdgesF64{h->col, h->val64}, d_val,
                           nnz, flip, 0, d_st);
    }
    HIP_TRY(hipGetLastError());
    WarmStats st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    tmp.drained = true;
    if (st.err & kErrNonFinite) return fail(MISSLAP_ERR_INVALID, "the new values hold a NaN or an infinity; the handle is unchanged");
    if (st.err & kErrNotF32)
        return fail(MISSLAP_ERR_INVALID,
                    "a new value is not exactly representable in fp32, and this handle keeps 8 B/edge fp32 values (its values "
                    "at create were all fp32-exact); the handle is unchanged -- create it with options.force_f64_values = 1 "
                    "(Python: force_f64=True) to update it with arbitrary doubles");
    // phase 2: the row-major layout, then the tile-major copy and its overflow lists from it, then the candidate lines
    if (h->f32) {
        hipLaunchKernelGGL(k_update_edges_f32, dim3(grid), dim3(256), 0, h->stream, d_val, nnz, flip, h->edges32);
    } else {
        hipLaunchKernelGGL(k_update_edges_f64, dim3(grid), dim3(256), 0, h->stream, d_val, nnz, flip, h->val64);
    }
    if (h->tiled_ok) {
        const int *cols = h->f32 ? reinterpret_cast<const int *>(h->edges32) : h->col;
        const int cs = h->f32 ? 2 : 1;
        const EdgesF32 e32{h->edges32};
        const EdgesF64 e64{h->col, h->val64};
        const dim3 gs(blocks_for(h->tile_L, 256)), bs(256);
        switch (h->tiled_fmt) {
            case 0: hipLaunchKernelGGL((k_tile_revalue<EdgesF32, 0>), gs, bs, 0, h->stream, e32, cols, cs, h->row_ptr, h->n_rows, h->T, h->tile_cols, kTileRB, h->seg4, h->tile_L, h->tiled); break;
            case 1: hipLaunchKernelGGL((k_tile_revalue<EdgesF64, 1>), gs, bs, 0, h->stream, e64, cols, cs, h->row_ptr, h->n_rows, h->T, h->tile_cols, kTileRB, h->seg4, h->tile_L, h->tiled); break;
            case 2: hipLaunchKernelGGL((k_tile_revalue<EdgesF32, 2>), gs, bs, 0, h->stream, e32, cols, cs, h->row_ptr, h->n_rows, h->T, h->tile_cols, kTileRB, h->seg4, h->tile_L, h->tiled); break;
            default: hipLaunchKernelGGL((k_tile_revalue<EdgesF64, 3>), gs, bs, 0, h->stream, e64, cols, cs, h->row_ptr, h->n_rows, h->T, h->tile_cols, kTileRB, h->seg4, h->tile_L, h->tiled); break;
        }
        const dim3 gp(blocks_for(h->n_rows, 256));
        if (h->f32)
            hipLaunchKernelGGL(k_ovf_revalue<EdgesF32>, gp, bs, 0, h->stream, e32, h->row_ptr, h->n_rows, h->ovf_ptr, h->tiled, h->tiled_fmt, h->ovf_q);
        else
            hipLaunchKernelGGL(k_ovf_revalue<EdgesF64>, gp, bs, 0, h->stream, e64, h->row_ptr, h->n_rows, h->ovf_ptr, h->tiled, h->tiled_fmt, h->ovf_q);
    }
    if (h->cand)
        hipLaunchKernelGGL(k_clear_lines, dim3(blocks_for((long long)h->n_rows * kCandLanes, 256)), dim3(256), 0, h->stream,
                           h->cand, h->n_rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    // what create derived from the values: C (eps0, the fp32 filter's bound, lines_safe_eps)
    std::memcpy(&h->max_abs, &st.max_bits, sizeof(double));
    h->lines_safe_eps = (h->max_abs + h->pmax0) * 0x1p-44;
    set_filter(h);
    // a handle on which nothing has run yet starts its next solve as if created with these values
    if (h->untouched) {
        if ((rc = reset_state(h, h->price, h->pmax0, h->eps_start_opt))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (max_abs_change) std::memcpy(max_abs_change, &st.delta_bits, sizeof(double));
    return MISSLAP_OK;
}

// device-resident caller input: order the solver's stream behind its producer (sync_device_inputs)
int order_behind(misslap_solver *h, void *input_stream) {
    misslap_options o;
    std::memset(&o, 0, sizeof(o));
    o.input_on_device = 1;
    o.input_stream = input_stream;
    return sync_device_inputs(&o, h->stream);
}
}  // namespace

MISSLAP_API int misslap_get_prices(misslap_solver *h, double *out, int32_t out_on_device) {
    if (!h || !out) return fail(MISSLAP_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->price, sizeof(double) * (size_t)h->n_cols,
                      out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return MISSLAP_OK;
}

MISSLAP_API int misslap_update_values(misslap_solver *h, const double *val, int64_t nnz, int32_t on_device,
                                      void *input_stream, double *max_abs_change) {
    if (!h || !val) return fail(MISSLAP_ERR_INVALID, "null argument");
    if (h->world != 1) return fail(MISSLAP_ERR_STATE, "value updates are for single-GPU handles (this one is shard %d of %d)",
                                   h->rank, h->world);
    if (nnz != h->nnz)
        return fail(MISSLAP_ERR_INVALID, "%lld values given, the handle holds %lld entries", (long long)nnz, (long long)h->nnz);
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (on_device) {
        if ((rc = order_behind(h, input_stream))) return rc;
        return update_values_device(h, val, max_abs_change);
    }
    DevScratch tmp;
    double *d_val = nullptr;
    if ((rc = tmp.alloc(&d_val, (size_t)nnz))) return rc;
    HIP_TRY(hipMemcpyAsync(d_val, val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, h->stream));
    rc = update_values_device(h, d_val, max_abs_change);
    HIP_TRY(hipStreamSynchronize(h->stream));
    tmp.drained = true;
    return rc;
}

MISSLAP_API int misslap_update_dense(misslap_solver *h, const double *mat, int32_t on_device, void *input_stream,
                                     double *max_abs_change) {
    if (!h || !mat) return fail(MISSLAP_ERR_INVALID, "null argument");
    if (!h->dense) return fail(MISSLAP_ERR_STATE, "misslap_update_dense needs a handle made by misslap_create_dense");
    if (h->world != 1) return fail(MISSLAP_ERR_STATE, "value updates are for single-GPU handles");
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    DevScratch tmp;
    const size_t cells = (size_t)h->n_rows * (size_t)h->dense_cols;
    const double *d_mat = mat;
    if (on_device) {
        if ((rc = order_behind(h, input_stream))) return rc;
    } else {
        double *m = nullptr;
        if ((rc = tmp.alloc(&m, cells))) return rc;
        HIP_TRY(hipMemcpyAsync(m, mat, sizeof(double) * cells, hipMemcpyHostToDevice, h->stream));
        d_mat = m;
    }
    double *d_val = nullptr;
    WarmStats *d_st = nullptr;
    if ((rc = tmp.alloc(&d_val, (size_t)h->nnz))) return rc;
    if ((rc = tmp.alloc(&d_st, 1))) return rc;
    HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(WarmStats), h->stream));
    const int *cols = h->f32 ? reinterpret_cast<const int *>(h->edges32) : h->col;
    hipLaunchKernelGGL(k_dense_gather, dim3(blocks_for(h->n_rows, 4)), dim3(256), 0, h->stream, d_mat, h->n_rows,
                       (int)h->dense_cols, h->row_ptr, cols, h->f32 ? 2 : 1, d_val, d_st);
    HIP_TRY(hipGetLastError());
    WarmStats st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (st.err & kErrPattern)
        return fail(MISSLAP_ERR_INVALID, "the v >= 0 pattern of the matrix differs from the handle's (same valid entries per "
                                         "row required); the handle is unchanged");
    rc = update_values_device(h, d_val, max_abs_change);
    HIP_TRY(hipStreamSynchronize(h->stream));
    tmp.drained = true;
    return rc;
}

MISSLAP_API int misslap_resolve(misslap_solver *h, const double *prices, int32_t prices_on_device, float eps_start,
                                int32_t *person_to_object_out, misslap_meta *meta) {
    if (!h) return fail(MISSLAP_ERR_INVALID, "null handle");
    if (h->world != 1) return fail(MISSLAP_ERR_STATE, "misslap_resolve drives one GPU; a sharded warm start is not supported");
    if (meta && h->abi >= 2 && (meta->struct_size < (int32_t)offsetof(misslap_meta, edges_scanned) || meta->struct_size > 65536))
        return fail(MISSLAP_ERR_INVALID, "misslap_meta.struct_size = %d: set it to sizeof(misslap_meta) before the call", meta->struct_size);
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    DevScratch tmp;
    const double *src = h->price;  // NULL prices: start from the current ones
    if (prices && prices_on_device) {
        HIP_TRY(hipDeviceSynchronize());  // (the caller's buffer may still be in production on any of its streams)
        src = prices;
    } else if (prices) {
        double *d = nullptr;
        if ((rc = tmp.alloc(&d, (size_t)h->n_cols))) return rc;
        HIP_TRY(hipMemcpyAsync(d, prices, sizeof(double) * (size_t)h->n_cols, hipMemcpyHostToDevice, h->stream));
        src = d;
    }
    WarmStats *d_st = nullptr;
    if ((rc = tmp.alloc(&d_st, 1))) return rc;
    HIP_TRY(hipMemsetAsync(d_st, 0, sizeof(WarmStats), h->stream));
    hipLaunchKernelGGL(k_check_prices, dim3(blocks_for(h->n_cols, 256 * 8)), dim3(256), 0, h->stream, src, h->n_cols, d_st);
    HIP_TRY(hipGetLastError());
    WarmStats st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (st.err & (kErrNegativePrice | kErrNonFinite))
        return fail(MISSLAP_ERR_INVALID, "starting prices must be finite and >= 0 with the sign bit clear (%s); the handle is "
                                         "unchanged", (st.err & kErrNonFinite) ? "a NaN or an infinity" : "a negative value or -0.0");
    double pmax0;
    std::memcpy(&pmax0, &st.max_bits, sizeof(double));
    if ((rc = reset_state(h, src, pmax0, eps_start))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));  // (src may be a temporary)
    tmp.drained = true;
    return misslap_solve(h, person_to_object_out, meta);
}
