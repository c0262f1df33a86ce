// abi_batch_stream.hpp -- the one call path of the six "verdict per problem, stream-ordered" batch entry points:
// misslap_solve_dense_batch_status (abi_dense_batch_status.hpp), misslap_solve_dense_batch_outside
// (abi_dense_batch_status.hpp), misslap_solve_sparse_batch_status (abi_sparse_batch_status.hpp),
// misslap_solve_sparse_batch_outside (abi_sparse_batch_status.hpp), misslap_solve_ell_batch and
// misslap_solve_ell_batch_outside (abi_ell_batch.hpp).  An entry point checks its own arguments, describes the call in a BatchStreamCall and supplies three steps; batch_stream_call runs them in either of
// the two modes of include/misslap.h:
//   with a workspace   every array is on the device: the launches go onto the caller's stream, nothing is allocated,
//                      copied or waited for;
//   without            the library's own stream and scratch: host arrays are uploaded, the outputs that live on the
//                      host are copied back, and the call waits once, at the end.
// (part of the single translation unit misslap.hip; included in the order given there, after abi_batch_common.hpp)
#pragma once

namespace {
// The output arrays of a call: the caller's, or (what the enqueue step is given) the device arrays behind them.
struct BatchStreamOut {
    int32_t *sol = nullptr;  // [sol_cells]
    size_t sol_cells = 0;
    int32_t *status = nullptr, *matching_size = nullptr;  // [B]; matching_size or null
    double *prices = nullptr;  // [prices_cells] or null
    size_t prices_cells = 0;
    double *outside_prices = nullptr;  // [outside_cells] or null: the second price array of the outside calls
    size_t outside_cells = 0;
    misslap_dense_batch_meta *meta = nullptr;  // [B]; the caller's may be null without a workspace
    misslap_dense_batch_info *info = nullptr;  // or null
};

struct BatchStreamCall {
    double t_start = 0;  // now_ms() on entry
    int64_t B = 0;
    BatchStreamOut out;  // as the caller passed them
    int32_t out_on_device = 0;
    void *stream = nullptr, *workspace = nullptr;
    int64_t workspace_bytes = 0;
    size_t carve_total = 0;        // what the call's sizing function returns
    const char *sizing = nullptr;  // that function's name
    // an input besides opt.input_on_device that a workspace call needs a device copy of: whether it is missing, and
    // how the error text names it
    bool device_input_missing = false;
    const char *device_input = "";
};

// host_check()         the checks of host-only inputs, made without a workspace before the device is touched
// upload(tmp, st)      without a workspace: every input that is not on the device yet, into scratch of tmp, copied on st
// enqueue(st, ws, d)   the launches of the call on st: ws is the carve, d the device outputs (d.meta never null, d.info
//                      or null takes the launch geometry); it allocates, waits for and copies nothing
template <class HostCheck, class Upload, class Enqueue>
int batch_stream_call(const misslap_options &opt, const BatchStreamCall &c, const HostCheck &host_check,
                      const Upload &upload, const Enqueue &enqueue) {
    const BatchStreamOut &out = c.out;
    int rc = 0;
    if (c.workspace) {
        if (!opt.input_on_device || !c.out_on_device || !out.meta || c.device_input_missing)
            return fail(MISSLAP_ERR_INVALID, "with a workspace every array is on the device: set input_on_device and "
                        "out_on_device, and pass %sa device meta array", c.device_input);
        if (c.workspace_bytes < (int64_t)c.carve_total || ((uintptr_t)c.workspace & 255))
            return fail(MISSLAP_ERR_INVALID, "workspace of %lld bytes at %p: %lld bytes, 256-byte aligned (%s)",
                        (long long)c.workspace_bytes, c.workspace, (long long)c.carve_total, c.sizing);
        if ((rc = batch_set_device(opt))) return rc;
        return enqueue((hipStream_t)c.stream, c.workspace, out);
    }

    int32_t stride = 0;
    if ((rc = batch_meta_stride(out.meta, &stride)) || (rc = host_check())) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;
    DevScratch tmp;
    if ((rc = upload(tmp, st))) return rc;
    char *ws = nullptr;
    misslap_dense_batch_info launch{};
    BatchStreamOut d = out;
    d.meta = nullptr;
    d.info = &launch;
    if ((rc = tmp.alloc(&ws, c.carve_total)) || (rc = tmp.alloc(&d.meta, (size_t)c.B))) return rc;
    if (!c.out_on_device &&
        ((rc = tmp.alloc(&d.sol, out.sol_cells)) || (rc = tmp.alloc(&d.status, (size_t)c.B)) ||
         (out.matching_size && (rc = tmp.alloc(&d.matching_size, (size_t)c.B))) ||
         (out.prices && (rc = tmp.alloc(&d.prices, out.prices_cells))) ||
         (out.outside_prices && (rc = tmp.alloc(&d.outside_prices, out.outside_cells)))))
        return rc;
    if ((rc = enqueue(st, ws, d))) return rc;
    if (!c.out_on_device) {
        auto back = [&](auto *host, const auto *dev, size_t n) {
            return host ? hipMemcpyAsync(host, dev, sizeof(*host) * n, hipMemcpyDeviceToHost, st) : hipSuccess;
        };
        HIP_TRY(back(out.sol, d.sol, out.sol_cells));
        HIP_TRY(back(out.status, d.status, (size_t)c.B));
        HIP_TRY(back(out.matching_size, d.matching_size, (size_t)c.B));
        HIP_TRY(back(out.prices, d.prices, out.prices_cells));
        HIP_TRY(back(out.outside_prices, d.outside_prices, out.outside_cells));
    }
    if ((rc = batch_meta_copy_back(out.meta, stride, d.meta, c.B, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    tmp.drained = true;
    batch_meta_keep_stride(out.meta, stride, c.B);
    if (out.info) {
        *out.info = launch;
        out.info->wall_ms = now_ms() - c.t_start;
    }
    return MISSLAP_OK;
}

inline int batch_no_host_check() { return MISSLAP_OK; }
}  // namespace
