// abi_batch_common.hpp -- what the one-workgroup-per-problem entry points share: the all-or-nothing solves
// (abi_dense_batch.hpp, abi_sparse_batch.hpp), the matching batch (abi_matching_batch.hpp) and the five solves with a
// verdict per problem (abi_batch_stream.hpp and its users).  The options whitelist, the device and stream, the meta
// stride and the records' way back to it, the host guards' thread pool, the starting-price texts, the workspace carve
// (batch_carve), the one solve launch (batch_solve_launch) and the all-or-nothing solve around it (batch_solve_run).
// (part of the single translation unit misslap.hip; included in the order given there, before abi_batch_stream.hpp)
#pragma once

namespace {
// normalise_options, then `who` takes the fields listed in `takes` only (the solver's other options must be 0);
// typed_mat: `who` reads mat_dtype (the dense stacks), every other entry point takes float64 only
int batch_options(const misslap_options *opt_in, misslap_options *opt, const char *who, const char *takes,
                  bool typed_mat = false) {
    int abi = 0;
    int rc = normalise_options(opt_in, opt, &abi);
    if (rc || (!typed_mat && (rc = float64_only(*opt, who)))) return rc;
    if (opt->tail_threshold > 0 || opt->force_f64_values || opt->profile || opt->shard_world > 1 || opt->rounds_per_sync ||
        opt->tiled_min_K || opt->tiled_shape || opt->tiled_force || opt->shard_min_K || opt->cand_mode || opt->nnz_limit ||
        opt->cand_build_max_K || opt->cand_refresh_min)
        return fail(MISSLAP_ERR_INVALID, "%s takes %s only: every other option must be 0", who, takes);
    return MISSLAP_OK;
}

// the calling thread's stream on a device (created on first use, kept for the life of the thread's process)
int thread_stream(int device, hipStream_t *out) {
    static thread_local std::vector<std::pair<int, hipStream_t>> streams;
    for (const auto &s : streams)
        if (s.first == device) {
            *out = s.second;
            return MISSLAP_OK;
        }
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    streams.emplace_back(device, st);
    *out = st;
    return MISSLAP_OK;
}

// opt.device made current
int batch_set_device(const misslap_options &opt) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MISSLAP_ERR_NO_DEVICE, "no HIP device available: libmisslap has no CPU fallback");
    if (opt.device < 0 || opt.device >= ndev) return fail(MISSLAP_ERR_INVALID, "device %d out of range", opt.device);
    HIP_TRY(hipSetDevice(opt.device));
    return MISSLAP_OK;
}

// opt.device made current, the calling thread's stream on it, ordered behind the producer stream of device inputs
int batch_device(const misslap_options &opt, hipStream_t *st) {
    int rc = batch_set_device(opt);
    if (rc) return rc;
    rc = thread_stream(opt.device, st);
    if (rc) return rc;
    return sync_device_inputs(&opt, *st);
}

// n elements of host array h into a new scratch buffer on the device (*d), copied on st
template <class T>
int upload(DevScratch &tmp, const T **d, const void *h, size_t n, hipStream_t st) {
    T *p = nullptr;
    int rc = tmp.alloc(&p, n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p, h, sizeof(T) * n, hipMemcpyHostToDevice, st));
    *d = p;
    return MISSLAP_OK;
}

// the stride of the caller's meta records: meta[0].struct_size (0 without meta)
int batch_meta_stride(const misslap_dense_batch_meta *meta, int32_t *stride) {
    *stride = 0;
    if (!meta) return MISSLAP_OK;
    *stride = meta[0].struct_size;
    if (*stride < (int32_t)offsetof(misslap_dense_batch_meta, its) || *stride > 4096)
        return fail(MISSLAP_ERR_INVALID, "misslap_dense_batch_meta.struct_size = %d: set it to sizeof (%d) in meta[0]",
                    *stride, (int)sizeof(misslap_dense_batch_meta));
    return MISSLAP_OK;
}

// Whether the matching guard of a batch runs on the device (k_matching_batch behind the check pass) or on the host
// threads.  One graph on one CU is slower than the host matcher (a DFS step waits on L2), so the device wins only once
// the batch spreads over the GPU: measured it lost at B = 1 (dense and sparse) and at sparse 64 x 2048,
// and won at dense B >= 64 and sparse B >= 256.
inline bool dense_guard_on_device(int64_t B) { return B >= 64; }
inline bool sparse_guard_on_device(int64_t B) { return B >= 256; }

// the two events around a launch
struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    int create() {
        HIP_TRY(hipEventCreate(&e[0]));
        HIP_TRY(hipEventCreate(&e[1]));
        return MISSLAP_OK;
    }
    int elapsed(double *ms) {
        float f = 0;
        HIP_TRY(hipEventElapsedTime(&f, e[0], e[1]));
        *ms = f;
        return MISSLAP_OK;
    }
    ~EventPair() {
        if (e[0]) (void)hipEventDestroy(e[0]);
        if (e[1]) (void)hipEventDestroy(e[1]);
    }
};

// The host side of a matching guard: item(t) for every t in [0, count) on up to 16 threads.
template <class F>
int run_host_guards(int64_t count, const F &item) {
    std::atomic<int64_t> next{0};
    std::atomic<int> oom{0};
    auto work = [&]() {
        for (int64_t t; (t = next.fetch_add(1)) < count;) {
            try {
                item(t);
            } catch (const std::bad_alloc &) {
                oom = 1;
            }
        }
    };
    const int nthr = (int)std::min<int64_t>(count, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    std::vector<std::thread> pool;
    for (int t = 1; t < nthr; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (oom) return fail(MISSLAP_ERR_HIP, "out of host memory in the matching guard");
    return MISSLAP_OK;
}

// the checks of AuctionSolver.resolve on problem b's starting prices (bad: bit 0 NaN / infinity, bit 1 sign bit set)
int reject_bad_prices(int64_t b, int bad) {
    if (bad & 1) return fail(MISSLAP_ERR_INVALID, "problem %lld: prices hold a NaN or an infinity", (long long)b);
    if (bad & 2)
        return fail(MISSLAP_ERR_INVALID, "problem %lld: prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
                    (long long)b);
    return MISSLAP_OK;
}

// a wavefront bids for one list position at a time: enough wavefronts for the first round's bidders, at most 16
inline int batch_solve_threads(int Ns) { return Ns <= 256 ? 256 : (Ns <= 512 ? 512 : 1024); }

// Byte offsets of the segments of a workspace, each on a 256-byte boundary, and their total (a segment of 0 bytes takes
// no room).  Every *_workspace_bytes function returns the total of the carve its enqueue step reads.
struct BatchCarve {
    size_t off[4] = {0, 0, 0, 0}, total = 0;
    template <class T>
    T *at(void *ws, int seg) const {
        return reinterpret_cast<T *>(static_cast<char *>(ws) + off[seg]);
    }
};
inline BatchCarve batch_carve(std::initializer_list<size_t> bytes) {
    BatchCarve c;
    int i = 0;
    for (size_t b : bytes) {
        c.off[i++] = c.total;
        c.total += (b + 255) & ~(size_t)255;
    }
    return c;
}

// The solve launch of every batch entry point: one workgroup per problem on the LDS carve Ns x Ms.  `s` is the
// BatchSolveArgs inside `a`; the caller has set a's own fields and s.eps_b (null unless the call takes an eps per
// problem), the rest of s is set here.  The > 64 KB dynamic-LDS opt-in is a property of the function on the current
// device, set on the host without a wait.  ev: the two events recorded around the launch, or null.  Nothing here
// allocates, waits or copies; info (or null) is zeroed but for the launch geometry.
template <class Args>
int batch_solve_launch(void (*kernel)(Args), Args &a, BatchSolveArgs &s, const misslap_options &opt, int64_t B, int64_t Ns,
                       int64_t Ms, int32_t *sol, int64_t sol_ld, double *prices, int64_t prices_ld, const double *p0,
                       int64_t p0_ld, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info, hipStream_t st,
                       EventPair *ev = nullptr) {
    s.eps_opt = opt.eps_start;
    s.p0 = p0;
    s.p0_ld = p0_ld;
    s.maximize = opt.maximize ? 1 : 0;
    s.max_iter = opt.max_iter;
    s.Ns = (int)Ns;
    s.Ms = (int)Ms;
    s.sol = sol;
    s.sol_ld = sol_ld;
    s.prices = prices;
    s.prices_ld = prices_ld;
    s.meta = meta;
    const int threads = batch_solve_threads((int)Ns);
    const size_t lds = batch_solve_lds_bytes(Ns, Ms);
    if (lds > 65536) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (ev) HIP_TRY(hipEventRecord(ev->e[0], st));
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(threads), lds, st, a);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev->e[1], st));
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->threads = threads;
        info->lds_bytes = (int32_t)lds;
    }
    return MISSLAP_OK;
}

// The meta records of a call back into the caller's host array of `stride`-byte records: the copy on st, and, once st
// has been waited for, the caller's struct_size put back (it is an input field).  Both do nothing without meta.
int batch_meta_copy_back(misslap_dense_batch_meta *meta, int32_t stride, const misslap_dense_batch_meta *d_meta, int64_t B,
                         hipStream_t st) {
    if (!meta) return MISSLAP_OK;
    const size_t w = std::min((size_t)stride, sizeof(misslap_dense_batch_meta));
    HIP_TRY(hipMemcpy2DAsync(meta, (size_t)stride, d_meta, sizeof(misslap_dense_batch_meta), w, (size_t)B,
                             hipMemcpyDeviceToHost, st));
    return MISSLAP_OK;
}
void batch_meta_keep_stride(misslap_dense_batch_meta *meta, int32_t stride, int64_t B) {
    if (!meta) return;
    for (int64_t b = 0; b < B; ++b)
        reinterpret_cast<misslap_dense_batch_meta *>(reinterpret_cast<char *>(meta) + (size_t)b * (size_t)stride)
            ->struct_size = stride;
}

// The solve of an all-or-nothing call once every problem is accepted: the launch of `kernel` (k_dense_batch_solve /
// k_sparse_batch_solve), then the outputs, the meta records and the info.  The caller has set a's own fields, a.s.eps_b
// and a.s.p0 / p0_ld.
template <class Args>
int batch_solve_run(void (*kernel)(Args), Args a, hipStream_t st, DevScratch &tmp, const misslap_options &opt, int64_t B,
                    int Ns, int Ms, int32_t *sol, int64_t sol_ld, double *prices_out, int64_t prices_ld,
                    int32_t out_on_device, misslap_dense_batch_meta *meta, int32_t stride, misslap_dense_batch_info *info,
                    double t_start, double t_checked, double t_matched, double guard_ms) {
    int rc = 0;
    int32_t *d_sol = sol;
    double *d_prices = prices_out;
    misslap_dense_batch_meta *d_meta = nullptr;
    if ((rc = tmp.alloc(&d_meta, (size_t)B))) return rc;
    if (!out_on_device) {
        if ((rc = tmp.alloc(&d_sol, (size_t)B * (size_t)sol_ld))) return rc;
        if (prices_out && (rc = tmp.alloc(&d_prices, (size_t)B * (size_t)prices_ld))) return rc;
    }
    EventPair ev;
    if ((rc = ev.create())) return rc;
    misslap_dense_batch_info launch{};
    if ((rc = batch_solve_launch(kernel, a, a.s, opt, B, Ns, Ms, d_sol, sol_ld, d_prices, prices_ld, a.s.p0, a.s.p0_ld,
                                 d_meta, &launch, st, &ev)))
        return rc;
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * (size_t)B * (size_t)sol_ld, hipMemcpyDeviceToHost, st));
        if (prices_out)
            HIP_TRY(hipMemcpyAsync(prices_out, d_prices, sizeof(double) * (size_t)B * (size_t)prices_ld,
                                   hipMemcpyDeviceToHost, st));
    }
    if ((rc = batch_meta_copy_back(meta, stride, d_meta, B, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    tmp.drained = true;
    batch_meta_keep_stride(meta, stride, B);
    if (info) {
        double ms = 0;
        if ((rc = ev.elapsed(&ms))) return rc;
        *info = launch;
        info->check_ms = t_checked - t_start - guard_ms;
        info->matching_ms = guard_ms + (t_matched - t_checked);
        info->solve_ms = ms;
        info->wall_ms = now_ms() - t_start;
    }
    return MISSLAP_OK;
}
}  // namespace
