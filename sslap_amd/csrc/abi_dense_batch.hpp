// abi_dense_batch.hpp -- C ABI: many small dense problems in one call, one workgroup per problem
// (misslap_solve_dense_batch; the kernels are in kernels_dense_batch.hpp).
// (part of the single translation unit misslap.hip; included in the order given there)
#pragma once

namespace {
// the calling thread's stream on a device (created on first use, kept for the life of the thread's process)
int dense_batch_stream(int device, hipStream_t *out) {
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

// "v >= 0" of _from_matrix (auction_.pyx:549) on the host, by bit pattern (the library is built with -fno-honor-nans)
inline bool dense_entry_valid_host(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b <= 0x7ff0000000000000ull || b == 0x8000000000000000ull;
}

// maximum-matching cardinality of one dense slice (row stride M): the guard of _from_matrix (auction_.pyx:562-566)
int dense_slice_matching(const double *A, int64_t M, int n, int m) {
    std::vector<int32_t> loc;
    loc.reserve((size_t)n * 2 * 8);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j)
            if (dense_entry_valid_host(A[(size_t)i * (size_t)M + j])) {
                loc.push_back(i);
                loc.push_back(j);
            }
    HopcroftKarp hk(loc.data(), (int64_t)(loc.size() / 2), n, m);
    return hk.solve();
}

// Whether the matching guard of a batch runs on the device (k_matching_batch behind the check pass) or on the host
// threads.  One graph on one CU is slower than the host matcher (a DFS step waits on L2), so the device wins only once
// the batch spreads over the GPU: measured it lost at B = 1 (dense and sparse) and at sparse 64 x 2048,
// and won at dense B >= 64 and sparse B >= 256.
inline bool dense_guard_on_device(int64_t B) { return B >= 64; }
inline bool sparse_guard_on_device(int64_t B) { return B >= 256; }

// the two events around a guard launch
struct GuardEvents {
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
    ~GuardEvents() {
        if (e[0]) (void)hipEventDestroy(e[0]);
        if (e[1]) (void)hipEventDestroy(e[1]);
    }
};
}  // namespace

MISSLAP_API int misslap_solve_dense_batch(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                                          const float *eps_start, const double *prices_in, int32_t cardinality_check,
                                          const misslap_options *opt_in, int32_t *sol, double *prices_out,
                                          int32_t out_on_device, misslap_dense_batch_meta *meta,
                                          misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int abi = 0;
    int rc = normalise_options(opt_in, &opt, &abi);
    if (rc) return rc;
    if (opt.tail_threshold > 0 || opt.force_f64_values || opt.profile || opt.shard_world > 1 || opt.rounds_per_sync ||
        opt.tiled_min_K || opt.tiled_shape || opt.tiled_force || opt.shard_min_K || opt.cand_mode || opt.nnz_limit ||
        opt.cand_build_max_K || opt.cand_refresh_min)
        return fail(MISSLAP_ERR_INVALID, "misslap_solve_dense_batch takes device, maximize, eps_start, max_iter, "
                                         "input_on_device and input_stream only: every other option must be 0");
    if (!mat || !sol) return fail(MISSLAP_ERR_INVALID, "null mat / sol");
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 problems", (long long)B);
    if (N < 1 || M < 1 || N > kDenseBatchMaxDim || M > kDenseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID,
                    "a %lld x %lld problem: the dense batch takes at most %d x %d (MISSLAP_DENSE_BATCH_MAX_DIM); solve larger "
                    "problems with misslap_create_dense / misslap_solve_batch",
                    (long long)N, (long long)M, kDenseBatchMaxDim, kDenseBatchMaxDim);
    int32_t stride = 0;
    if (meta) {
        stride = meta[0].struct_size;
        if (stride < (int32_t)offsetof(misslap_dense_batch_meta, its) || stride > 4096)
            return fail(MISSLAP_ERR_INVALID, "misslap_dense_batch_meta.struct_size = %d: set it to sizeof (%d) in meta[0]",
                        stride, (int)sizeof(misslap_dense_batch_meta));
    }
    if (shapes)
        for (int64_t b = 0; b < B; ++b)
            if (shapes[2 * b] < 1 || shapes[2 * b] > N || shapes[2 * b + 1] < 1 || shapes[2 * b + 1] > M)
                return fail(MISSLAP_ERR_INVALID, "problem %lld: shape (%d, %d) outside 1 .. %lld x 1 .. %lld", (long long)b,
                            shapes[2 * b], shapes[2 * b + 1], (long long)N, (long long)M);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MISSLAP_ERR_NO_DEVICE, "no HIP device available: libmisslap has no CPU fallback");
    if (opt.device < 0 || opt.device >= ndev) return fail(MISSLAP_ERR_INVALID, "device %d out of range", opt.device);
    HIP_TRY(hipSetDevice(opt.device));
    hipStream_t st = nullptr;
    if ((rc = dense_batch_stream(opt.device, &st))) return rc;
    if ((rc = sync_device_inputs(&opt, st))) return rc;

    const size_t cells = (size_t)B * (size_t)N * (size_t)M, pcells = (size_t)B * (size_t)M;
    DevScratch tmp;
    const double *d_mat = mat, *d_p0 = prices_in;
    if (!opt.input_on_device) {
        double *p = nullptr;
        if ((rc = tmp.alloc(&p, cells))) return rc;
        HIP_TRY(hipMemcpyAsync(p, mat, sizeof(double) * cells, hipMemcpyHostToDevice, st));
        d_mat = p;
        if (prices_in) {
            double *q = nullptr;
            if ((rc = tmp.alloc(&q, pcells))) return rc;
            HIP_TRY(hipMemcpyAsync(q, prices_in, sizeof(double) * pcells, hipMemcpyHostToDevice, st));
            d_p0 = q;
        }
    }
    int *d_shapes = nullptr;
    float *d_eps = nullptr;
    DenseBatchCheck *d_chk = nullptr;
    misslap_dense_batch_meta *d_meta = nullptr;
    if ((rc = tmp.alloc(&d_chk, (size_t)B)) || (rc = tmp.alloc(&d_meta, (size_t)B))) return rc;
    if (shapes) {
        if ((rc = tmp.alloc(&d_shapes, (size_t)B * 2))) return rc;
        HIP_TRY(hipMemcpyAsync(d_shapes, shapes, sizeof(int32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, st));
    }
    if (eps_start) {
        if ((rc = tmp.alloc(&d_eps, (size_t)B))) return rc;
        HIP_TRY(hipMemcpyAsync(d_eps, eps_start, sizeof(float) * (size_t)B, hipMemcpyHostToDevice, st));
    }

    // ---- validation: every problem before any is solved
    hipLaunchKernelGGL(k_dense_batch_check, dim3((unsigned)B), dim3(256), 0, st, d_mat, (long long)N, (long long)M,
                       d_shapes, d_p0, d_chk);
    HIP_TRY(hipGetLastError());
    // the matching guard of every problem on the device, behind the validation pass and read back with it
    const bool device_guard = cardinality_check && dense_guard_on_device(B);
    std::vector<int> card;
    GuardEvents gev;
    if (device_guard) {
        int *d_card = nullptr;
        if ((rc = tmp.alloc(&d_card, (size_t)B))) return rc;
        MatchBatchArgs g{};
        g.mat = d_mat;
        g.N = N;
        g.M = M;
        g.shapes = d_shapes;
        g.Ns = (int)N;
        g.Ms = (int)M;
        g.size = d_card;
        if ((rc = gev.create())) return rc;
        HIP_TRY(hipEventRecord(gev.e[0], st));
        hipLaunchKernelGGL(k_matching_batch<true>, dim3((unsigned)B), dim3(kMatchBatchThreads),
                           matching_batch_lds_bytes(N, M, true), st, g);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(gev.e[1], st));
        card.assign((size_t)B, -1);
        HIP_TRY(hipMemcpyAsync(card.data(), d_card, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    }
    std::vector<DenseBatchCheck> chk((size_t)B);
    HIP_TRY(hipMemcpyAsync(chk.data(), d_chk, sizeof(DenseBatchCheck) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double guard_ms = 0;
    if (device_guard && (rc = gev.elapsed(&guard_ms))) return rc;
    const double t_checked = now_ms();
    auto dims = [&](int64_t b, int &n, int &m) {
        n = shapes ? shapes[2 * b] : (int)N;
        m = shapes ? shapes[2 * b + 1] : (int)M;
    };
    // the checks of _from_matrix and AuctionSolver.__init__ in their order; the matching guard comes after them
    auto first_error = [&](int64_t b, char *buf, size_t len) -> bool {
        int n, m;
        dims(b, n, m);
        const DenseBatchCheck &c = chk[(size_t)b];
        if (c.nvalid < (unsigned long long)n)  // auction_.pyx:559-560
            snprintf(buf, len, "Matrix is infeasible - Fewer than %d valid values provided for %d rows.", n, n);
        else if (c.empty_row != 0x7fffffff)
            snprintf(buf, len, "every row must have at least one valid (>= 0) entry");
        else if (c.has_inf)
            snprintf(buf, len, "val holds a NaN or an infinity");
        else
            return false;
        return true;
    };
    if (cardinality_check && !device_guard) {
        // the host copy of the matrix the guard reads (device input: copied back once)
        std::vector<double> host_copy;
        const double *H = mat;
        if (opt.input_on_device) {
            host_copy.resize(cells);
            HIP_TRY(hipMemcpy(host_copy.data(), mat, sizeof(double) * cells, hipMemcpyDeviceToHost));
            H = host_copy.data();
        }
        card.assign((size_t)B, -1);
        std::atomic<int64_t> next{0};
        std::atomic<int> oom{0};
        auto work = [&]() {
            char buf[256];
            for (int64_t b; (b = next.fetch_add(1)) < B;) {
                if (first_error(b, buf, sizeof(buf))) continue;
                int n, m;
                dims(b, n, m);
                try {
                    card[(size_t)b] = dense_slice_matching(H + (size_t)b * (size_t)N * (size_t)M, M, n, m);
                } catch (const std::bad_alloc &) {
                    oom = 1;
                }
            }
        };
        const int nthr = (int)std::min<int64_t>(B, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
        std::vector<std::thread> pool;
        for (int t = 1; t < nthr; ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        if (oom) return fail(MISSLAP_ERR_HIP, "out of host memory in the matching guard");
    }
    const double t_matched = now_ms();
    for (int64_t b = 0; b < B; ++b) {
        char buf[256];
        int n, m;
        dims(b, n, m);
        if (first_error(b, buf, sizeof(buf))) return fail(MISSLAP_ERR_INVALID, "problem %lld: %s", (long long)b, buf);
        if (cardinality_check && card[(size_t)b] < n)  // :562-566
            return fail(MISSLAP_ERR_INVALID, "problem %lld: Matrix is infeasible (Maximum matching possible only involves %d "
                        "out of %d rows.)", (long long)b, card[(size_t)b], n);
        const int bad = chk[(size_t)b].bad_price;  // (the checks of AuctionSolver.resolve)
        if (bad & 1) return fail(MISSLAP_ERR_INVALID, "problem %lld: prices hold a NaN or an infinity", (long long)b);
        if (bad & 2)
            return fail(MISSLAP_ERR_INVALID, "problem %lld: prices must be >= 0 (with the sign bit clear: -0.0 is rejected)",
                        (long long)b);
    }

    // ---- the solve: one launch, one workgroup per problem
    int32_t *d_sol = sol;
    double *d_prices = prices_out;
    if (!out_on_device) {
        if ((rc = tmp.alloc(&d_sol, (size_t)B * (size_t)N))) return rc;
        if (prices_out && (rc = tmp.alloc(&d_prices, pcells))) return rc;
    }
    DenseBatchArgs a;
    a.mat = d_mat;
    a.N = N;
    a.M = M;
    a.shapes = d_shapes;
    a.eps_b = d_eps;
    a.eps_opt = opt.eps_start;
    a.p0 = d_p0;
    a.chk = d_chk;
    a.maximize = opt.maximize ? 1 : 0;
    a.max_iter = opt.max_iter;
    a.sol = d_sol;
    a.prices = d_prices;
    a.meta = d_meta;
    // a wavefront bids for one list position at a time: enough wavefronts for the first round's bidders, at most 16
    const int threads = N <= 256 ? 256 : (N <= 512 ? 512 : 1024);
    const size_t lds = dense_batch_lds_bytes(N, M);
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreate(&ev[0]));
    HIP_TRY(hipEventCreate(&ev[1]));
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() {
            (void)hipEventDestroy(e[0]);
            (void)hipEventDestroy(e[1]);
        }
    } ev_guard{ev};
    HIP_TRY(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_dense_batch_solve, dim3((unsigned)B), dim3(threads), lds, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], st));
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(sol, d_sol, sizeof(int32_t) * (size_t)B * (size_t)N, hipMemcpyDeviceToHost, st));
        if (prices_out)
            HIP_TRY(hipMemcpyAsync(prices_out, d_prices, sizeof(double) * pcells, hipMemcpyDeviceToHost, st));
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
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        info->threads = threads;
        info->lds_bytes = (int32_t)lds;
        info->check_ms = t_checked - t_start - guard_ms;
        info->matching_ms = guard_ms + (t_matched - t_checked);
        info->solve_ms = ms;
        info->wall_ms = now_ms() - t_start;
    }
    return MISSLAP_OK;
}
