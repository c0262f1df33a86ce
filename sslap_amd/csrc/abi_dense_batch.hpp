// abi_dense_batch.hpp -- C ABI: many small dense problems in one call, one workgroup per problem
// (misslap_solve_dense_batch; the kernels are in kernels_dense_batch.hpp, the shared host helpers in abi_batch_common.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_batch_stream.hpp)
#pragma once

namespace {
// "v >= 0" of _from_matrix (auction_.pyx:549) on the host, by bit pattern (the library is built with -fno-honor-nans)
inline bool dense_entry_valid_host(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b <= 0x7ff0000000000000ull || b == 0x8000000000000000ull;
}

template <class T>
inline bool dense_entry_valid_host(T v) {  // float, F16, Bf16: by bit pattern in the element's own type (device_common.hpp)
    return dense_entry_valid(v);
}

// The entry rule a call's options ask for: true for MISSLAP_DENSE_ENTRIES_FINITE, and opt->mat_dtype is left as the
// element type alone (normalise_options has checked the word), which is what every later reader of it expects.
inline bool dense_take_entries_finite(misslap_options *opt) {
    const bool finite = (opt->mat_dtype & MISSLAP_DENSE_ENTRIES_FINITE) != 0;
    opt->mat_dtype &= ~(int32_t)MISSLAP_DENSE_ENTRIES_FINITE;
    return finite;
}

// f(T{}) with T the element type mat_dtype names (normalise_options has checked the range)
template <class F>
auto dense_dtype_dispatch(int32_t mat_dtype, F &&f) {
    switch (mat_dtype) {
    case MISSLAP_DTYPE_F32: return f(float{});
    case MISSLAP_DTYPE_F16: return f(F16{});
    case MISSLAP_DTYPE_BF16: return f(Bf16{});
    default: return f(double{});
    }
}
inline size_t dense_dtype_bytes(int32_t mat_dtype) {
    return dense_dtype_dispatch(mat_dtype, [](auto t) { return sizeof(t); });
}

// a host stack of `cells` elements of mat_dtype into a new scratch buffer on the device (*d), copied on st
int upload_stack(DevScratch &tmp, const void **d, const void *h, size_t cells, int32_t mat_dtype, hipStream_t st) {
    const char *p = nullptr;
    const int rc = upload(tmp, &p, h, cells * dense_dtype_bytes(mat_dtype), st);
    *d = p;
    return rc;
}

// maximum-matching cardinality of one dense slice (row stride M): the guard of _from_matrix (auction_.pyx:562-566)
template <class T>
int dense_slice_matching(const T *A, int64_t M, int n, int m) {
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

// the size of a dense stack: 1 .. 2^31 - 1 problems within the cap
int dense_batch_dims(int64_t B, int64_t N, int64_t M) {
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 problems", (long long)B);
    if (N < 1 || M < 1 || N > kDenseBatchMaxDim || M > kDenseBatchMaxDim)
        return fail(MISSLAP_ERR_INVALID,
                    "a %lld x %lld problem: the dense batch takes at most %d x %d (MISSLAP_DENSE_BATCH_MAX_DIM); solve larger "
                    "problems with misslap_create_dense / misslap_solve_batch",
                    (long long)N, (long long)M, kDenseBatchMaxDim, kDenseBatchMaxDim);
    return MISSLAP_OK;
}

// The strides of a strided stack, in elements: element (b, i, j) of the view lies at mat[b * sB + i * sN + j * sM].
// None may be negative, and the offset of the view's last element must fit 62 bits (it is formed in 64 bits on the
// device, and scaled by the element size); made before any device is touched.  `who`: the entry point.
int dense_strides_check(int64_t B, int64_t N, int64_t M, int64_t sB, int64_t sN, int64_t sM, const char *who) {
    if (sB < 0 || sN < 0 || sM < 0)
        return fail(MISSLAP_ERR_INVALID, "%s: strides (%lld, %lld, %lld): a stride must be >= 0 (elements)", who,
                    (long long)sB, (long long)sN, (long long)sM);
    const unsigned __int128 extent = (unsigned __int128)(B - 1) * (unsigned __int128)sB +
                                     (unsigned __int128)(N - 1) * (unsigned __int128)sN +
                                     (unsigned __int128)(M - 1) * (unsigned __int128)sM;
    if (extent >> 62)
        return fail(MISSLAP_ERR_INVALID,
                    "%s: strides (%lld, %lld, %lld) of a %lld x %lld x %lld stack: the last element's offset does not fit "
                    "62 bits", who, (long long)sB, (long long)sN, (long long)sM, (long long)B, (long long)N, (long long)M);
    return MISSLAP_OK;
}
// the strides of the contiguous stack: such a call takes the contiguous kernels
inline bool dense_strides_compact(int64_t N, int64_t M, int64_t sB, int64_t sN, int64_t sM) {
    return sM == 1 && sN == M && sB == N * M;
}
// Rounds of at least this many bidders of a strided solve bid one lane per person where the stack's rows run along the
// unit stride (DenseBatchRows::bid_lanes; DESIGN.md 4.19 has the measurement behind the value).
// MISSLAP_STRIDED_LANE_MIN_K overrides it (tools/dense_strided.py: 0 = every round, a value above the cap = none).
constexpr int kStridedLaneMinK = 64;
inline DenseStrides dense_strides_arg(int64_t sB, int64_t sN, int64_t sM) {
    int min_K = kStridedLaneMinK;
    if (const char *e = std::getenv("MISSLAP_STRIDED_LANE_MIN_K")) min_K = std::atoi(e);  // (read per call)
    return DenseStrides{(long long)sB, (long long)sN, (long long)sM, min_K};
}

// The layout of a call's stack: strides null (the contiguous entry points) or {sB, sN, sM} of a strided one (`who`).
// *str becomes null for DenseContig, else `store`, filled: a view.  A strided stack lies on the device (a host
// stack is uploaded whole, and is compact); all of this is checked before any device is touched.
// finite: the call's kernels are those of DenseView<true>, so *str is never null: a contiguous stack (of either kind
// of entry point) gets its natural strides (N * M, M, 1).
int dense_stack_layout(const char *who, const misslap_options &opt, int64_t B, int64_t N, int64_t M,
                       const int64_t *strides, DenseStrides *store, const DenseStrides **str, bool finite = false) {
    *str = nullptr;
    if (!strides) {
        if (finite) {
            *store = dense_strides_arg(N * M, M, 1);
            *str = store;
        }
        return MISSLAP_OK;
    }
    const int rc = dense_strides_check(B, N, M, strides[0], strides[1], strides[2], who);
    if (rc) return rc;
    if (!opt.input_on_device)
        return fail(MISSLAP_ERR_INVALID, "%s: a strided stack is a device array: set input_on_device", who);
    if (!finite && dense_strides_compact(N, M, strides[0], strides[1], strides[2])) return MISSLAP_OK;
    *store = dense_strides_arg(strides[0], strides[1], strides[2]);
    *str = store;
    return MISSLAP_OK;
}

// body(T{}, lay) with T the element type mat_dtype names and lay the layout dense_stack_layout chose: DenseContig
// (str null), DenseView<false>{*str} or, finite, DenseView<true>{*str}.  Every launch of a dense kernel on a call's
// stack comes through here, and nothing else knows how many layouts there are.
template <class F>
auto dense_dispatch(int32_t mat_dtype, const DenseStrides *str, bool finite, F &&body) {
    return dense_dtype_dispatch(mat_dtype, [&](auto t) {
        if (finite) return body(t, DenseView<true>{*str});
        if (str) return body(t, DenseView<false>{*str});
        return body(t, DenseContig{});
    });
}

// The matcher on a dense stack of element type T and layout lay (g: everything but the strides; lds: its carve):
// the one place that maps a layout to the matcher's source.
template <class T, class Lay>
void dense_guard_launch(hipStream_t st, int64_t B, MatchBatchArgs g, const Lay &lay, size_t lds) {
    constexpr MatchSrc kSrc = !Lay::kView    ? MatchSrc::Dense
                              : Lay::kFinite ? MatchSrc::DenseStridedFinite
                                             : MatchSrc::DenseStrided;
    if constexpr (Lay::kView) {
        g.sB = lay.str.sB;
        g.sN = lay.str.sN;
        g.sM = lay.str.sM;
    }
    hipLaunchKernelGGL((k_matching_batch<kSrc, T>), dim3((unsigned)B), dim3(kMatchBatchThreads), lds, st, g);
}

// a host shapes array (or null): every problem within the stack
int dense_batch_host_shapes(const int32_t *shapes, int64_t B, int64_t N, int64_t M) {
    if (shapes)
        for (int64_t b = 0; b < B; ++b)
            if (shapes[2 * b] < 1 || shapes[2 * b] > N || shapes[2 * b + 1] < 1 || shapes[2 * b + 1] > M)
                return fail(MISSLAP_ERR_INVALID, "problem %lld: shape (%d, %d) outside 1 .. %lld x 1 .. %lld", (long long)b,
                            shapes[2 * b], shapes[2 * b + 1], (long long)N, (long long)M);
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int misslap_solve_dense_batch(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                                          const float *eps_start, const double *prices_in, int32_t cardinality_check,
                                          const misslap_options *opt_in, int32_t *sol, double *prices_out,
                                          int32_t out_on_device, misslap_dense_batch_meta *meta,
                                          misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_dense_batch",
                           "device, maximize, eps_start, max_iter, mat_dtype, input_on_device and input_stream", true);
    if (rc) return rc;
    if (dense_take_entries_finite(&opt))  // (this call has a host guard and kernels of its own: not taught the mode)
        return fail(MISSLAP_ERR_INVALID,
                    "misslap_solve_dense_batch does not take MISSLAP_DENSE_ENTRIES_FINITE in mat_dtype: call "
                    "misslap_solve_dense_batch_status");
    if (!mat || !sol) return fail(MISSLAP_ERR_INVALID, "null mat / sol");
    if ((rc = dense_batch_dims(B, N, M))) return rc;
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    if ((rc = dense_batch_host_shapes(shapes, B, N, M))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;

    const size_t cells = (size_t)B * (size_t)N * (size_t)M, pcells = (size_t)B * (size_t)M;
    DevScratch tmp;
    const void *d_mat = mat;  // elements of opt.mat_dtype, whatever the parameter's declared type
    const double *d_p0 = prices_in;
    if (!opt.input_on_device && ((rc = upload_stack(tmp, &d_mat, mat, cells, opt.mat_dtype, st)) ||
                                 (prices_in && (rc = upload(tmp, &d_p0, prices_in, pcells, st)))))
        return rc;
    const int *d_shapes = nullptr;
    const float *d_eps = nullptr;
    DenseBatchCheck *d_chk = nullptr;
    if ((rc = tmp.alloc(&d_chk, (size_t)B)) || (shapes && (rc = upload(tmp, &d_shapes, shapes, (size_t)B * 2, st))) ||
        (eps_start && (rc = upload(tmp, &d_eps, eps_start, (size_t)B, st))))
        return rc;

    // ---- validation: every problem before any is solved
    DenseCheckArgs<DenseContig> k{};  // (shapes_out null: the shapes are checked above)
    k.mat = d_mat;
    k.N = N;
    k.M = M;
    k.shapes = d_shapes;
    k.p0 = d_p0;
    k.out = d_chk;
    dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        hipLaunchKernelGGL((k_dense_batch_check<decltype(t), DenseContig, false>), dim3((unsigned)B), dim3(256), 0, st, k);
    });
    HIP_TRY(hipGetLastError());
    // the matching guard of every problem on the device, behind the validation pass and read back with it
    const bool device_guard = cardinality_check && dense_guard_on_device(B);
    std::vector<int> card;
    EventPair gev;
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
        dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
            dense_guard_launch<decltype(t)>(st, B, g, DenseContig{}, matching_batch_lds_bytes(N, M, true));
        });
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
        std::vector<unsigned char> host_copy;
        const void *H = mat;
        if (opt.input_on_device) {
            host_copy.resize(cells * dense_dtype_bytes(opt.mat_dtype));
            HIP_TRY(hipMemcpy(host_copy.data(), mat, host_copy.size(), hipMemcpyDeviceToHost));
            H = host_copy.data();
        }
        card.assign((size_t)B, -1);
        rc = run_host_guards(B, [&](int64_t b) {
            char buf[256];
            if (first_error(b, buf, sizeof(buf))) return;
            int n, m;
            dims(b, n, m);
            card[(size_t)b] = dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
                return dense_slice_matching(static_cast<const decltype(t) *>(H) + (size_t)b * (size_t)N * (size_t)M, M, n, m);
            });
        });
        if (rc) return rc;
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
        if ((rc = reject_bad_prices(b, chk[(size_t)b].bad_price))) return rc;  // (the checks of AuctionSolver.resolve)
    }

    // ---- the solve: one launch, one workgroup per problem
    DenseBatchArgs a{};
    a.s.eps_b = d_eps;
    a.s.p0 = d_p0;
    a.s.p0_ld = M;
    a.mat = d_mat;
    a.N = N;
    a.M = M;
    a.shapes = d_shapes;
    a.chk = d_chk;
    return dense_dtype_dispatch(opt.mat_dtype, [&](auto t) {
        return batch_solve_run(k_dense_batch_solve<decltype(t)>, a, st, tmp, opt, B, (int)N, (int)M, sol, N, prices_out, M,
                               out_on_device, meta, stride, info, t_start, t_checked, t_matched, guard_ms);
    });
}
