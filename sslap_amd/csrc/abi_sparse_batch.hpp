// abi_sparse_batch.hpp -- C ABI: many small sparse (loc / val) problems in one call, one workgroup per problem
// (misslap_solve_sparse_batch; the kernels are in kernels_sparse_batch.hpp, the shared host helpers in
// abi_batch_common.hpp).
// (part of the single translation unit misslap.hip; included in the order given there, after abi_dense_batch.hpp)
#pragma once

namespace {
// The feasibility guard of from_sparse for one problem (auction_.pyx:608-612 on the true graph n_true x m_true):
// misslap_hopcroft_karp's argument checks in its order, then the matching.  Returns false and the text of the first
// failure; the matcher never sees an index outside the graph.
bool sparse_problem_guard(const int32_t *loc, int64_t nnz, int n_true, int m_true, char *buf, size_t len) {
    if (n_true < 0 || m_true < 0) {
        snprintf(buf, len, "bad argument");
        return false;
    }
    for (int64_t k = 0; k < nnz; ++k) {
        const int32_t i = loc[2 * k], j = loc[2 * k + 1];
        if (i < 0 || i >= n_true || j < 0 || j >= m_true) {
            snprintf(buf, len, "loc entry %lld = (%d, %d) outside %d x %d", (long long)k, i, j, n_true, m_true);
            return false;
        }
        if (k && i < loc[2 * (k - 1)]) {
            snprintf(buf, len, "loc rows must be sorted in ascending order");
            return false;
        }
    }
    // Indices far beyond the entry count (a malformed problem: it has empty rows) are ranked first, so that the matcher's
    // arrays stay O(nnz).  Rows and columns without an entry take no part in a matching: the cardinality is the same.
    std::vector<int32_t> ranked;
    int nr = n_true, mr = m_true;
    if (n_true > nnz || m_true > nnz) {
        std::vector<int32_t> rows((size_t)nnz), cols((size_t)nnz);
        for (int64_t k = 0; k < nnz; ++k) {
            rows[(size_t)k] = loc[2 * k];
            cols[(size_t)k] = loc[2 * k + 1];
        }
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        ranked.resize(2 * (size_t)nnz);
        for (int64_t k = 0; k < nnz; ++k) {
            ranked[2 * (size_t)k] = (int32_t)(std::lower_bound(rows.begin(), rows.end(), loc[2 * k]) - rows.begin());
            ranked[2 * (size_t)k + 1] = (int32_t)(std::lower_bound(cols.begin(), cols.end(), loc[2 * k + 1]) - cols.begin());
        }
        nr = (int)rows.size();
        mr = (int)cols.size();
        loc = ranked.data();
    }
    HopcroftKarp hk(loc, nnz, nr, mr);
    const int card = hk.solve();
    if (card < n_true) {
        snprintf(buf, len, "Matrix is infeasible (Maximum matching possible only involves %d out of %d rows.)", card, n_true);
        return false;
    }
    return true;
}
// B and the host offsets of a sparse batch; *zmax: the largest problem's entries (at least 1)
int sparse_batch_offsets(int64_t B, const int64_t *offsets, int64_t *zmax) {
    if (B < 1 || B > 0x7fffffff) return fail(MISSLAP_ERR_INVALID, "B = %lld: 1 .. 2^31 - 1 problems", (long long)B);
    if (offsets[0] != 0) return fail(MISSLAP_ERR_INVALID, "offsets[0] = %lld: must be 0", (long long)offsets[0]);
    *zmax = 1;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t z = offsets[b + 1] - offsets[b];
        if (z < 0) return fail(MISSLAP_ERR_INVALID, "offsets must be non-decreasing (offsets[%lld] > offsets[%lld])",
                               (long long)b, (long long)b + 1);
        if (z >= 0x7fffffff)
            return fail(MISSLAP_ERR_INVALID, "problem %lld: %lld entries; a problem takes fewer than 2^31 - 1", (long long)b,
                        (long long)z);
        *zmax = std::max(*zmax, z);
    }
    return MISSLAP_OK;
}
}  // namespace

MISSLAP_API int misslap_solve_sparse_batch(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                           const int64_t *sizes, const float *eps_start, const double *prices_in,
                                           int64_t prices_ld, int32_t cardinality_check, const misslap_options *opt_in,
                                           int32_t *sol, int64_t sol_ld, double *prices_out, int64_t prices_out_ld,
                                           int32_t out_on_device, misslap_dense_batch_meta *meta,
                                           misslap_dense_batch_info *info) {
    const double t_start = now_ms();
    misslap_options opt;
    int rc = batch_options(opt_in, &opt, "misslap_solve_sparse_batch",
                           "device, maximize, eps_start, max_iter, input_on_device and input_stream");
    if (rc) return rc;
    if (!loc || !val || !offsets || !sol) return fail(MISSLAP_ERR_INVALID, "null loc / val / offsets / sol");
    int64_t zmax = 1;
    if ((rc = sparse_batch_offsets(B, offsets, &zmax))) return rc;
    if (sol_ld < 1 || (prices_out && prices_out_ld < 1) || (prices_in && prices_ld < 1))
        return fail(MISSLAP_ERR_INVALID, "sol_ld / prices_out_ld / prices_ld must be >= 1");
    int32_t stride = 0;
    if ((rc = batch_meta_stride(meta, &stride))) return rc;
    hipStream_t st = nullptr;
    if ((rc = batch_device(opt, &st))) return rc;

    const size_t nnz = (size_t)offsets[B];
    DevScratch tmp;
    const int32_t *d_loc = loc;
    const double *d_val = val, *d_p0 = prices_in;
    if (!opt.input_on_device &&
        ((rc = upload(tmp, &d_loc, loc, 2 * nnz, st)) || (rc = upload(tmp, &d_val, val, nnz, st)) ||
         (prices_in && (rc = upload(tmp, &d_p0, prices_in, (size_t)B * (size_t)prices_ld, st)))))
        return rc;
    const long long *d_off = nullptr;
    int *d_rs = nullptr;
    const float *d_eps = nullptr;
    SparseBatchCheck *d_chk = nullptr;
    if ((rc = upload(tmp, &d_off, offsets, (size_t)B + 1, st)) || (rc = tmp.alloc(&d_rs, nnz + (size_t)B)) ||
        (rc = tmp.alloc(&d_chk, (size_t)B)) || (eps_start && (rc = upload(tmp, &d_eps, eps_start, (size_t)B, st))))
        return rc;

    // ---- check pass: every problem before any is solved
    SparseCheckArgs<SparsePacked> k{};
    k.w = SparsePacked{d_loc, d_val};
    k.offsets = d_off;
    k.p0 = d_p0;
    k.p0_ld = prices_ld;
    k.row_start = d_rs;
    k.out = d_chk;
    hipLaunchKernelGGL((k_sparse_batch_check<SparsePacked, false>), dim3((unsigned)B), dim3(256), 0, st, k);
    HIP_TRY(hipGetLastError());
    // The matching guard on the device, behind the check pass and read back with it, for every problem whose graph the
    // check pass finds clean (rows ascending from 0 without a gap, no negative index) and within the cap: card[b] >= 0.
    // The carve is sized before the maxima are known: a clean graph has at most as many rows as entries.  Small batches
    // keep the host guard for every problem (card[b] = -1; sparse_guard_on_device).
    const bool device_guard = cardinality_check && sparse_guard_on_device(B);
    std::vector<int> card((size_t)B, -1);
    EventPair gev;
    if (device_guard) {
        int *d_card = nullptr;
        if ((rc = tmp.alloc(&d_card, (size_t)B))) return rc;
        MatchBatchArgs g{};
        g.loc = d_loc;
        g.offsets = d_off;
        g.schk = d_chk;
        g.Ns = (int)std::min<int64_t>(zmax, kSparseBatchMaxDim);
        g.Ms = kSparseBatchMaxDim;
        g.size = d_card;
        if ((rc = gev.create())) return rc;
        HIP_TRY(hipEventRecord(gev.e[0], st));
        hipLaunchKernelGGL(k_matching_batch<MatchSrc::Loc>, dim3((unsigned)B), dim3(kMatchBatchThreads),
                           matching_batch_lds_bytes(g.Ns, g.Ms, false), st, g);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(gev.e[1], st));
        HIP_TRY(hipMemcpyAsync(card.data(), d_card, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, st));
    }
    std::vector<SparseBatchCheck> chk((size_t)B);
    HIP_TRY(hipMemcpyAsync(chk.data(), d_chk, sizeof(SparseBatchCheck) * (size_t)B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double guard_ms = 0;
    if (device_guard && (rc = gev.elapsed(&guard_ms))) return rc;
    const double t_checked = now_ms();

    // the checks of from_sparse ahead of its guard (:604-605)
    auto pre_guard_error = [&](int64_t b, char *buf, size_t len) -> bool {
        const int64_t z = offsets[b + 1] - offsets[b];
        const int64_t N = sizes ? sizes[2 * b + 1] : (int64_t)chk[(size_t)b].max_row;  // sic, :592 / :594
        if (z == 0)
            snprintf(buf, len, "no entries");
        else if (z < N)
            snprintf(buf, len, "Matrix is infeasible - Fewer than %lld valid values provided for %lld rows.", (long long)N,
                     (long long)N);
        else
            return false;
        return true;
    };
    // the guard on the true graph: the device's cardinality where it has one, else per problem on up to 16 host threads
    // (device input: only those problems' loc slices are copied back)
    std::vector<std::string> guard_err;
    if (cardinality_check) {
        guard_err.assign((size_t)B, std::string());
        std::vector<int64_t> on_host;
        for (int64_t b = 0; b < B; ++b) {
            char buf[256];
            if (pre_guard_error(b, buf, sizeof(buf))) continue;
            const int card_b = card[(size_t)b];
            if (card_b < 0) {
                on_host.push_back(b);
                continue;
            }
            const int n_true = chk[(size_t)b].max_row + 1;
            if (card_b < n_true) {
                snprintf(buf, sizeof(buf), "Matrix is infeasible (Maximum matching possible only involves %d out of %d rows.)",
                         card_b, n_true);
                guard_err[(size_t)b] = buf;
            }
        }
        // Device input: the host copy the host guard reads.  Without the device guard that is the whole of loc in one
        // copy, as before; with it, only the host-guarded problems' entries, one copy per run of problems whose entries
        // are adjacent in loc.  host_at[t]: where problem on_host[t] starts in host_copy.
        std::vector<int32_t> host_copy;
        std::vector<int64_t> host_at;
        if (opt.input_on_device && !on_host.empty()) {
            if (!device_guard) {
                host_copy.resize(2 * nnz);
                HIP_TRY(hipMemcpy(host_copy.data(), loc, sizeof(int32_t) * 2 * nnz, hipMemcpyDeviceToHost));
                for (int64_t b : on_host) host_at.push_back(offsets[b]);
            } else {
                int64_t total = 0;
                for (int64_t b : on_host) {
                    host_at.push_back(total);
                    total += offsets[b + 1] - offsets[b];
                }
                host_copy.resize(2 * (size_t)total);
                for (size_t t = 0; t < on_host.size();) {
                    size_t u = t + 1;  // the run on_host[t .. u)
                    while (u < on_host.size() && offsets[on_host[u]] == offsets[on_host[u - 1] + 1]) ++u;
                    const int64_t first = offsets[on_host[t]], last = offsets[on_host[u - 1] + 1];
                    HIP_TRY(hipMemcpyAsync(host_copy.data() + 2 * host_at[t], loc + 2 * first,
                                           sizeof(int32_t) * 2 * (size_t)(last - first), hipMemcpyDeviceToHost, st));
                    t = u;
                }
                HIP_TRY(hipStreamSynchronize(st));
            }
        }
        rc = run_host_guards((int64_t)on_host.size(), [&](int64_t t) {
            char buf[256];
            const int64_t b = on_host[(size_t)t];
            const SparseBatchCheck &c = chk[(size_t)b];
            const int32_t *H = opt.input_on_device ? host_copy.data() + 2 * host_at[(size_t)t] : loc + 2 * offsets[b];
            // n_true = max row + 1, m_true = max column + 1 (int arithmetic of the front-end's int())
            if (!sparse_problem_guard(H, offsets[b + 1] - offsets[b], (int)((int64_t)c.max_row + 1),
                                      (int)((int64_t)c.max_col + 1), buf, sizeof(buf)))
                guard_err[(size_t)b] = buf;
        });
        if (rc) return rc;
    }
    const double t_matched = now_ms();
    int Ns = 1, Ms = 1;
    for (int64_t b = 0; b < B; ++b) {
        char buf[256];
        const SparseBatchCheck &c = chk[(size_t)b];
        if (pre_guard_error(b, buf, sizeof(buf))) return fail(MISSLAP_ERR_INVALID, "problem %lld: %s", (long long)b, buf);
        if (cardinality_check && !guard_err[(size_t)b].empty())
            return fail(MISSLAP_ERR_INVALID, "problem %lld: %s", (long long)b, guard_err[(size_t)b].c_str());
        // AuctionSolver.__init__ (build_from_device_coo's checks and texts, in its order)
        const char *bad = nullptr;
        if (c.last_row < 0) bad = "negative row index";
        else if (c.err & kErrColNegative) bad = "loc holds a negative row or column index";
        else if (c.err & kErrRowsUnsorted) bad = "loc rows must be sorted in ascending order (auction_.pyx:33-48 contract)";
        else if (c.err & kErrRowGap) bad = "every row 0..N-1 must have at least one entry (auction_.pyx:33-48 contract)";
        else if (c.err & kErrNonFinite) bad = "val holds a NaN or an infinity";
        else if (c.max_col >= 0x7ffffffe) bad = "column index too large (max + 1 must fit an int32)";
        if (bad) return fail(MISSLAP_ERR_INVALID, "problem %lld: %s", (long long)b, bad);
        const int n = c.last_row + 1, m = c.max_col + 1;
        if (n > kSparseBatchMaxDim || m > kSparseBatchMaxDim)
            return fail(MISSLAP_ERR_INVALID, "problem %lld: %d x %d exceeds MISSLAP_SPARSE_BATCH_MAX_DIM (%d); solve it with "
                        "from_sparse / solve_batch", (long long)b, n, m, kSparseBatchMaxDim);
        if (prices_in) {  // (the checks of AuctionSolver.resolve)
            if (m > prices_ld)
                return fail(MISSLAP_ERR_INVALID, "problem %lld: prices hold %lld columns, the problem has %d", (long long)b,
                            (long long)prices_ld, m);
            if ((rc = reject_bad_prices(b, c.bad_price))) return rc;
        }
        if (n > sol_ld || (prices_out && m > prices_out_ld))
            return fail(MISSLAP_ERR_INVALID, "problem %lld: %d x %d does not fit sol_ld = %lld / prices_out_ld = %lld",
                        (long long)b, n, m, (long long)sol_ld, (long long)prices_out_ld);
        Ns = std::max(Ns, n);
        Ms = std::max(Ms, m);
    }

    // ---- the solve: one launch, one workgroup per problem
    SparseBatchArgs<SparsePacked> a{};
    a.s.eps_b = d_eps;
    a.s.p0 = d_p0;
    a.s.p0_ld = prices_ld;
    a.w = SparsePacked{d_loc, d_val};
    a.offsets = d_off;
    a.row_start = d_rs;
    a.chk = d_chk;
    return batch_solve_run(k_sparse_batch_solve, a, st, tmp, opt, B, Ns, Ms, sol, sol_ld, prices_out, prices_out_ld,
                           out_on_device, meta, stride, info, t_start, t_checked, t_matched, guard_ms);
}
