// kernels_sparse_batch.hpp -- many small SPARSE problems, one workgroup per problem for its whole solve
// (misslap_solve_sparse_batch, include/misslap.h; the host side is abi_sparse_batch.hpp), and the same solve with a
// verdict per problem (misslap_solve_sparse_batch_status; abi_sparse_batch_status.hpp).
//
// The round loop is batch_solve (kernels_batch_solve.hpp); this file has the check pass and the sparse row source.
// What differs from the dense source is where a row comes from.  Problem b is the entries offsets[b] .. offsets[b + 1]
// of the caller's loc / val, in their STORED order -- the order the reference's AuctionSolver walks them (flat_j / val
// after cumulative_idxs, auction_.pyx:33-48, :202-233) -- and row i of it is the run row_start[i] .. row_start[i + 1]
// that the check pass found.  So:
//   BID      one wavefront per unassigned list position; lane l holds the row's stored indices l, l + 64, ... (rows of
//            any length), the tie key is the stored index: top2_wave_reduce keeps the reference's ">=" rule (the last
//            stored maximum wins, :351) and counts a repeated maximum -- a duplicate (i, j) entry included -- into the
//            second best as the sequential scan does (:353).  The object is col[start + g].
//   eCE      choice_cost is the value at the LAST stored entry of row i whose column is p2o[i] (the loop of :462-467
//            overwrites it on every match), then every stored entry is tested against it (:475-485).
//   get_obj  every stored entry whose column is p2o[i] is added, in row order and stored order (:508-521): a
//            duplicate of the chosen entry counts once per copy.
#pragma once

namespace misslap {

constexpr int kSparseBatchMaxDim = MISSLAP_SPARSE_BATCH_MAX_DIM;

// per problem, from the check pass ahead of the solve
struct SparseBatchCheck {
    unsigned long long absmax_bits;  // max |v| over the problem's values, as bits
    int max_row;    // max row index over every entry (the reference's N of :594 is this, without + 1)
    int max_col;    // max column index over every entry
    int last_row;   // row of the last stored entry (AuctionSolver's N - 1 with rows ascending, :209)
    int err;        // kErrColNegative / kErrRowsUnsorted / kErrRowGap / kErrNonFinite, as k_ingest_rows / _vals set them
    int bad_price;  // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
    int pad;
};

struct SparseBatchArgs {
    BatchSolveArgs s;             // Ns / Ms: the batch's largest n_b / n_cols
    const int *loc;               // [nnz][2]
    const double *val;            // [nnz]
    const long long *offsets;     // [B + 1]
    const int *row_start;         // [nnz + B]: problem b's row starts (local indices) at offsets[b] + b
    const SparseBatchCheck *chk;  // [B]
};

// Check pass, one workgroup per problem: the checks of AuctionSolver.__init__ (k_ingest_rows / k_ingest_vals with the
// same rules), the maxima of from_sparse (:594-595) and of the guard (n_true, m_true), C = max |v|, the starting prices,
// and the row starts.  A row start is written only where the rows seen so far are gap-free (r <= local index), so a
// malformed problem never writes outside its own nnz_b + 1 slots.
__global__ __launch_bounds__(256) void k_sparse_batch_check(const int *loc, const double *val, const long long *offsets,
                                                            const double *p0, long long p0_ld, int *row_start,
                                                            SparseBatchCheck *out) {
    const int b = blockIdx.x;
    const long long s = offsets[b], e = offsets[b + 1];
    const int nnz = (int)(e - s);  // (the host rejects problems of 2^31 - 1 entries or more)
    int *rs = row_start + s + b;
    __shared__ unsigned long long s_abs;
    __shared__ int s_err, s_maxr, s_maxc, s_badp;
    if (threadIdx.x == 0) {
        s_abs = 0ull;
        s_err = 0;
        s_maxr = INT_MIN;
        s_maxc = INT_MIN;
        s_badp = 0;
    }
    __syncthreads();
    const int last_row = nnz > 0 ? loc[2 * (e - 1)] : -1;
    int err = 0, mr = INT_MIN, mc = INT_MIN;
    unsigned long long am = 0ull;
    for (int k = threadIdx.x; k < nnz; k += blockDim.x) {
        const long long g = s + k;
        const int r = loc[2 * g], c = loc[2 * g + 1];
        mr = r > mr ? r : mr;
        mc = c > mc ? c : mc;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(val[g]) & 0x7fffffffffffffffull;
        if (bits >= 0x7ff0000000000000ull) err |= kErrNonFinite;
        am = bits > am ? bits : am;
        if (r < 0 || c < 0) {
            err |= kErrColNegative;
            continue;
        }
        const int rp = k ? loc[2 * (g - 1)] : -1;
        if (r < rp) err |= kErrRowsUnsorted;
        else if (r > rp) {
            if (r != rp + 1 || r > last_row) err |= kErrRowGap;
            else if (r <= k) rs[r] = k;  // (r > k implies a gap earlier in the problem)
        }
    }
    if (err) atomicOr(&s_err, err);
    if (mr != INT_MIN) atomicMax(&s_maxr, mr);
    if (mc != INT_MIN) atomicMax(&s_maxc, mc);
    if (am) atomicMax(&s_abs, am);
    __syncthreads();
    const int m = s_maxc + 1;  // n_cols (only meaningful without errors)
    if (p0 && s_err == 0 && m > 0)  // (the host rejects m > p0_ld)
        batch_check_prices(p0 + (size_t)b * (size_t)p0_ld, (long long)m < p0_ld ? m : (int)p0_ld, &s_badp);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (last_row >= 0 && last_row < nnz) rs[last_row + 1] = nnz;  // :47
        SparseBatchCheck c;
        c.absmax_bits = s_abs;
        c.max_row = s_maxr;
        c.max_col = s_maxc;
        c.last_row = last_row;
        c.err = s_err;
        c.bad_price = s_badp;
        c.pad = 0;
        out[b] = c;
    }
}

// The sparse row source of batch_solve: problem b's entries from global index s, row i at s + rs[i] .. s + rs[i + 1].
struct SparseBatchRows {
    const int *loc;
    const double *val;
    const long long *offsets;
    long long s;
    const int *rs;
    int maximize;

    // the row in stored order, lane l at stored indices l, l + 64, ...; the tie key is the stored index
    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        const long long g0 = s + rs[i];
        const int len = rs[i + 1] - rs[i];
        Top2 x;
        x.v = -__builtin_huge_val();
        x.w = -__builtin_huge_val();
        x.g = -1;
        double cb = 0.0;
        int cj = 0;
        for (int q = lane; q < len; q += kWave) {
            const int c = loc[2 * (g0 + q) + 1];
            const double v = val[g0 + q];
            const double cost = maximize ? v : v * -1.0;  // :236-237
            const double vi = cost - price[c];
            if (vi >= x.v) {  // :351 (the first entry is always taken: vi >= -inf for every non-NaN vi)
                x.w = x.v;
                x.v = vi;
                x.g = q;
                cb = cost;
                cj = c;
            } else if (vi > x.w) {
                x.w = vi;
            }
        }
        const Top2 r = top2_wave_reduce(x);
        const int gl = r.g & (kWave - 1);  // the lane that holds stored index r.g
        costbest = readlane_f64(cb, gl);
        obj = __builtin_amdgcn_readlane(cj, gl);
        return r;
    }

    // eCE_satisfied (auction_.pyx:443-485) for row i: choice_cost from the last stored entry of column j
    __device__ __forceinline__ bool ece_bad(int i, int j, const double *price, double tol, double eps) const {
        const int lane = lane_id();
        const long long g0 = s + rs[i];
        const int len = rs[i + 1] - rs[i];
        int last = -1;  // the last stored index of column j (:462-467)
        for (int q = lane; q < len; q += kWave)
            if (loc[2 * (g0 + q) + 1] == j) last = q;
        last = wave_max_i32(last);
        const double vj = val[g0 + last];
        const double choice_cost = maximize ? vj : vj * -1.0;
        const double LHS = choice_cost - price[j] + tol;  // :475
        bool bad = false;
        for (int q = lane; q < len; q += kWave) {
            const double v = val[g0 + q];
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[loc[2 * (g0 + q) + 1]]) - eps) bad = true;  // :482
        }
        return bad;
    }

    // get_obj (:489-523) over EVERY entry of the chosen column: a wavefront per row gathers the row's one matching value;
    // a row with several matches (duplicate entries) is marked (nsel[i] > 1) and re-walked by the summing lane.
    __device__ __forceinline__ void gather(const int *p2o, int n, double *selv, int *nsel) const {
        const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int i = wave; i < n; i += nw) {
            const int j = p2o[i];
            if (j < 0) continue;
            const long long g0 = s + rs[i];
            const int len = rs[i + 1] - rs[i];
            int cnt = 0, at = -1;
            for (int q = lane; q < len; q += kWave)
                if (loc[2 * (g0 + q) + 1] == j) {
                    ++cnt;
                    at = q;
                }
            for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
            at = wave_max_i32(at);
            if (lane == 0) {
                nsel[i] = cnt;
                selv[i] = val[g0 + at];
            }
        }
    }

    // a double sum in row order, within a row in stored order
    __device__ __forceinline__ double objective(const int *p2o, int n, const double *selv, const int *nsel) const {
        double obj = 0;
        for (int i = 0; i < n; ++i) {
            const int j = p2o[i];
            if (j == -1) continue;
            if (nsel[i] == 1) {
                const double v = maximize ? selv[i] : selv[i] * -1.0;
                if (maximize) obj += v;
                else obj -= v;
                continue;
            }
            const long long g0 = s + rs[i];
            const int len = rs[i + 1] - rs[i];
            for (int q = 0; q < len; ++q)
                if (loc[2 * (g0 + q) + 1] == j) {
                    const double v = maximize ? val[g0 + q] : val[g0 + q] * -1.0;
                    if (maximize) obj += v;
                    else obj -= v;
                }
        }
        return obj;
    }

    __device__ __forceinline__ int meta_cols(int m) const { return m; }
    __device__ __forceinline__ int64_t meta_nnz() const { return (int64_t)(offsets[blockIdx.x + 1] - s); }
};

__global__ __launch_bounds__(1024) void k_sparse_batch_solve(SparseBatchArgs a) {
    const int b = blockIdx.x;
    const SparseBatchCheck ck = a.chk[b];
    const long long s = a.offsets[b];
    const SparseBatchRows rows{a.loc, a.val, a.offsets, s, a.row_start + s + b, a.s.maximize};
    batch_solve(a.s, rows, ck.last_row + 1, ck.max_col + 1, ck.absmax_bits);
}

// ---- status mode (misslap_solve_sparse_batch_status): a verdict per problem instead of all or nothing

struct SparseBatchStatusArgs {
    SparseBatchArgs d;       // d.s.Ns / Ms = sol_ld / prices_ld: the caller's bound on every problem (dims), the LDS carve
    const long long *sizes;  // [B][2] or null: from_sparse's `size` of each problem (N = sizes[b][1], auction_.pyx:592)
    const int *card;         // [B] the guard's cardinalities (-1: not matched), or null: no guard in this call
    int fast;                // eps_start = 1 / N of each problem (:614-615)
    int *status;             // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;      // [B] or null: the guard's cardinality, -1 where it did not run
};

// a check record's maximum as a count: max + 1, 0 without a non-negative index, saturated at INT_MAX
__device__ __forceinline__ int sparse_batch_count(int mx) { return mx < 0 ? 0 : (mx == INT_MAX ? INT_MAX : mx + 1); }

// The sparse checks of a verdict ahead of the starting prices, in the order of misslap_solve_sparse_batch
// (abi_sparse_batch.hpp: pre_guard_error, the guard, AuctionSolver.__init__, the cap, the leading dimensions);
// batch_verdict adds the prices.  N: the reference's N of :592 / :594; card: the guard's cardinality, -1 without one.
__device__ __forceinline__ int sparse_batch_verdict(const SparseBatchCheck &c, long long nnz, long long N, int fast,
                                                    int card, int Ns, int Ms, long long p0_ld, bool has_p0) {
    if (nnz == 0) return MISSLAP_BATCH_STATUS_NO_ENTRIES;
    if (fast && N == 0) return MISSLAP_BATCH_STATUS_DIVISION_BY_ZERO;
    if (nnz < N) return MISSLAP_BATCH_STATUS_TOO_FEW_VALUES;
    if (card >= 0 && card < c.max_row + 1) return MISSLAP_BATCH_STATUS_INFEASIBLE;  // (matched: max_row + 1 <= the cap)
    if (c.last_row < 0 || (c.err & kErrColNegative)) return MISSLAP_BATCH_STATUS_NEGATIVE_INDEX;
    if (c.err & kErrRowsUnsorted) return MISSLAP_BATCH_STATUS_ROWS_UNSORTED;
    if (c.err & kErrRowGap) return MISSLAP_BATCH_STATUS_ROW_GAP;
    if (c.err & kErrNonFinite) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    // (from here on rows ascend from 0 without a gap and no index is negative: n = last_row + 1 = max_row + 1 <= nnz)
    // (Ns, Ms <= MISSLAP_SPARSE_BATCH_MAX_DIM: a column whose + 1 does not fit an int32 is beyond Ms too)
    if (c.last_row >= Ns || c.max_col >= Ms) return MISSLAP_BATCH_STATUS_TOO_LARGE;
    if (has_p0 && c.max_col >= p0_ld) return MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW;
    return MISSLAP_BATCH_STATUS_OK;
}

// k_sparse_batch_solve with the verdict formed here, from what the check pass and the guard left on the device.  A
// condemned problem's workgroup writes the defined outputs and leaves before any LDS state exists and before anything of
// loc, val or the row starts is read: an index beyond the carve never reaches the price array.  The others run the same
// batch_solve on the same row source.
__global__ __launch_bounds__(1024) void k_sparse_batch_solve_status(SparseBatchStatusArgs a) {
    const int b = blockIdx.x;
    const SparseBatchCheck ck = a.d.chk[b];
    const long long s = a.d.offsets[b];
    const long long nnz = a.d.offsets[b + 1] - s;
    const long long N = a.sizes ? a.sizes[2 * b + 1] : (long long)ck.max_row;  // sic, :592 / :594
    const int card = a.card ? a.card[b] : -1;
    const int own = sparse_batch_verdict(ck, nnz, N, a.fast, card, a.d.s.Ns, a.d.s.Ms, a.d.s.p0_ld, a.d.s.p0 != nullptr);
    const int code = batch_verdict(own, false, 0, 0, ck.bad_price);
    batch_publish_verdict(a.status, a.matching_size, b, code, card);
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(a.d.s, sparse_batch_count(ck.max_row), sparse_batch_count(ck.max_col), nnz);
        return;
    }
    BatchSolveArgs bs = a.d.s;
    if (a.fast) batch_fast_eps(bs, (double)N);
    const SparseBatchRows rows{a.d.loc, a.d.val, a.d.offsets, s, a.d.row_start + s + b, bs.maximize};
    batch_solve(bs, rows, ck.last_row + 1, ck.max_col + 1, ck.absmax_bits);
}

}  // namespace misslap
