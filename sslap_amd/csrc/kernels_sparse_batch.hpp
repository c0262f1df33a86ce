// kernels_sparse_batch.hpp -- many small SPARSE problems, one workgroup per problem for its whole solve
// (misslap_solve_sparse_batch, include/misslap.h; the host side is abi_sparse_batch.hpp).
//
// The round structure, the LDS state and the phase loop are those of k_dense_batch_solve (kernels_dense_batch.hpp);
// what differs is where a row comes from.  Problem b is the entries offsets[b] .. offsets[b + 1] of the caller's
// loc / val, in their STORED order -- the order the reference's AuctionSolver walks them (flat_j / val after
// cumulative_idxs, auction_.pyx:33-48, :202-233) -- and row i of it is the run row_start[i] .. row_start[i + 1] that the
// check pass found.  So:
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
    const int *loc;               // [nnz][2]
    const double *val;            // [nnz]
    const long long *offsets;     // [B + 1]
    const int *row_start;         // [nnz + B]: problem b's row starts (local indices) at offsets[b] + b
    const float *eps_b;           // [B] or null
    float eps_opt;
    const double *p0;             // [B][p0_ld] or null
    long long p0_ld;
    const SparseBatchCheck *chk;  // [B]
    int maximize;
    long long max_iter;
    int Ns, Ms;                   // the batch's largest n_b / n_cols: the LDS carve
    int *sol;                     // [B][sol_ld]
    long long sol_ld;
    double *prices;               // [B][prices_ld] or null
    long long prices_ld;
    misslap_dense_batch_meta *meta;  // [B]
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
    if (p0 && s_err == 0 && m > 0) {
        const int mm = (long long)m < p0_ld ? m : (int)p0_ld;  // (the host rejects m > p0_ld)
        int bad = 0;
        for (int j = threadIdx.x; j < mm; j += blockDim.x) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(p0[(size_t)b * (size_t)p0_ld + j]);
            bad |= (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull ? 1 : 0;
            bad |= (bits >> 63) ? 2 : 0;
        }
        if (bad) atomicOr(&s_badp, bad);
    }
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

// LDS of one problem, sized by the batch's largest n_b and n_cols: the layout of k_dense_batch_solve, 24 M + 28 N bytes
__host__ __device__ constexpr size_t sparse_batch_lds_bytes(long long N, long long M) { return dense_batch_lds_bytes(N, M); }

// eCE_satisfied(eps) (auction_.pyx:443-485, tol = 1e-7) on a state with everybody assigned; one wavefront per row.
__device__ __forceinline__ bool sparse_batch_ece(const int *loc, const double *val, long long s, const int *rs, int n,
                                                 int maximize, const double *price, const int *p2o, float eps_f,
                                                 int *s_fail) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double tol = 1e-7, eps = (double)eps_f;
    if (threadIdx.x == 0) *s_fail = 0;
    __syncthreads();
    for (int i = wave; i < n; i += nw) {
        const long long g0 = s + rs[i];
        const int len = rs[i + 1] - rs[i];
        const int j = p2o[i];
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
        if (__ballot(bad) && lane == 0) *s_fail = 1;
    }
    __syncthreads();
    const bool ok = *s_fail == 0;
    __syncthreads();  // (s_fail is rewritten by the next call)
    return ok;
}

__global__ __launch_bounds__(1024) void k_sparse_batch_solve(SparseBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_holes, s_nmove, s_fail;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = T >> 6;
    const int Ns = a.Ns, Ms = a.Ms;
    const SparseBatchCheck ck = a.chk[b];
    const int n = ck.last_row + 1, m = ck.max_col + 1;
    double *price = reinterpret_cast<double *>(s_raw);                           // [M]  auction_.pyx:169
    unsigned long long *bkey = reinterpret_cast<unsigned long long *>(price + Ms); // [M]  :193 best bid as key, 0 = none
    unsigned long long *bid_key = bkey + Ms;                                       // [N]  the round's bids by list position
    int *o2p = reinterpret_cast<int *>(bid_key + Ns);                              // [M]  :178
    int *bpos = o2p + Ms;                                                          // [M]  :194 winning list position
    int *p2o = bpos + Ms;                                                          // [N]  :177
    int *U = p2o + Ns;                                                             // [N]  :199 unassigned list
    int *bid_obj = U + Ns;                                                         // [N]
    int *hole = bid_obj + Ns;                                                      // [N]  push_all_left lists
    int *mover = hole + Ns;                                                        // [N]

    const long long s = a.offsets[b];
    const int *rs = a.row_start + s + b;
    const int *loc = a.loc;
    const double *val = a.val;
    const double *P0 = a.p0 ? a.p0 + (size_t)b * (size_t)a.p0_ld : nullptr;
    // AuctionSolver.__init__ (:241-252): C = max |a_ij| as a float, eps0 = C / 2 unless eps_start > 0
    const float C = (float)__longlong_as_double((long long)ck.absmax_bits);
    float eps = (float)((double)C / 2.0);
    const float target_eps = (float)(1.0 / (double)n);
    const float theta = (float)0.15;
    const float e0 = a.eps_b ? a.eps_b[b] : a.eps_opt;
    if (e0 > 0) eps = e0;
    const float start_eps = eps;

    for (int j = tid; j < m; j += T) {
        price[j] = P0 ? P0[j] : 0.0;
        bkey[j] = 0ull;
        bpos[j] = kPosNone;
        o2p[j] = -1;
    }
    for (int i = tid; i < n; i += T) {
        p2o[i] = -1;
        U[i] = i;
    }
    int K = n;  // num_unassigned, uniform
    long long nits = 0;
    int nred = 0;
    unsigned long long bids = 0;
    __syncthreads();

    for (;;) {  // solve() (:271-292); leaves after at most max_iter rounds
        // ---- BID (:339-365): the row in stored order, lane l at stored indices l, l + 64, ...
        for (int k = wave; k < K; k += nw) {
            const int i = U[k];
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
                const double cost = a.maximize ? v : v * -1.0;  // :236-237
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
            const int gl = r.g & (kWave - 1);                // the lane that holds stored index r.g
            const double costbest = readlane_f64(cb, gl);
            const int jbest = __builtin_amdgcn_readlane(cj, gl);
            const double bid = costbest - r.w + (double)eps;  // :360
            if (lane == 0) {
                const unsigned long long key = bid_to_key(bid);
                bid_key[k] = key;
                bid_obj[k] = jbest;
                atomicMax(&bkey[jbest], key);
            }
        }
        bids += (unsigned long long)K;
        __syncthreads();
        // ---- RESOLVE (:375-385): earliest list position among the holders of the best bid
        for (int k = tid; k < K; k += T) {
            const int j = bid_obj[k];
            if (bid_key[k] == bkey[j]) atomicMin(&bpos[j], k);
        }
        if (tid == 0) s_holes = 0;
        __syncthreads();
        // ---- ASSIGN (:388-427)
        int holes = 0;
        for (int k = tid; k < K; k += T) {
            const int j = bid_obj[k];
            if (bpos[j] == k) {  // (a loser reads the winner's position or kPosNone, never its own)
                const int i = U[k], prev = o2p[j];
                price[j] = key_to_bid(bid_key[k]);  // :397
                if (prev != -1) {
                    p2o[prev] = -1;  // :404
                    U[k] = prev;     // :409
                } else {
                    U[k] = -1;  // :412
                    ++holes;
                }
                p2o[i] = j;  // :417
                o2p[j] = i;  // :418
                bkey[j] = 0ull;     // :421-422
                bpos[j] = kPosNone;
            }
        }
        if (holes) atomicAdd(&s_holes, holes);
        __syncthreads();
        const int Kn = K - s_holes;  // :429
        // ---- push_all_left (:137-162): k-th hole in [0, Kn) <- k-th person in [Kn, K), one wavefront
        if (wave == 0) {
            int cl = 0, cm = 0;
            for (int base = 0; base < K; base += kWave) {
                const int pos = base + lane;
                const int u = pos < K ? U[pos] : -1;
                const bool isl = pos < Kn && u == -1, ism = pos >= Kn && pos < K && u != -1;
                const unsigned long long bl = __ballot(isl), bm = __ballot(ism);
                if (isl) hole[cl + __popcll(bl & lanemask_lt())] = pos;
                if (ism) mover[cm + __popcll(bm & lanemask_lt())] = u;
                cl += __popcll(bl);
                cm += __popcll(bm);
            }
            if (lane == 0) s_nmove = cl;
        }
        __syncthreads();
        for (int q = tid; q < s_nmove; q += T) U[hole[q]] = mover[q];
        __syncthreads();
        K = Kn;
        ++nits;
        // ---- terminate() (:308-309) and the end of an eps-phase (:275-292)
        const bool optimal = K == 0 && sparse_batch_ece(loc, val, s, rs, n, a.maximize, price, p2o, target_eps, &s_fail);
        if (nits >= a.max_iter || optimal) break;
        if (K == 0) {
            if (eps < target_eps) break;  // :280
            eps = eps * theta;            // :283
            for (int j = tid; j < m; j += T) o2p[j] = -1;  // :287
            for (int i = tid; i < n; i += T) {
                p2o[i] = -1;  // :286
                U[i] = i;     // :289
            }
            K = n;   // :288
            ++nred;  // :292
            __syncthreads();
        }
    }

    // ---- meta (:297-304) and the outputs
    const bool ece = K == 0 && sparse_batch_ece(loc, val, s, rs, n, a.maximize, price, p2o, target_eps, &s_fail);
    int *sol = a.sol + (size_t)b * (size_t)a.sol_ld;
    for (int i = tid; i < a.sol_ld; i += T) sol[i] = i < n ? p2o[i] : -1;
    if (a.prices) {
        double *po = a.prices + (size_t)b * (size_t)a.prices_ld;
        for (int j = tid; j < a.prices_ld; j += T) po[j] = j < m ? price[j] : 0.0;
    }
    // get_obj (:489-523): a double sum in row order, within a row in stored order, over EVERY entry of the chosen
    // column.  A wavefront per row gathers the row's one matching value into LDS (the bid keys are no longer needed);
    // a row with several matches (duplicate entries) is marked and re-walked in order by the summing lane.
    double *selv = reinterpret_cast<double *>(bid_key);
    int *nsel = bid_obj;
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
    __syncthreads();
    if (tid == 0) {
        double obj = 0;
        for (int i = 0; i < n; ++i) {
            const int j = p2o[i];
            if (j == -1) continue;
            if (nsel[i] == 1) {
                const double v = a.maximize ? selv[i] : selv[i] * -1.0;
                if (a.maximize) obj += v;
                else obj -= v;
                continue;
            }
            const long long g0 = s + rs[i];
            const int len = rs[i + 1] - rs[i];
            for (int q = 0; q < len; ++q)
                if (loc[2 * (g0 + q) + 1] == j) {
                    const double v = a.maximize ? val[g0 + q] : val[g0 + q] * -1.0;
                    if (a.maximize) obj += v;
                    else obj -= v;
                }
        }
        misslap_dense_batch_meta r;
        r.struct_size = (int32_t)sizeof(misslap_dense_batch_meta);
        r.n_rows = n;
        r.n_cols = m;
        r.eCE = ece ? 1 : 0;
        r.nnz = (int64_t)(a.offsets[b + 1] - s);
        r.its = nits;
        r.n_assigned = n - K;
        r.nreductions = nred;
        r.soln_found = ece ? 1 : 0;  // is_optimal (:433-439)
        r.start_eps = start_eps;
        r.final_eps = eps;
        r.target_eps = target_eps;
        r.obj_f32 = (float)obj;
        r.obj_f64 = obj;
        r.bids_made = bids;
        a.meta[b] = r;
    }
}

}  // namespace misslap
