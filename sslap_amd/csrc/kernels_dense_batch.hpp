// kernels_dense_batch.hpp -- many small dense problems, one workgroup per problem for its whole solve
// (misslap_solve_dense_batch, include/misslap.h; the host side is abi_dense_batch.hpp).
//
// A problem of at most MISSLAP_DENSE_BATCH_MAX_DIM rows and columns keeps the whole state of the reference's solver
// (auction_.pyx:167-200) in LDS: prices, person_to_object, object_to_person, the unassigned list, the per-object best
// key / position and the round's bids.  Values are read from the caller's dense rows (row stride = the stack's M) in
// global memory, where a small problem stays in L2.  One workgroup runs the epsilon-scaling loop of solve()
// (:268-306) from the first bid to the last eCE check without returning to the host, so B problems take one launch.
//
// Per round, each step separated from the next by a workgroup barrier:
//   BID      one wavefront per unassigned list position: lanes scan the row in column order (lane l holds columns
//            l, l + 64, ...), the row's top two of a_ij - p_j under the reference's ">=" rule are reduced across lanes
//            (top2_wave_reduce), bid = (costbest - wi) + eps in fp64 with fp32 eps (:339-365).  The bid's key goes into
//            bid_key[k] and through ds_max_u64 into bkey[j].
//   RESOLVE  among the positions holding an object's best key, the smallest wins (ds_min_u32): strict ">" in list
//            order (:375-385).
//   ASSIGN   every winner at once.  The writes of distinct winners touch distinct objects, persons and list slots, so
//            this is the reference's ascending-j walk (:388-427): the winner's price, the evicted owner takes the
//            winner's slot, else the slot becomes a hole.
//   COMPACT  push_all_left (:137-162, :430): the k-th hole in [0, K') receives the k-th person in [K', K).  (With N <= M
//            the reference's bound `size = num_cols` is never reached; with N > M the problem has no complete
//            assignment and the reference reads past its list.)
// After the round: terminate() (:308-309), and at the end of a phase eps *= theta or stop (:275-292), with the eCE test
// of :443-485 at target eps = 1 / N.
#pragma once

namespace misslap {

constexpr int kDenseBatchMaxDim = MISSLAP_DENSE_BATCH_MAX_DIM;
constexpr int kDenseBatchCols = kDenseBatchMaxDim / kWave;  // columns per lane in a row scan

// per problem, from the validation pass ahead of the solve
struct DenseBatchCheck {
    unsigned long long nvalid;       // valid entries of the slice
    unsigned long long absmax_bits;  // max |v| over them, as bits (non-negative doubles order like their bit patterns)
    int empty_row;                   // first row without a valid entry (INT_MAX: none)
    int has_inf;                     // a valid entry is +inf
    int mref;                        // max valid column + 1 (auction_.pyx:209-212)
    int bad_price;                   // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
};

struct DenseBatchArgs {
    const double *mat;
    long long N, M;           // the stack: row stride M, problem stride N * M
    const int *shapes;        // [B][2] (n_b, m_b) or null
    const float *eps_b;       // [B] or null
    float eps_opt;
    const double *p0;         // [B][M] or null
    const DenseBatchCheck *chk;
    int maximize;
    long long max_iter;
    int *sol;                 // [B][N]
    double *prices;           // [B][M] or null
    misslap_dense_batch_meta *meta;  // [B]
};

__device__ __forceinline__ void dense_batch_shape(const int *shapes, long long N, long long M, int b, int &n, int &m) {
    n = shapes ? shapes[2 * b] : (int)N;
    m = shapes ? shapes[2 * b + 1] : (int)M;
}

// Validation, one workgroup per problem: valid count, empty rows, +inf, C = max |v|, the reference's M, prices.
__global__ __launch_bounds__(256) void k_dense_batch_check(const double *mat, long long N, long long M, const int *shapes,
                                                           const double *p0, DenseBatchCheck *out) {
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int n, m;
    dense_batch_shape(shapes, N, M, b, n, m);
    const double *A = mat + (size_t)b * (size_t)N * (size_t)M;
    __shared__ unsigned long long s_cnt, s_abs;
    __shared__ int s_empty, s_inf, s_mref, s_badp;
    if (threadIdx.x == 0) {
        s_cnt = 0;
        s_abs = 0;
        s_empty = 0x7fffffff;
        s_inf = 0;
        s_mref = 0;
        s_badp = 0;
    }
    __syncthreads();
    unsigned long long cnt = 0, am = 0;
    int inf = 0, mx = -1;
    for (int r = wave; r < n; r += nw) {
        const double *row = A + (size_t)r * (size_t)M;
        int rc = 0;
        for (int c = lane; c < m; c += kWave) {
            const double v = row[c];
            if (dense_entry_valid(v)) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
                ++rc;
                am = bits > am ? bits : am;
                inf |= bits == 0x7ff0000000000000ull;
                mx = c > mx ? c : mx;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) rc += __shfl_xor(rc, off);
        if (rc == 0 && lane == 0) atomicMin(&s_empty, r);
        cnt += (unsigned long long)rc;  // (uniform; lane 0's copy is added below)
    }
    if (lane == 0) atomicAdd(&s_cnt, cnt);
    if (am) atomicMax(&s_abs, am);
    if (inf) atomicOr(&s_inf, 1);
    if (mx >= 0) atomicMax(&s_mref, mx + 1);
    if (p0) {
        int bad = 0;
        for (int j = threadIdx.x; j < m; j += blockDim.x) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(p0[(size_t)b * (size_t)M + j]);
            bad |= (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull ? 1 : 0;
            bad |= (bits >> 63) ? 2 : 0;
        }
        if (bad) atomicOr(&s_badp, bad);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DenseBatchCheck r;
        r.nvalid = s_cnt;
        r.absmax_bits = s_abs;
        r.empty_row = s_empty;
        r.has_inf = s_inf;
        r.mref = s_mref;
        r.bad_price = s_badp;
        out[b] = r;
    }
}

// LDS of one problem, carved from the dynamic allocation (sized by the stack's N and M): 24 M + 28 N bytes
__host__ __device__ constexpr size_t dense_batch_lds_bytes(long long N, long long M) {
    return (size_t)M * (8 + 8 + 4 + 4) + (size_t)N * (8 + 4 + 4 + 4 + 4 + 4);
}

// eCE_satisfied(eps) (auction_.pyx:443-485, tol = 1e-7) on a state with everybody assigned.  In a dense row every column
// is stored once, so choice_cost -- never reset per row in the reference -- is the cost of the row's own column.
__device__ __forceinline__ bool dense_batch_ece(const double *A, long long M, int n, int m, int maximize,
                                                const double *price, const int *p2o, float eps_f, int *s_fail) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double tol = 1e-7, eps = (double)eps_f;
    if (threadIdx.x == 0) *s_fail = 0;
    __syncthreads();
    for (int i = wave; i < n; i += nw) {
        const double *row = A + (size_t)i * (size_t)M;
        const int j = p2o[i];
        const double vj = row[j];
        const double choice_cost = maximize ? vj : vj * -1.0;
        const double LHS = choice_cost - price[j] + tol;  // :475
        bool bad = false;
        for (int c = lane; c < m; c += kWave) {
            const double v = row[c];
            if (!dense_entry_valid(v)) continue;
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[c]) - eps) bad = true;  // :482
        }
        if (__ballot(bad) && lane == 0) *s_fail = 1;
    }
    __syncthreads();
    const bool ok = *s_fail == 0;
    __syncthreads();  // (s_fail is rewritten by the next call)
    return ok;
}

__global__ __launch_bounds__(1024) void k_dense_batch_solve(DenseBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_holes, s_nmove, s_fail;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = T >> 6;
    const int Ns = (int)a.N, Ms = (int)a.M;
    int n, m;
    dense_batch_shape(a.shapes, a.N, a.M, b, n, m);
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

    const DenseBatchCheck ck = a.chk[b];
    const double *A = a.mat + (size_t)b * (size_t)a.N * (size_t)a.M;
    const double *P0 = a.p0 ? a.p0 + (size_t)b * (size_t)a.M : nullptr;
    // AuctionSolver.__init__ (:241-252): C = max |a_ij| as a float, eps0 = C / 2 unless eps_start > 0
    const float C = (float)__longlong_as_double((long long)ck.absmax_bits);
    float eps = (float)((double)C / 2.0);
    const float target_eps = (float)(1.0 / (double)n);
    const float theta = (float)0.15;
    const float e0 = a.eps_b ? a.eps_b[b] : a.eps_opt;
    if (e0 > 0) eps = e0;
    const float start_eps = eps;

    for (int j = tid; j < Ms; j += T) {
        price[j] = (P0 && j < m) ? P0[j] : 0.0;
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
        // ---- BID (:339-365)
        for (int k = wave; k < K; k += nw) {
            const int i = U[k];
            const double *row = A + (size_t)i * (size_t)a.M;
            double vals[kDenseBatchCols];
#pragma unroll
            for (int q = 0; q < kDenseBatchCols; ++q) {
                if (q * kWave >= m) break;
                const int c = lane + q * kWave;
                vals[q] = c < m ? row[c] : -1.0;
            }
            Top2 x;
            x.v = -__builtin_huge_val();
            x.w = -__builtin_huge_val();
            x.g = -1;
            double cb = 0.0;
#pragma unroll
            for (int q = 0; q < kDenseBatchCols; ++q) {
                if (q * kWave >= m) break;
                const int c = lane + q * kWave;
                if (c < m && dense_entry_valid(vals[q])) {
                    const double cost = a.maximize ? vals[q] : vals[q] * -1.0;  // :236-237
                    const double vi = cost - price[c];
                    if (vi >= x.v) {  // :351 (the first entry is always taken: vi >= -inf for every non-NaN vi)
                        x.w = x.v;
                        x.v = vi;
                        x.g = c;
                        cb = cost;
                    } else if (vi > x.w) {
                        x.w = vi;
                    }
                }
            }
            const Top2 r = top2_wave_reduce(x);
            const double costbest = readlane_f64(cb, r.g & (kWave - 1));  // the lane that holds column r.g
            const double bid = costbest - r.w + (double)eps;               // :360
            if (lane == 0) {
                const unsigned long long key = bid_to_key(bid);
                bid_key[k] = key;
                bid_obj[k] = r.g;
                atomicMax(&bkey[r.g], key);
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
        const bool optimal = K == 0 && dense_batch_ece(A, a.M, n, m, a.maximize, price, p2o, target_eps, &s_fail);
        if (nits >= a.max_iter || optimal) break;
        if (K == 0) {
            if (eps < target_eps) break;  // :280
            eps = eps * theta;            // :283
            for (int j = tid; j < Ms; j += T) o2p[j] = -1;  // :287
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
    const bool ece = K == 0 && dense_batch_ece(A, a.M, n, m, a.maximize, price, p2o, target_eps, &s_fail);
    int *sol = a.sol + (size_t)b * (size_t)a.N;
    for (int i = tid; i < Ns; i += T) sol[i] = i < n ? p2o[i] : -1;
    if (a.prices) {
        double *po = a.prices + (size_t)b * (size_t)a.M;
        for (int j = tid; j < Ms; j += T) po[j] = j < m ? price[j] : 0.0;
    }
    // get_obj (:489-523): a double sum in row order.  The selected values are gathered into LDS (the bid keys are no
    // longer needed), then one lane adds them in order.
    double *selv = reinterpret_cast<double *>(bid_key);
    for (int i = tid; i < n; i += T) {
        const int j = p2o[i];
        selv[i] = j >= 0 ? A[(size_t)i * (size_t)a.M + j] : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double obj = 0;
        for (int i = 0; i < n; ++i) {
            if (p2o[i] == -1) continue;
            const double val = a.maximize ? selv[i] : selv[i] * -1.0;
            if (a.maximize) obj += val;
            else obj -= val;
        }
        misslap_dense_batch_meta r;
        r.struct_size = (int32_t)sizeof(misslap_dense_batch_meta);
        r.n_rows = n;
        r.n_cols = ck.mref;
        r.eCE = ece ? 1 : 0;
        r.nnz = (int64_t)ck.nvalid;
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
