// kernels_batch_solve.hpp -- the round loop of the one-workgroup-per-problem batch solves, shared by
// every solve kernel of kernels_dense_batch.hpp, kernels_sparse_batch.hpp and kernels_ell_batch.hpp, and what those
// kernels share around it: the verdict of a status-mode problem, the outputs of a condemned one, the eps of `fast`, the
// outside option of a row and the outputs of an outside call.  The host side is batch_solve_launch in
// abi_batch_common.hpp.
//
// A problem within the batch caps (MISSLAP_DENSE_BATCH_MAX_DIM, MISSLAP_SPARSE_BATCH_MAX_DIM) keeps the whole state of
// the reference's solver (auction_.pyx:167-200) in LDS: prices, person_to_object, object_to_person, the unassigned
// list, the per-object best key / position and the round's bids.  One workgroup runs the epsilon-scaling loop of solve()
// (:268-306) from the first bid to the last eCE check without returning to the host, so B problems take one launch.
//
// Per round, each step separated from the next by a workgroup barrier:
//   BID      one wavefront per unassigned list position: the row source scans person i's row, reduces the row's top two
//            of a_ij - p_j under the reference's ">=" rule across lanes (top2_wave_reduce) and names the winning object;
//            bid = (costbest - wi) + eps in fp64 with fp32 eps (:339-365).  The bid's key goes into bid_key[k] and
//            through ds_max_u64 into bkey[j].
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
//
// A row source supplies what differs between the layouts.  There are two: DenseBatchRows (kernels_dense_batch.hpp) and
// the list row source ListBatchRows below, which SparseBatchRows and EllBatchRows name with their run accessors:
//   bid(i, price, cb, obj)          the wavefront's reduced Top2 of row i, the winner's cost (all lanes) and its object
//   ece_bad(i, j, price, tol, eps)  this lane's part of the eCE row test of row i assigned to object j
//   gather(p2o, n, selv, nsel)      the objective's per-row gather into LDS (after the last barrier of the loop)
//   objective(p2o, n, selv, nsel)   the sum of get_obj, on one lane, in the reference's order
//   meta_cols(m), meta_nnz()        the meta record's n_cols and nnz
// Only the problem's own m objects and n persons are initialised and reset; the slots beyond them in the carve are
// never read.
#pragma once

namespace misslap {

// What every solve takes per batch (the first member of DenseBatchArgs / SparseBatchArgs / EllBatchArgs; filled by
// batch_solve_launch)
struct BatchSolveArgs {
    const float *eps_b;        // [B] or null
    float eps_opt;
    const double *p0;          // [B][p0_ld] or null
    long long p0_ld;
    int maximize;
    long long max_iter;
    int Ns, Ms;                // the batch's largest n_b / m_b: the LDS carve
    int *sol;                  // [B][sol_ld]
    long long sol_ld;
    double *prices;            // [B][prices_ld] or null
    long long prices_ld;
    misslap_dense_batch_meta *meta;  // [B]
};

// LDS of one problem, carved from the dynamic allocation (sized by the batch's Ns and Ms): 24 M + 28 N bytes
__host__ __device__ constexpr size_t batch_solve_lds_bytes(long long N, long long M) {
    return (size_t)M * (8 + 8 + 4 + 4) + (size_t)N * (8 + 4 + 4 + 4 + 4 + 4);
}

// Where batch_solve keeps the prices and person_to_object of its problem in that allocation (s_raw: its start), for a
// kernel that reads them behind it: both hold the final state once batch_solve has returned.  The offsets follow the
// carve at the top of batch_solve -- price[Ms], bkey[Ms], bid_key[Ns], o2p[Ms], bpos[Ms], p2o[Ns], ... -- and must move
// with it.
__device__ __forceinline__ const double *batch_solve_price(const unsigned char *s_raw) {
    return reinterpret_cast<const double *>(s_raw);
}
__device__ __forceinline__ const int *batch_solve_p2o(const unsigned char *s_raw, int Ns, int Ms) {
    return reinterpret_cast<const int *>(s_raw + (size_t)Ms * (8 + 8 + 4 + 4) + (size_t)Ns * 8);
}

// The starting prices p[0 .. m) of one problem in a check pass: bit 0 NaN / infinity, bit 1 sign bit set, into *s_badp
__device__ __forceinline__ void batch_check_prices(const double *p, int m, int *s_badp) {
    int bad = 0;
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(p[j]);
        bad |= (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull ? 1 : 0;
        bad |= (bits >> 63) ? 2 : 0;
    }
    if (bad) atomicOr(s_badp, bad);
}

// The part of a status-mode verdict (MISSLAP_BATCH_STATUS_*, include/misslap.h) that every layout shares.  `code` is
// what the layout's own checks of the values gave (0: none failed); behind them, in the order of the all-or-nothing
// calls: the matching guard (card: its cardinality; guarded: it ran for this call), then the starting prices.
__device__ __forceinline__ int batch_verdict(int code, bool guarded, int card, int n, int bad_price) {
    if (code) return code;
    if (guarded && card < n) return MISSLAP_BATCH_STATUS_INFEASIBLE;
    if (bad_price & 1) return MISSLAP_BATCH_STATUS_PRICE_NOT_FINITE;
    if (bad_price & 2) return MISSLAP_BATCH_STATUS_PRICE_NEGATIVE;
    return MISSLAP_BATCH_STATUS_OK;
}

// The outputs of a condemned problem (status != 0), written by its whole workgroup before any LDS state exists:
// sol[b][:] = -1, prices[b][:] = 0, and a meta record that holds the three counts of the check pass and zeros.
__device__ __forceinline__ void batch_condemn(const BatchSolveArgs &a, int n, int n_cols, long long nnz) {
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    int *sol = a.sol + (size_t)b * (size_t)a.sol_ld;
    for (long long i = tid; i < a.sol_ld; i += T) sol[i] = -1;
    if (a.prices) {
        double *po = a.prices + (size_t)b * (size_t)a.prices_ld;
        for (long long j = tid; j < a.prices_ld; j += T) po[j] = 0.0;
    }
    if (tid == 0) {
        misslap_dense_batch_meta r{};
        r.struct_size = (int32_t)sizeof(misslap_dense_batch_meta);
        r.n_rows = n;
        r.n_cols = n_cols;
        r.nnz = nnz;
        a.meta[b] = r;
    }
}

// The verdict of problem b and the guard's cardinality (-1 where it did not run), published by thread 0
__device__ __forceinline__ void batch_publish_verdict(int *status, int *matching_size, int b, int code, int card) {
    if (threadIdx.x == 0) {
        status[b] = code;
        if (matching_size) matching_size[b] = card;
    }
}

// `fast`: the problem starts at eps = 1 / n (auction_.pyx:568-569, :614-615) -- the front end's
// (1.0 / float64(n)).astype(float32), the same two IEEE operations
__device__ __forceinline__ void batch_fast_eps(BatchSolveArgs &s, double n) {
    s.eps_b = nullptr;
    s.eps_opt = (float)(1.0 / n);
}

// One entry's net value vi, with tie key `key`, into a lane's running top two under the reference's ">=" rule (:351; the
// first entry is always taken: vi >= -inf for every non-NaN vi).  True where it became the best: the caller then keeps
// its cost and its object.
__device__ __forceinline__ bool top2_take(Top2 &x, double vi, int key) {
    if (vi >= x.v) {
        x.w = x.v;
        x.v = vi;
        x.g = key;
        return true;
    }
    if (vi > x.w) x.w = vi;
    return false;
}

// The outside option of the rows of one problem (the <.., true> row sources): row i's value is O[i * stride] (stride 0:
// one value for the problem), its object is the problem's m + i.  Empty in the plain mode.
template <bool Out>
struct BatchOutside {};
template <>
struct BatchOutside<true> {
    const double *O;
    int stride;
    __device__ __forceinline__ double value(int i) const { return O[i * stride]; }
};

// The list row source of batch_solve, for every layout whose row is a run of (column, value) entries in stored order:
// the sparse batch's packed arrays and views, and the ELL batch's padded candidate lists.  A run accessor Acc states
// what differs between them:
//   start(i), len(i)     where row i's run begins (in the accessor's own index width) and how many slots it has
//   col(g), value(g)     entry g's column and value, in their stored types; the value is widened where it is used
//                        (dense_widen, exact), the column is compared in its own width and narrowed only once it is
//                        known to be an entry, so an int64 column is never narrowed before it is tested
//   kHoles               whether a negative column is a hole: skipped before anything is done with its column (it never
//                        indexes price[]), and its value is never interpreted
//   count()              the problem's entries, for the meta record
// Everything else is here once: the stored order the reference's AuctionSolver walks (flat_j / val after
// cumulative_idxs, auction_.pyx:33-48, :202-233), the tie key and the outside entry.
//   BID      lane l holds the row's slots l, l + 64, ... (rows of any length), the tie key is the slot index:
//            top2_wave_reduce keeps the reference's ">=" rule (the last stored maximum wins, :351) and counts a repeated
//            maximum -- a duplicate (i, j) entry included -- into the second best as the sequential scan does (:353).
//            Dropping holes keeps the order of the entries and the key is only ever compared, so the slot index serves
//            as the stored index.
//   eCE      choice_cost is the value at the LAST slot of row i whose column is p2o[i] (the loop of :462-467 overwrites
//            it on every match), then every entry is tested against it (:475-485).
//   get_obj  every entry whose column is p2o[i] is added, in row order and slot order (:508-521): a duplicate of the
//            chosen entry counts once per copy.
// Out: the row's virtual last entry (i, m + i) with the row's outside value.  Its tie key is len, above every slot, and
// lane len & 63 takes it AFTER its own slots (slot len would be that lane's next one), so every lane still scans in
// ascending stored order, the virtual entry wins ">=" ties as the last stored entry must, and the winner's lane is
// r.g & 63 as before.  A row of len = 0 is a one-entry row: its second best is -inf and it bids +inf.  A chosen object
// j >= m is that entry: nothing of the run is read for it.
template <class Acc, bool Out>
struct ListBatchRows {
    using Col = typename Acc::Col;  // the column's stored width
    Acc a;
    int maximize;
    int m;  // the real columns (read in the outside mode only)
    BatchOutside<Out> out;

    // the row in stored order, lane l at slots l, l + 64, ...; the tie key is the slot index
    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        const auto g0 = a.start(i);
        const int len = a.len(i);
        Top2 x;
        x.v = -__builtin_huge_val();
        x.w = -__builtin_huge_val();
        x.g = -1;
        double cb = 0.0;
        int cj = 0;
        for (int q = lane; q < len; q += kWave) {
            const Col c = a.col(g0 + q);
            const auto e = a.value(g0 + q);
            if constexpr (Acc::kHoles)
                if (c < 0) continue;
            const double v = dense_widen(e);
            const double cost = maximize ? v : v * -1.0;  // :236-237
            const double vi = cost - price[(int)c];
            // (top2_take, spelled out: through the helper the sparse instances number the running state's registers in
            // another order, and here every solve instance is the code it was before the sources were folded)
            if (vi >= x.v) {
                x.w = x.v;
                x.v = vi;
                x.g = q;
                cb = cost;
                cj = (int)c;
            } else if (vi > x.w) {
                x.w = vi;
            }
        }
        if constexpr (Out) {
            if (lane == (len & (kWave - 1))) {
                const double v = out.value(i);
                const double cost = maximize ? v : v * -1.0;
                const double vi = cost - price[m + i];
                if (top2_take(x, vi, len)) {
                    cb = cost;
                    cj = m + i;
                }
            }
        }
        const Top2 r = top2_wave_reduce(x);
        const int gl = r.g & (kWave - 1);  // the lane that holds slot r.g
        costbest = readlane_f64(cb, gl);
        obj = __builtin_amdgcn_readlane(cj, gl);
        return r;
    }

    // eCE_satisfied (auction_.pyx:443-485) for row i: choice_cost from the last slot of column j (j >= 0: never a hole)
    __device__ __forceinline__ bool ece_bad(int i, int j, const double *price, double tol, double eps) const {
        const int lane = lane_id();
        const auto g0 = a.start(i);
        const int len = a.len(i);
        int last = -1;  // :462-467
        for (int q = lane; q < len; q += kWave)
            if (a.col(g0 + q) == (Col)j) last = q;
        last = wave_max_i32(last);
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : dense_widen(a.value(g0 + (last < 0 ? 0 : last)));  // (j < m: stored)
        else vj = dense_widen(a.value(g0 + last));
        const double choice_cost = maximize ? vj : vj * -1.0;
        const double LHS = choice_cost - price[j] + tol;  // :475
        bool bad = false;
        if constexpr (Out) {
            if (lane == 0) {
                const double v = out.value(i);
                const double cost = maximize ? v : v * -1.0;
                if (LHS < (cost - price[m + i]) - eps) bad = true;
            }
        }
        for (int q = lane; q < len; q += kWave) {
            const Col c = a.col(g0 + q);
            if constexpr (Acc::kHoles)
                if (c < 0) continue;
            const double v = dense_widen(a.value(g0 + q));
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[(int)c]) - eps) bad = true;  // :482
        }
        return bad;
    }

    // get_obj (:489-523) over EVERY entry of the chosen column: a wavefront per row gathers the row's one matching value;
    // a row with several matches (a repeated column) is marked (nsel[i] > 1) and re-walked by the summing lane.
    __device__ __forceinline__ void gather(const int *p2o, int n, double *selv, int *nsel) const {
        const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int i = wave; i < n; i += nw) {
            const int j = p2o[i];
            if (j < 0) continue;
            if constexpr (Out) {
                if (j >= m) {  // the row's outside entry: exactly one match
                    if (lane == 0) {
                        nsel[i] = 1;
                        selv[i] = out.value(i);
                    }
                    continue;
                }
            }
            const auto g0 = a.start(i);
            const int len = a.len(i);
            int cnt = 0, at = -1;
            for (int q = lane; q < len; q += kWave)
                if (a.col(g0 + q) == (Col)j) {
                    ++cnt;
                    at = q;
                }
            for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
            at = wave_max_i32(at);
            if (lane == 0) {
                nsel[i] = cnt;
                selv[i] = dense_widen(a.value(g0 + at));
            }
        }
    }

    // a double sum in row order, within a row in slot order
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
            const auto g0 = a.start(i);
            const int len = a.len(i);
            for (int q = 0; q < len; ++q)
                if (a.col(g0 + q) == (Col)j) {
                    const double e = dense_widen(a.value(g0 + q));
                    const double v = maximize ? e : e * -1.0;
                    if (maximize) obj += v;
                    else obj -= v;
                }
        }
        return obj;
    }

    // (m_: batch_solve's object count, in the outside mode m + n)
    __device__ __forceinline__ int meta_cols(int m_) const { return m_; }
    __device__ __forceinline__ int64_t meta_nnz() const { return a.count(); }
};

// The price outputs of an outside call (po: [M_ld] the real columns, oo: [N_ld] the outside objects, either may be null)
// for a condemned problem, next to batch_condemn: zeros.  (tid, T: threadIdx.x and blockDim.x as the kernel read them at
// its top -- read here instead, the same values change the schedule of the whole kernel.)
__device__ __forceinline__ void batch_outside_condemn(double *po, int M_ld, double *oo, int N_ld, int tid, int T) {
    if (po)
        for (int j = tid; j < M_ld; j += T) po[j] = 0.0;
    if (oo)
        for (int i = tid; i < N_ld; i += T) oo[i] = 0.0;
}

// The outputs of an outside call in the caller's terms, behind batch_solve(s, ..) on the n x (m + n) problem, from the LDS
// state it leaves (nothing writes price[] or p2o[] behind its last barrier, and every thread rewrites only the sol cells
// it wrote itself): an object >= m becomes -1 in sol, price[0 .. m) are the real prices, price[m .. m + n) the outside ones.
__device__ __forceinline__ void batch_outside_outputs(const unsigned char *s_raw, const BatchSolveArgs &s, int b, int n,
                                                      int m, int M_ld, int N_ld, double *po, double *oo, int tid,
                                                      int T) {
    const double *price = batch_solve_price(s_raw);
    const int *p2o = batch_solve_p2o(s_raw, s.Ns, s.Ms);
    int *sol = s.sol + (size_t)b * (size_t)s.sol_ld;
    for (int i = tid; i < n; i += T)
        if (p2o[i] >= m) sol[i] = -1;
    if (po)
        for (int j = tid; j < M_ld; j += T) po[j] = j < m ? price[j] : 0.0;
    if (oo)
        for (int i = tid; i < N_ld; i += T) oo[i] = i < n ? price[m + i] : 0.0;
}

// Whether a row source has a second bid mapping for whole rounds, bid_lanes(U, K, price, eps, bid_key, bid_obj, bkey):
// it makes the K bids of a round itself (keys, objects and the per-object maxima, as the BID step below leaves them) and
// returns true, or does nothing and returns false.  Only the strided dense source has one (kernels_dense_batch.hpp);
// for every other source the BID step compiles to what it was.
template <class Rows>
struct RowsBidLanes {
    static constexpr bool value = false;
};

// eCE_satisfied(eps) (auction_.pyx:443-485, tol = 1e-7) on a state with everybody assigned; one wavefront per row.
template <class Rows>
__device__ __forceinline__ bool batch_ece(const Rows &rows, int n, const double *price, const int *p2o, float eps_f,
                                          int *s_fail) {
    const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double tol = 1e-7, eps = (double)eps_f;
    if (threadIdx.x == 0) *s_fail = 0;
    __syncthreads();
    for (int i = wave; i < n; i += nw) {
        const bool bad = rows.ece_bad(i, p2o[i], price, tol, eps);
        if (__ballot(bad) && lane == 0) *s_fail = 1;
    }
    __syncthreads();
    const bool ok = *s_fail == 0;
    __syncthreads();  // (s_fail is rewritten by the next call)
    return ok;
}

// The solve of problem blockIdx.x: n persons, m objects, C = max |a_ij| as bits.
template <class Rows>
__device__ __forceinline__ void batch_solve(const BatchSolveArgs &a, const Rows &rows, int n, int m,
                                            unsigned long long absmax_bits) {
    // (the order of the carve below is restated by batch_solve_price / batch_solve_p2o above, for batch_outside_outputs,
    // which reads the final state behind this function.  Change both together.)
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_holes, s_nmove, s_fail;
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = T >> 6;
    const int Ns = a.Ns, Ms = a.Ms;
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

    const double *P0 = a.p0 ? a.p0 + (size_t)b * (size_t)a.p0_ld : nullptr;
    // AuctionSolver.__init__ (:241-252): C = max |a_ij| as a float, eps0 = C / 2 unless eps_start > 0
    const float C = (float)__longlong_as_double((long long)absmax_bits);
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
        // ---- BID (:339-365)
        bool bid_done = false;
        if constexpr (RowsBidLanes<Rows>::value) bid_done = rows.bid_lanes(U, K, price, eps, bid_key, bid_obj, bkey);
        for (int k = wave; !bid_done && k < K; k += nw) {
            double costbest;
            int j;
            const Top2 r = rows.bid(U[k], price, costbest, j);
            const double bid = costbest - r.w + (double)eps;  // :360
            if (lane == 0) {
                const unsigned long long key = bid_to_key(bid);
                bid_key[k] = key;
                bid_obj[k] = j;
                atomicMax(&bkey[j], key);
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
        const bool optimal = K == 0 && batch_ece(rows, n, price, p2o, target_eps, &s_fail);
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
    const bool ece = K == 0 && batch_ece(rows, n, price, p2o, target_eps, &s_fail);
    // (int loop bounds: a 64-bit bound costs the dense kernel a VGPR; a row is written up to 2^31 - 1 entries)
    const int sol_n = (int)(a.sol_ld < INT_MAX ? a.sol_ld : INT_MAX);
    const int prices_n = (int)(a.prices_ld < INT_MAX ? a.prices_ld : INT_MAX);
    int *sol = a.sol + (size_t)b * (size_t)a.sol_ld;
    for (int i = tid; i < sol_n; i += T) sol[i] = i < n ? p2o[i] : -1;
    if (a.prices) {
        double *po = a.prices + (size_t)b * (size_t)a.prices_ld;
        for (int j = tid; j < prices_n; j += T) po[j] = j < m ? price[j] : 0.0;
    }
    // get_obj (:489-523): the chosen values are gathered into LDS (the bid keys and objects are no longer needed), then
    // one lane adds them in row order.
    double *selv = reinterpret_cast<double *>(bid_key);
    int *nsel = bid_obj;
    rows.gather(p2o, n, selv, nsel);
    __syncthreads();
    if (tid == 0) {
        const double obj = rows.objective(p2o, n, selv, nsel);
        misslap_dense_batch_meta r;
        r.struct_size = (int32_t)sizeof(misslap_dense_batch_meta);
        r.n_rows = n;
        r.n_cols = rows.meta_cols(m);
        r.eCE = ece ? 1 : 0;
        r.nnz = rows.meta_nnz();
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
