// kernels_points_candidates.hpp -- two point sets into padded candidate lists: per row the (at most) K nearest columns
// under a per-row limit, in the (B, N, K) cols / vals layout misslap_solve_ell_batch reads in place
// (misslap_points_batch_candidates, include/misslap.h; the host side is abi_points_candidates.hpp).  The (B, N, M) cost
// stack is never stored.  sslap_amd.points_to_ell is the definition; the outputs are that function's bit for bit.
//
// The cost is the chain of kernels_points_batch.hpp (points_load / points_cost, not restated here).  Every column gets
// an integer key
//     key = 0                   the cost is not finite: a NaN or an infinite coordinate, or an overflow (stored as +inf)
//     key = bits(cost) + 1      else: a finite cost is >= +0.0, and non-negative doubles order as their bit patterns
// so (key, column) is the order of the definition -- non-finite costs first, then by cost, ties by column -- and the
// limit is a key as well (points_limit_key): column c is a candidate iff key <= limit key.  Nothing here compares
// floating-point values: the build has -fno-honor-nans.  Coordinates and the limit are classified by
// integer loads of their bits, BEFORE the same coordinates are loaded as values, and an overflow is caught on the
// cost's bits (>= those of +inf, as an unsigned compare).
//
// No per-problem state, so the launch covers the whole GPU: one wavefront per row, four rows per workgroup, the row
// index uniform (x_i comes from a uniform address, as in PointBatchRows::bid), lane l takes columns l, l + 64, ...
//   one streaming pass    each step of 64 columns forms the candidate mask with a ballot; a lane's slot is the running
//                         uniform count plus its prefix in the mask, which is ascending column order without a sort.
//                         Slots at or beyond K are not written; the count runs on.  Holes (cols -1, vals 0.0) behind
//                         the last candidate.  This is the whole work of a row with count <= K.
//   the truncated path    only where count > K: a bisection on the key for the K-th smallest (key, column) -- T, the
//                         smallest key with at least K candidates at or below it; every candidate below T is kept and
//                         the first (K - their number) at T in column order -- that recomputes the costs in every step
//                         (no register array: the streaming pass pays nothing for it) and ends early where a midpoint
//                         has exactly K at or below it; then the same column-order compaction with that test, which
//                         rewrites all K slots.
#pragma once

namespace misslap {

constexpr int kPointsCandidatesMaxK = MISSLAP_POINTS_CANDIDATES_MAX_K;
constexpr int kPointsCandidatesThreads = 256;  // four rows per workgroup
constexpr unsigned long long kPointsKeyInf = 0x7ff0000000000000ull;  // the bits of +inf; also the largest key (DBL_MAX)

struct PointsCandidatesArgs {
    PointsView x, y;
    long long N, M;
    int B, D, K;
    const int *shapes;      // [B][2] or null: the caller's device array
    const double *limit;    // null (no limit), [B] (limit_ld == 0) or [B][limit_ld]
    long long limit_ld;
    int *cols;              // [B][N][K]
    double *vals;           // [B][N][K]
    int *counts;            // [B][N]
    int *rows;              // [B]
};

// The limit of a row as a key: the largest key a candidate may have.  The value's bits as an integer (for the reason
// given at points_coord_bad), under the IEEE comparison "cost <= limit" for costs >= +0.0: +0.0 .. +inf admit the costs
// up to themselves, -0.0 admits +0.0, a negative value and every NaN admit no finite cost (key 0 stays: a cost that is
// not finite is always a candidate).
__device__ __forceinline__ unsigned long long points_limit_key(const double *p) {
    if (!p) return kPointsKeyInf;  // every finite cost
    unsigned long long u;
    __builtin_memcpy(&u, p, sizeof u);
    if (u > kPointsKeyInf) return u == 0x8000000000000000ull ? 1ull : 0ull;
    return u == kPointsKeyInf ? kPointsKeyInf : u + 1ull;
}

// The key of column point p for the row whose widened coordinates are xi (xbad: one of them is a NaN or infinite)
template <class T>
__device__ __forceinline__ unsigned long long points_candidate_key(const double (&xi)[kPointsBatchMaxCoords], bool xbad,
                                                                   const T *p, long long sD, int D) {
    bool bad = xbad;
#pragma unroll
    for (int k = 0; k < kPointsBatchMaxCoords; ++k)
        if (k < D) bad |= points_coord_bad(p + (size_t)k * (size_t)sD);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(points_cost(xi, p, sD, D));
    return bad || bits >= kPointsKeyInf ? 0ull : bits + 1ull;
}

__device__ __forceinline__ double points_candidate_value(unsigned long long key) {
    return __longlong_as_double((long long)(key ? key - 1ull : kPointsKeyInf));
}

// The streaming pass of one row: the candidates of columns 0 .. m - 1 into slots 0 .. K - 1 in column order; returns their
// number.  D is a compile-time constant here (the kernel's uniform switch): with the run-time D every load of a
// coordinate sits in a basic block of its own behind a scalar branch on k < D and is waited for at once -- 2 D dependent
// latencies per step -- while with the constant the loads of a step are issued back to back (DESIGN 4.29 found the same
// in the finish's scan).
template <class T, int D>
__device__ __forceinline__ int points_candidates_stream(const double (&xi)[kPointsBatchMaxCoords], bool xbad, const T *Y,
                                                        long long yP, long long yD, int m, unsigned long long lim, int K,
                                                        int *cols, double *vals) {
    const int lane = lane_id();
    const unsigned long long below_me = lanemask_lt();
    int count = 0;
    for (int c0 = 0; c0 < m; c0 += kWave) {
        const int c = c0 + lane;
        unsigned long long key = ~0ull;  // (beyond m: no candidate under any limit)
        if (c < m) key = points_candidate_key(xi, xbad, Y + (size_t)c * (size_t)yP, yD, D);
        const bool cand = key <= lim;
        const unsigned long long mask = __ballot(cand);
        const int slot = count + (int)__popcll(mask & below_me);
        if (cand && slot < K) {
            cols[slot] = c;
            vals[slot] = points_candidate_value(key);
        }
        count += (int)__popcll(mask);
    }
    return count;
}

// The truncated path of one row with more than K candidates: the K smallest by (key, column) into the K slots, in
// column order.  The run-time D: this path is rare, and eight copies of its three loops are not worth their code.
template <class T>
__device__ __forceinline__ void points_candidates_truncate(const double (&xi)[kPointsBatchMaxCoords], bool xbad, const T *Y,
                                                           long long yP, long long yD, int D, int m,
                                                           unsigned long long lim, int K, int *cols, double *vals) {
    const int lane = lane_id();
    const unsigned long long below_me = lanemask_lt();
    // T = the smallest key with at least K candidates at or below it; `under` = how many lie below T.
    // Invariant: at least K candidates have key <= hi, and `under` < K have key < lo.
    unsigned long long lo = 0, hi = lim;
    int under = 0, ties = 0;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        int le = 0;
        for (int c0 = 0; c0 < m; c0 += kWave) {
            const int c = c0 + lane;
            unsigned long long key = ~0ull;
            if (c < m) key = points_candidate_key(xi, xbad, Y + (size_t)c * (size_t)yP, yD, D);
            le += (int)__popcll(__ballot(key <= mid));
        }
        if (le == K) {  // exactly the K smallest: every candidate at or below mid is kept
            lo = mid;
            ties = K;
            break;
        }
        if (le > K) {
            hi = mid;
        } else {
            lo = mid + 1ull;
            under = le;
        }
    }
    if (!ties) ties = K - under;
    // (the streaming pass wrote some of these slots from other lanes: its stores are complete first)
    __threadfence();
    int base = 0, seen = 0;  // slots filled; candidates at T passed
    for (int c0 = 0; c0 < m; c0 += kWave) {
        const int c = c0 + lane;
        unsigned long long key = ~0ull;
        if (c < m) key = points_candidate_key(xi, xbad, Y + (size_t)c * (size_t)yP, yD, D);
        const bool at = key == lo;
        const unsigned long long atmask = __ballot(at);
        const bool keep = key < lo || (at && seen + (int)__popcll(atmask & below_me) < ties);
        const unsigned long long mask = __ballot(keep);
        const int slot = base + (int)__popcll(mask & below_me);
        if (keep && slot < K) {
            cols[slot] = c;
            vals[slot] = points_candidate_value(key);
        }
        base += (int)__popcll(mask);
        seen += (int)__popcll(atmask);
    }
}

template <class T>
__global__ __launch_bounds__(kPointsCandidatesThreads) void k_points_candidates(PointsCandidatesArgs a) {
    const int lane = lane_id(), D = a.D, K = a.K, N = (int)a.N, M = (int)a.M;
    const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kPointsCandidatesThreads / kWave) + ((int)threadIdx.x >> 6));
    for (long long bb = blockIdx.y; bb < (long long)a.B; bb += gridDim.y) {
        const int b = (int)bb;
        int n, m;
        dense_batch_shape(a.shapes, N, M, b, n, m);
        if (n < 1 || n > N || m < 1 || m > M) n = m = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) a.rows[b] = n;
        if (i >= N) continue;
        const size_t row = (size_t)b * (size_t)N + (size_t)i;
        int *cols = a.cols + row * (size_t)K;
        double *vals = a.vals + row * (size_t)K;
        int count = 0;
        if (i < n) {
            const T *X = static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB + (size_t)i * (size_t)a.x.sP;
            const T *Y = static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB;
            const long long yP = a.y.sP, yD = a.y.sD;
            bool xbad = false;
            for (int k = 0; k < D; ++k) xbad |= points_coord_bad(X + (size_t)k * (size_t)a.x.sD);
            double xi[kPointsBatchMaxCoords];
            points_load(X, a.x.sD, D, xi);
            const unsigned long long lim =
                points_limit_key(a.limit ? a.limit + (a.limit_ld ? (size_t)b * (size_t)a.limit_ld + (size_t)i : (size_t)b) : nullptr);
            switch (D) {  // (uniform)
            case 1: count = points_candidates_stream<T, 1>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 2: count = points_candidates_stream<T, 2>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 3: count = points_candidates_stream<T, 3>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 4: count = points_candidates_stream<T, 4>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 5: count = points_candidates_stream<T, 5>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 6: count = points_candidates_stream<T, 6>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 7: count = points_candidates_stream<T, 7>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            default: count = points_candidates_stream<T, 8>(xi, xbad, Y, yP, yD, m, lim, K, cols, vals); break;
            }
            if (count > K) points_candidates_truncate(xi, xbad, Y, yP, yD, D, m, lim, K, cols, vals);  // (uniform)
        }
        for (int s = (count < K ? count : K) + lane; s < K; s += kWave) {
            cols[s] = -1;
            vals[s] = 0.0;
        }
        if (lane == 0) a.counts[row] = count;
    }
}

}  // namespace misslap
