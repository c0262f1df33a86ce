// kernels_points_whiten.hpp -- the points batch with a whitening matrix per row: the Mahalanobis cost
//     c[b][i][j] = | W[b][i] (x[b][i] - y[b][j]) |^2,   W[b][i] lower triangular, D x D
// for the check pass, the solve and the candidate builder of the points batch (misslap_solve_points_batch_whitened,
// misslap_points_batch_candidates_whitened, include/misslap.h; the host side is abi_points_whiten.hpp behind the shared
// call paths of abi_points_batch.hpp and abi_points_candidates.hpp).  Everything that does not form a cost is shared
// with the plain kernels (kernels_points_batch.hpp, kernels_points_candidates.hpp), which are not touched: the kernels
// here are instances of their own, so a call without a matrix runs exactly the code it ran before.
//
// The cost is the chain of sslap_amd.points_to_dense(whiten=) on the coordinates and the matrix widened to double
// (exact):
//     d_l = x_l - y_l                                                        l = 0 .. D - 1
//     z_k = W[k][0] * d_0;  z_k = z_k + W[k][l] * d_l  for l = 1 .. k         k = 0 .. D - 1
//     s_0 = z_0 * z_0;      s_k = s_(k-1) + z_k * z_k;                        c = s_(D-1)
// D^2 + 3 D - 1 separately rounded double operations in this order (-ffp-contract=off: nothing is fused).  A sum of
// squares is never negative and never -0.0, so every finite cost is an entry under the dense rule, as in the plain call.
// D = 1 .. MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS (4): a row's triangle is 10 doubles, which bid() holds next to the
// row's 4 coordinates -- in scalar registers, the row index being uniform -- under the 128 registers of a 1024-thread
// workgroup.  Only W[b][i][k][l] with l <= k < D and i < n_b is ever read: the upper triangle and the rows beyond the
// shape may hold anything.  W is a view: element (k, l) of row i of problem b lies at w[b * sB + i * sN + k * sK + l * sL]
// for element strides >= 0 (sN = 0: one matrix per problem; sB = sN = 0: one for the call).
//
// What is not finite (the build has -fno-honor-nans): every coordinate and every matrix element that is
// read is classified by an integer load of its bits (points_coord_bad).  With finite inputs the chain can still leave
// the finite numbers, and unlike the plain chain it can produce a NaN: two products overflow to +inf and -inf and their
// sum is a NaN, which a test of the cost's bits (folded into |c| == inf) does not see.  In evaluation order the first
// intermediate that is not finite is always an infinity, never a NaN, so the check pass and the builder's key carry a
// flag over every d_l, every product and every partial z tested as |v| == inf, a compare the folding leaves alone;
// z * z and the sum of squares only overflow to +inf, which the test of the cost's bits catches.  The solve's own
// scans run on problems with status 0 and need no flag.
#pragma once

namespace misslap {

constexpr int kPointsWhitenMaxCoords = MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS;
constexpr int kPointsWhitenTri = kPointsWhitenMaxCoords * (kPointsWhitenMaxCoords + 1) / 2;
static_assert(kPointsWhitenMaxCoords <= kPointsBatchMaxCoords, "a whitened call is a points call");

// one row, widened: its coordinates x[k], k < D, and its triangle w[k (k + 1) / 2 + l], l <= k < D; the rest is never read
struct WhitenRow {
    double x[kPointsWhitenMaxCoords];
    double w[kPointsWhitenTri];
};

template <class T>
__device__ __forceinline__ void whiten_load(const T *xp, long long xD, const T *wp, long long sK, long long sL, int D,
                                            WhitenRow &r) {
#pragma unroll
    for (int k = 0; k < kPointsWhitenMaxCoords; ++k)
        if (k < D) {
            r.x[k] = dense_widen(xp[(size_t)k * (size_t)xD]);
#pragma unroll
            for (int l = 0; l <= k; ++l)
                r.w[k * (k + 1) / 2 + l] = dense_widen(wp[(size_t)k * (size_t)sK + (size_t)l * (size_t)sL]);
        }
}

// Whether an element of the triangle of the row at wp is a NaN or an infinity: integer loads (points_coord_bad)
template <class T>
__device__ __forceinline__ bool whiten_row_bad(const T *wp, long long sK, long long sL, int D) {
    bool bad = false;
    for (int k = 0; k < D; ++k)
        for (int l = 0; l <= k; ++l) bad |= points_coord_bad(wp + (size_t)k * (size_t)sK + (size_t)l * (size_t)sL);
    return bad;
}

template <bool Flag>
__device__ __forceinline__ void whiten_mark(double v, bool &inf) {
    if constexpr (Flag) inf |= __builtin_fabs(v) == __builtin_huge_val();
}

// The cost of (row r, the point at p): the definition's chain.  Flag: `inf` also gathers |v| == inf over every
// difference, product and partial z.
template <class T, bool Flag>
__device__ __forceinline__ double whiten_cost_as(const WhitenRow &r, const T *p, long long sD, int D, bool &inf) {
    double d[kPointsWhitenMaxCoords];
#pragma unroll
    for (int k = 0; k < kPointsWhitenMaxCoords; ++k)
        if (k < D) {
            d[k] = r.x[k] - dense_widen(p[(size_t)k * (size_t)sD]);
            whiten_mark<Flag>(d[k], inf);
        }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kPointsWhitenMaxCoords; ++k)
        if (k < D) {
            double z = r.w[k * (k + 1) / 2] * d[0];
            whiten_mark<Flag>(z, inf);
#pragma unroll
            for (int l = 1; l <= k; ++l) {
                const double q = r.w[k * (k + 1) / 2 + l] * d[l];
                whiten_mark<Flag>(q, inf);
                z = z + q;
                whiten_mark<Flag>(z, inf);
            }
            const double q = z * z;
            s = k == 0 ? q : s + q;
        }
    return s;
}
template <class T>
__device__ __forceinline__ double whiten_cost(const WhitenRow &r, const T *p, long long sD, int D) {
    bool unused = false;
    return whiten_cost_as<T, false>(r, p, sD, D, unused);
}

struct PointsWhitenCheckArgs {
    PointsCheckArgs c;
    WhitenView w;
};

// The check pass of a whitened call: k_points_batch_check with the whitened cost.  The non-finite flag has three parts:
// (1) the exponent bits of every coordinate inside the shape and of the triangle of every row < n_b, loaded as integers;
// (2) |v| == inf over the chain's differences, products and partial sums (see the head of this file); (3) the cost's
// own bits, for the overflow of a square or of their sum to +inf.
template <class T, bool Out>
__global__ __launch_bounds__(256) void k_points_whiten_check(PointsWhitenCheckArgs wa) {
    const PointsCheckArgs &a = wa.c;
    const long long N = a.N, M = a.M;
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6, D = a.D;
    int n, m;
    dense_batch_shape(a.shapes, N, M, b, n, m);
    if (n < 1 || n > N || m < 1 || m > M) n = m = 0;
    if (threadIdx.x == 0) {
        a.shapes_out[2 * b] = n;
        a.shapes_out[2 * b + 1] = m;
    }
    __shared__ unsigned long long s_abs;
    __shared__ int s_flags, s_badp;
    if (threadIdx.x == 0) {
        s_abs = 0;
        s_flags = 0;
        s_badp = 0;
    }
    __syncthreads();
    const T *X = static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB;
    const T *Y = static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB;
    const T *W = static_cast<const T *>(wa.w.p) + (size_t)b * (size_t)wa.w.sB;
    unsigned long long am = 0;
    int flags = 0;
    // (1) the coordinates of the n and the m points inside the shape, and the triangles of the n rows
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const T *p = X + (size_t)i * (size_t)a.x.sP;
        for (int k = 0; k < D; ++k) flags |= points_coord_bad(p + (size_t)k * (size_t)a.x.sD) ? 1 : 0;
        flags |= whiten_row_bad(W + (size_t)i * (size_t)wa.w.sN, wa.w.sK, wa.w.sL, D) ? 1 : 0;
    }
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        const T *p = Y + (size_t)j * (size_t)a.y.sP;
        for (int k = 0; k < D; ++k) flags |= points_coord_bad(p + (size_t)k * (size_t)a.y.sD) ? 1 : 0;
    }
    // (2), (3) the costs: the maximum, an infinity inside the chain, and +inf by overflow
    for (int r = wave; r < n; r += nw) {
        WhitenRow row;
        whiten_load(X + (size_t)r * (size_t)a.x.sP, a.x.sD, W + (size_t)r * (size_t)wa.w.sN, wa.w.sK, wa.w.sL, D, row);
        for (int c = lane; c < m; c += kWave) {
            bool inf = false;
            const double cost = whiten_cost_as<T, true>(row, Y + (size_t)c * (size_t)a.y.sP, a.y.sD, D, inf);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(cost) & 0x7fffffffffffffffull;
            if (inf || (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) flags |= 1;
            else am = bits > am ? bits : am;
        }
        if constexpr (Out) {
            if (lane == 0) {
                // (the value's bits as an integer; the dense rule "v >= 0" on them, as in k_points_batch_check)
                unsigned long long u;
                __builtin_memcpy(&u, a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld + (size_t)r : (size_t)b),
                                 sizeof u);
                if (u <= 0x7ff0000000000000ull || u == 0x8000000000000000ull) {
                    const unsigned long long bits = u & 0x7fffffffffffffffull;
                    am = bits > am ? bits : am;
                    flags |= bits == 0x7ff0000000000000ull ? 1 : 0;
                } else {
                    flags |= 2;
                }
            }
        }
    }
    if (am) atomicMax(&s_abs, am);
    if (flags) atomicOr(&s_flags, flags);
    if (a.p0) batch_check_prices(a.p0 + (size_t)b * (size_t)M, m, &s_badp);
    if constexpr (Out) {
        if (a.p0) {
            const double *src = a.p0 + (size_t)b * (size_t)M;
            double *dst = a.aug + (size_t)b * (size_t)(M + N);
            for (int j = threadIdx.x; j < m + n; j += blockDim.x) dst[j] = j < m ? src[j] : 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        PointsBatchCheck r;
        r.absmax_bits = s_abs;
        r.flags = s_flags;
        r.bad_price = s_badp;
        a.out[b] = r;
    }
}

// The whitened row source of batch_solve: PointBatchRows with the whitened cost.  bid and ece_bad run one wavefront per
// row, so the row's coordinates and triangle come from addresses that are uniform over the wavefront; gather runs one
// thread per row.  The order of every scan, the tie rule and the outside entry are PointBatchRows'.
template <class T, bool Out>
struct WhitenBatchRows {
    const T *X, *Y, *W;
    long long xP, xD, yP, yD, wN, wK, wL;  // element strides
    int D, n, m, maximize;
    BatchOutside<Out> out;

    __device__ __forceinline__ const T *yp(int c) const { return Y + (size_t)c * (size_t)yP; }
    __device__ __forceinline__ void load(int i, WhitenRow &r) const {
        whiten_load(X + (size_t)i * (size_t)xP, xD, W + (size_t)i * (size_t)wN, wK, wL, D, r);
    }

    __device__ __forceinline__ void take(Top2 &x, double &cb, double v, int c, const double *price) const {
        const double cost = maximize ? v : v * -1.0;  // :236-237
        const double vi = cost - price[c];
        if (top2_take(x, vi, c)) cb = cost;
    }

    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        i = __builtin_amdgcn_readfirstlane(i);  // (uniform already: the row may live in scalar registers)
        WhitenRow r;
        load(i, r);
        Top2 x;
        x.v = -__builtin_huge_val();
        x.w = -__builtin_huge_val();
        x.g = -1;
        double cb = 0.0;
        for (int c = lane; c < m; c += kWave) take(x, cb, whiten_cost(r, yp(c), yD, D), c, price);
        if constexpr (Out) {
            if (lane == ((m + i) & (kWave - 1))) take(x, cb, out.value(i), m + i, price);
        }
        const Top2 t = top2_wave_reduce(x);
        costbest = readlane_f64(cb, t.g & (kWave - 1));  // the lane that holds column t.g
        obj = t.g;
        return t;
    }

    // eCE_satisfied (auction_.pyx:443-485) for row i: choice_cost is the cost of column j, every column is tested
    __device__ __forceinline__ bool ece_bad(int i, int j, const double *price, double tol, double eps) const {
        i = __builtin_amdgcn_readfirstlane(i);  // (one wavefront per row)
        WhitenRow r;
        load(i, r);
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : whiten_cost(r, yp(j), yD, D);
        else vj = whiten_cost(r, yp(j), yD, D);
        const double choice_cost = maximize ? vj : vj * -1.0;
        const double LHS = choice_cost - price[j] + tol;  // :475
        bool bad = false;
        if constexpr (Out) {
            if (lane_id() == 0) {
                const double v = out.value(i);
                const double cost = maximize ? v : v * -1.0;
                if (LHS < (cost - price[m + i]) - eps) bad = true;
            }
        }
        for (int c = lane_id(); c < m; c += kWave) {
            const double v = whiten_cost(r, yp(c), yD, D);
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[c]) - eps) bad = true;  // :482
        }
        return bad;
    }

    // get_obj (:489-523): one thread per row recomputes its chosen cost
    __device__ __forceinline__ void gather(const int *p2o, int n_, double *selv, int *) const {
        for (int i = threadIdx.x; i < n_; i += blockDim.x) {
            const int j = p2o[i];
            if constexpr (Out) {
                if (j >= m) {  // the row's outside entry
                    selv[i] = out.value(i);
                    continue;
                }
            }
            double v = 0.0;
            if (j >= 0) {
                WhitenRow r;
                load(i, r);
                v = whiten_cost(r, yp(j), yD, D);
            }
            selv[i] = v;
        }
    }

    // a double sum in row order
    __device__ __forceinline__ double objective(const int *p2o, int n_, const double *selv, const int *) const {
        double obj = 0;
        for (int i = 0; i < n_; ++i) {
            if (p2o[i] == -1) continue;
            const double val = maximize ? selv[i] : selv[i] * -1.0;
            if (maximize) obj += val;
            else obj -= val;
        }
        return obj;
    }

    __device__ __forceinline__ int meta_cols(int m_) const { return m_; }
    __device__ __forceinline__ int64_t meta_nnz() const { return (int64_t)n * (int64_t)m + (Out ? (int64_t)n : 0); }
};

struct PointsWhitenArgs {
    PointsBatchArgs a;
    WhitenView w;
};

// The solve of a whitened call: k_points_batch_solve on the whitened row source.
template <class T, bool Out>
__global__ __launch_bounds__(1024) void k_points_whiten_solve(PointsWhitenArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const PointsBatchArgs &a = wa.a;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = a.shapes[2 * b], m = a.shapes[2 * b + 1];
    const PointsBatchCheck ck = a.chk[b];
    const int code = batch_verdict(points_batch_verdict<Out>(ck, n, m), false, -1, n, ck.bad_price);
    batch_publish_verdict(a.status, a.matching_size, b, code, Out || n < 1 ? -1 : (n < m ? n : m));
    const int N = (int)a.N, M = (int)a.M;
    const int mo = Out ? m + n : m;
    double *po = nullptr, *oo = nullptr;
    if constexpr (Out) {
        po = a.prices ? a.prices + (size_t)b * (size_t)M : nullptr;
        oo = a.outside_prices ? a.outside_prices + (size_t)b * (size_t)N : nullptr;
    }
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(a.s, n, mo, (long long)n * (long long)m + (Out ? n : 0));
        if constexpr (Out) batch_outside_condemn(po, M, oo, N, tid, nt);
        return;
    }
    BatchSolveArgs s = a.s;
    if (a.fast) batch_fast_eps(s, n);
    BatchOutside<Out> out;
    if constexpr (Out) {
        out.O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
        out.stride = a.outside_ld ? 1 : 0;
    }
    const WhitenBatchRows<T, Out> rows{static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB,
                                       static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB,
                                       static_cast<const T *>(wa.w.p) + (size_t)b * (size_t)wa.w.sB,
                                       a.x.sP, a.x.sD, a.y.sP, a.y.sD, wa.w.sN, wa.w.sK, wa.w.sL,
                                       a.D, n, m, s.maximize, out};
    batch_solve(s, rows, n, mo, ck.absmax_bits);
    if constexpr (Out) batch_outside_outputs(s_raw, a.s, b, n, m, M, N, po, oo, tid, nt);
}

// ---- the candidate builder (kernels_points_candidates.hpp) on the whitened cost.  The key, the limit key, the stored
// value, the streaming pass and the truncated path are that file's, restated on whiten_candidate_key.

// The key of column point p for row r (rbad: a coordinate or a matrix element of the row is a NaN or infinite)
template <class T, int D>
__device__ __forceinline__ unsigned long long whiten_candidate_key(const WhitenRow &r, bool rbad, const T *p, long long sD) {
    bool bad = rbad;
#pragma unroll
    for (int k = 0; k < D; ++k) bad |= points_coord_bad(p + (size_t)k * (size_t)sD);
    bool inf = false;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(whiten_cost_as<T, true>(r, p, sD, D, inf));
    return bad || inf || bits >= kPointsKeyInf ? 0ull : bits + 1ull;
}

// One row of the builder with the compile-time D (the loads of a step issue back to back): the
// streaming pass, and where it counted more than K candidates the truncated path; returns the count.
template <class T, int D>
__device__ __forceinline__ int whiten_candidates_row(const WhitenRow &r, bool rbad, const T *Y, long long yP, long long yD,
                                                     int m, unsigned long long lim, int K, int *cols, double *vals) {
    const int lane = lane_id();
    const unsigned long long below_me = lanemask_lt();
    int count = 0;
    for (int c0 = 0; c0 < m; c0 += kWave) {
        const int c = c0 + lane;
        unsigned long long key = ~0ull;  // (beyond m: no candidate under any limit)
        if (c < m) key = whiten_candidate_key<T, D>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
        const bool cand = key <= lim;
        const unsigned long long mask = __ballot(cand);
        const int slot = count + (int)__popcll(mask & below_me);
        if (cand && slot < K) {
            cols[slot] = c;
            vals[slot] = points_candidate_value(key);
        }
        count += (int)__popcll(mask);
    }
    if (count <= K) return count;  // (uniform)
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
            if (c < m) key = whiten_candidate_key<T, D>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
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
        if (c < m) key = whiten_candidate_key<T, D>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
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
    return count;
}

struct PointsWhitenCandidatesArgs {
    PointsCandidatesArgs c;
    WhitenView w;
};

template <class T>
__global__ __launch_bounds__(kPointsCandidatesThreads) void k_points_whiten_candidates(PointsWhitenCandidatesArgs wa) {
    const PointsCandidatesArgs &a = wa.c;
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
            const T *W = static_cast<const T *>(wa.w.p) + (size_t)b * (size_t)wa.w.sB + (size_t)i * (size_t)wa.w.sN;
            const long long yP = a.y.sP, yD = a.y.sD;
            bool rbad = whiten_row_bad(W, wa.w.sK, wa.w.sL, D);
            for (int k = 0; k < D; ++k) rbad |= points_coord_bad(X + (size_t)k * (size_t)a.x.sD);
            WhitenRow r;
            whiten_load(X, a.x.sD, W, wa.w.sK, wa.w.sL, D, r);
            const unsigned long long lim =
                points_limit_key(a.limit ? a.limit + (a.limit_ld ? (size_t)b * (size_t)a.limit_ld + (size_t)i : (size_t)b) : nullptr);
            switch (D) {  // (uniform)
            case 1: count = whiten_candidates_row<T, 1>(r, rbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 2: count = whiten_candidates_row<T, 2>(r, rbad, Y, yP, yD, m, lim, K, cols, vals); break;
            case 3: count = whiten_candidates_row<T, 3>(r, rbad, Y, yP, yD, m, lim, K, cols, vals); break;
            default: count = whiten_candidates_row<T, 4>(r, rbad, Y, yP, yD, m, lim, K, cols, vals); break;
            }
        }
        for (int s = (count < K ? count : K) + lane; s < K; s += kWave) {
            cols[s] = -1;
            vals[s] = 0.0;
        }
        if (lane == 0) a.counts[row] = count;
    }
}

}  // namespace misslap
