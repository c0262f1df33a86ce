// kernels_points_batch.hpp -- many small dense problems whose costs are squared distances between two point sets,
// c[b][i][j] = |x[b][i] - y[b][j]|^2, one workgroup per problem for its whole solve (misslap_solve_points_batch,
// include/misslap.h; the host side is abi_points_batch.hpp).  The cost stack is never stored: the third row source of
// batch_solve (kernels_batch_solve.hpp) forms every cost it needs from the coordinates, in registers.
//
// The cost, wherever one is needed -- the bid, the eCE test, the objective's gather, the check pass's maximum -- is the
// chain of sslap_amd.points_to_dense on the coordinates widened to double (exact):
//     d_k = x_k - y_k,  s_0 = d_0 * d_0,  s_k = s_(k-1) + d_k * d_k,  c = s_(D-1)
// 3 D - 1 separately rounded double operations in this order (the library is built with -ffp-contract=off: nothing is
// fused).  A square is never negative and never -0.0, so every finite cost is an entry under the dense rule "v >= 0":
// the problem is the dense problem on that stack with n_b * m_b entries and m_b columns, and its result is the dense
// call's bit for bit.  A cost that is not finite (a NaN or an infinite coordinate, an overflow) condemns the problem in
// the check pass, so the round loop only ever sees finite costs.
//
// Coordinate type T (double, float: misslap_options.mat_dtype); D = 1 .. MISSLAP_POINTS_BATCH_MAX_COORDS is a run-time
// bound of fully unrolled loops, so there is one instance per (T, Out).  Both point sets are views: coordinate k of
// point i of problem b lies at p[b * sB + i * sP + k * sD] for element strides >= 0 (the host has checked that the
// extent fits 62 bits); loads are one element each and only elements of the view are read.  y is read through L1 / L2
// in every round: at most 2048 points x 8 coordinates x 8 bytes = 128 KB per problem, and the LDS carve of batch_solve
// at 2048 x 2048 with outside (155 648 bytes) leaves no room to stage it.
//
// Outside mode Out: as in kernels_dense_batch.hpp -- row i also holds the virtual entry (i, m_b + i) with the row's
// outside value, the carve has M + N objects, and the outputs are rewritten behind batch_solve.
#pragma once

namespace misslap {

constexpr int kPointsBatchMaxDim = MISSLAP_POINTS_BATCH_MAX_DIM;
constexpr int kPointsBatchMaxCoords = MISSLAP_POINTS_BATCH_MAX_COORDS;

// one point set of a call: its first element and the element strides of problem, point and coordinate
struct PointsView {
    const void *p;
    long long sB, sP, sD;
};

// the whitening matrices of a call (kernels_points_whiten.hpp): the first element and the element strides of problem,
// row, matrix row and matrix column; p null: the call has none
struct WhitenView {
    const void *p;
    long long sB, sN, sK, sL;
};

// per problem, from the check pass
struct PointsBatchCheck {
    unsigned long long absmax_bits;  // the largest cost (and outside value of a row < n), as bits
    int flags;                       // bit 0: a cost is not finite, or the outside value of a row < n is +inf;
                                     // bit 1 (outside mode): the outside value of a row < n is negative or a NaN;
                                     // bit 2 (kernels_boxes_batch.hpp only): a box inside the shape is a bad box
    int bad_price;                   // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
};

// The D coordinates of one point, widened: x[k] for k < D, the rest is never read
template <class T>
__device__ __forceinline__ void points_load(const T *p, long long sD, int D, double (&x)[kPointsBatchMaxCoords]) {
#pragma unroll
    for (int k = 0; k < kPointsBatchMaxCoords; ++k)
        if (k < D) x[k] = dense_widen(p[(size_t)k * (size_t)sD]);
}

// The cost of (x, the point at p): the definition's chain
template <class T>
__device__ __forceinline__ double points_cost(const double (&x)[kPointsBatchMaxCoords], const T *p, long long sD, int D) {
    const double d0 = x[0] - dense_widen(p[0]);
    double s = d0 * d0;
#pragma unroll
    for (int k = 1; k < kPointsBatchMaxCoords; ++k)
        if (k < D) {
            const double d = x[k] - dense_widen(p[(size_t)k * (size_t)sD]);
            const double q = d * d;
            s = s + q;
        }
    return s;
}

// Whether the coordinate at p is a NaN or an infinity: its exponent bits, loaded as an integer.  (It must never exist as
// a floating-point value here: the build has -fno-honor-nans, and the same test on the bits OF a double or a float is
// turned into |v| == inf, which a NaN fails.)
__device__ __forceinline__ bool points_coord_bad(const double *p) {
    unsigned long long u;
    __builtin_memcpy(&u, p, sizeof u);
    return (u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}
__device__ __forceinline__ bool points_coord_bad(const float *p) {
    unsigned u;
    __builtin_memcpy(&u, p, sizeof u);
    return (u & 0x7f800000u) == 0x7f800000u;
}

struct PointsCheckArgs {
    PointsView x, y;
    long long N, M;
    int D;
    const int *shapes;      // [B][2] or null: the caller's, possibly a device array that no host has seen
    const double *p0;       // [B][M] or null
    PointsBatchCheck *out;  // [B]
    int *shapes_out;        // [B][2]: the sanitised shapes, which the solve reads
    const double *outside;  // [B] (outside_ld == 0) or [B][outside_ld]; read when Out
    long long outside_ld;
    double *aug;            // [B][M + N] or null (Out with starting prices: [p0[:m_b], zeros(n_b)])
};

// The check pass, one workgroup per problem: the shape every later kernel uses (one outside 1 .. N x 1 .. M becomes
// (0, 0) and nothing of that problem is read), C = the largest cost as bits, the non-finite flag, the outside values
// under the dense rule, the starting prices, and with Out the staged augmented prices.
// The non-finite flag has two parts, because the build has -fno-honor-nans: the result of an arithmetic operation is
// assumed not to be a NaN, and the compiler turns a test of a COST's exponent bits into |c| == inf, which a NaN fails.
// (1) The exponent bits of every coordinate inside the shape, loaded as integers (points_coord_bad): a NaN or an
// infinite coordinate makes every cost it enters a NaN or an infinity.  (2) With finite coordinates a cost is
// finite or, by overflow, +inf -- a difference overflows to an infinity, a square and a sum of squares to +inf, and
// nothing subtracts two infinities -- and +inf is what the folded test still catches.
template <class T, bool Out>
__global__ __launch_bounds__(256) void k_points_batch_check(PointsCheckArgs a) {
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
    unsigned long long am = 0;
    int flags = 0;
    // (1) the coordinates of the n and the m points inside the shape
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const T *p = X + (size_t)i * (size_t)a.x.sP;
        for (int k = 0; k < D; ++k) flags |= points_coord_bad(p + (size_t)k * (size_t)a.x.sD) ? 1 : 0;
    }
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        const T *p = Y + (size_t)j * (size_t)a.y.sP;
        for (int k = 0; k < D; ++k) flags |= points_coord_bad(p + (size_t)k * (size_t)a.y.sD) ? 1 : 0;
    }
    // (2) the costs: the maximum, and +inf by overflow
    for (int r = wave; r < n; r += nw) {
        double xi[kPointsBatchMaxCoords];
        points_load(X + (size_t)r * (size_t)a.x.sP, a.x.sD, D, xi);
        for (int c = lane; c < m; c += kWave) {
            const double cost = points_cost(xi, Y + (size_t)c * (size_t)a.y.sP, a.y.sD, D);
            const unsigned long long bits = (unsigned long long)__double_as_longlong(cost) & 0x7fffffffffffffffull;
            if ((bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) flags |= 1;
            else am = bits > am ? bits : am;
        }
        if constexpr (Out) {
            if (lane == 0) {
                // (the value's bits as an integer, for the reason given at points_coord_bad; the dense rule "v >= 0" on
                // them: +0 .. +inf and -0.0 are entries, a negative value and every NaN are not)
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

// The points row source of batch_solve: problem b's n x m costs between X[i] and Y[c].
//   BID      one wavefront per list position.  The D coordinates of x_i are loaded once, from an address that is uniform
//            over the wavefront; lane l takes columns l, l + 64, ... in ascending order, loads y_c, forms the cost and
//            feeds top2_take under the reference's ">=" rule with the tie key c, as DenseBatchRows::take does.
//   eCE      every column is an entry; choice_cost is the cost of the row's own column.
//   get_obj  one thread per row recomputes the chosen cost into LDS, then one lane adds them in row order.
// Out: lane (m + i) & 63 takes the virtual entry (i, m + i) AFTER its own real columns, as the dense row source does, so
// every lane scans in ascending column order and the winner's lane is r.g & 63.
template <class T, bool Out>
struct PointBatchRows {
    const T *X, *Y;
    long long xP, xD, yP, yD;  // element strides of point and coordinate
    int D, n, m, maximize;
    BatchOutside<Out> out;

    __device__ __forceinline__ const T *xp(int i) const { return X + (size_t)i * (size_t)xP; }
    __device__ __forceinline__ const T *yp(int c) const { return Y + (size_t)c * (size_t)yP; }

    // one candidate of a scan: value v of object c, against the best two so far
    __device__ __forceinline__ void take(Top2 &x, double &cb, double v, int c, const double *price) const {
        const double cost = maximize ? v : v * -1.0;  // :236-237
        const double vi = cost - price[c];
        if (top2_take(x, vi, c)) cb = cost;
    }

    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        i = __builtin_amdgcn_readfirstlane(i);  // (uniform already: the row's coordinates may live in scalar registers)
        double xi[kPointsBatchMaxCoords];
        points_load(xp(i), xD, D, xi);
        Top2 x;
        x.v = -__builtin_huge_val();
        x.w = -__builtin_huge_val();
        x.g = -1;
        double cb = 0.0;
        // One column per step.  Two forms with two columns in flight were tried and dropped: "#pragma unroll 2" takes all
        // 128 registers of a 1024-thread workgroup and spills to scratch; requesting the next column's coordinates by
        // hand before this column's cost is formed fits (111 registers at float, 126 at double) and was measured 3 % to
        // 16 % SLOWER at every size of tools/points_batch.py.
        for (int c = lane; c < m; c += kWave) take(x, cb, points_cost(xi, yp(c), yD, D), c, price);
        if constexpr (Out) {
            if (lane == ((m + i) & (kWave - 1))) take(x, cb, out.value(i), m + i, price);
        }
        const Top2 r = top2_wave_reduce(x);
        costbest = readlane_f64(cb, r.g & (kWave - 1));  // the lane that holds column r.g
        obj = r.g;
        return r;
    }

    // eCE_satisfied (auction_.pyx:443-485) for row i: choice_cost is the cost of column j, every column is tested
    __device__ __forceinline__ bool ece_bad(int i, int j, const double *price, double tol, double eps) const {
        double xi[kPointsBatchMaxCoords];
        points_load(xp(i), xD, D, xi);
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : points_cost(xi, yp(j), yD, D);
        else vj = points_cost(xi, yp(j), yD, D);
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
            const double v = points_cost(xi, yp(c), yD, D);
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
                double xi[kPointsBatchMaxCoords];
                points_load(xp(i), xD, D, xi);
                v = points_cost(xi, yp(j), yD, D);
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

    // (m_: batch_solve's object count, in the outside mode m + n: every column holds an entry)
    __device__ __forceinline__ int meta_cols(int m_) const { return m_; }
    __device__ __forceinline__ int64_t meta_nnz() const { return (int64_t)n * (int64_t)m + (Out ? (int64_t)n : 0); }
};

struct PointsBatchArgs {
    BatchSolveArgs s;      // plain: p0_ld = prices_ld = M, Ms = M; outside: Ms = M + N, p0 the staged prices, prices null
    PointsView x, y;
    long long N, M;
    int D;
    const int *shapes;     // [B][2] the check pass's sanitised shapes
    const PointsBatchCheck *chk;
    int fast;              // eps_start = 1 / n_b of each problem (auction_.pyx:568-569)
    int *status;           // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;    // [B] or null
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]; read when Out
    long long outside_ld;
    double *prices;          // Out: [B][M] or null, the real columns
    double *outside_prices;  // Out: [B][N] or null
};

// The checks of a verdict ahead of the starting prices, in their order.  Every pair is an edge, so the maximum matching
// of a problem is min(n, m) and n > m is infeasible without a matcher; with an outside option it is solved.
template <bool Out>
__device__ __forceinline__ int points_batch_verdict(const PointsBatchCheck &c, int n, int m) {
    if (n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (Out && (c.flags & 2)) return MISSLAP_BATCH_STATUS_BAD_OUTSIDE;
    if (c.flags & 1) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    if (!Out && n > m) return MISSLAP_BATCH_STATUS_INFEASIBLE;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve: the verdict, batch_solve on the n x m (Out: n x (m + n)) problem, and with Out the outputs in the caller's
// terms (batch_outside_outputs).  A condemned problem's workgroup writes the defined outputs and leaves before any LDS
// state exists.
template <class T, bool Out>
__global__ __launch_bounds__(1024) void k_points_batch_solve(PointsBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
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
    const PointBatchRows<T, Out> rows{static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB,
                                      static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB,
                                      a.x.sP, a.x.sD, a.y.sP, a.y.sD, a.D, n, m, s.maximize, out};
    batch_solve(s, rows, n, mo, ck.absmax_bits);
    if constexpr (Out) batch_outside_outputs(s_raw, a.s, b, n, m, M, N, po, oo, tid, nt);
}

}  // namespace misslap
