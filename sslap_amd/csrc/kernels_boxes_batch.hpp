// kernels_boxes_batch.hpp -- the batch solve from two box sets: costs 1 - IoU or 1 - GIoU of boxes (x1, y1, x2, y2),
// for the check pass, the solve and the candidate builder (misslap_solve_boxes_batch, misslap_boxes_batch_candidates,
// include/misslap.h; the host side is abi_boxes_batch.hpp behind the shared call paths of abi_points_batch.hpp and
// abi_points_candidates.hpp).  A box set is a point set of D = 4 coordinates, so the views, the argument structs, the
// workspace and everything that does not form a cost are the points call's (kernels_points_batch.hpp,
// kernels_points_candidates.hpp), which are not touched: the kernels here are instances of their own.
//
// The cost is the chain of sslap_amd.boxes_to_dense on the coordinates widened to double (exact):
//     per box   w = x2 - x1,  h = y2 - y1,  area = w * h
//     per pair  iw = min(ax2, bx2) - max(ax1, bx1);  iw = iw > 0 ? iw : 0      (ih likewise, from the y's)
//               inter = iw * ih;  s = area_a + area_b;  u = s - inter;  iou = u > 0 ? inter / u : 0
//     iou       c = 1 - iou
//     giou      cw = max(ax2, bx2) - min(ax1, bx1)  (ch likewise);  hull = cw * ch;  e = hull - u;  e = e > 0 ? e : 0
//               r = hull > 0 ? e / hull : 0;  c = 1 - (iou - r)
// every operation a separately rounded double operation in this order (-ffp-contract=off: nothing is fused; the
// division is the correctly rounded one).  min, max and the selects are exact and never see a NaN where their result is
// used (below).  For boxes with x2 >= x1 and y2 >= y1 rounding is monotone, so iw <= both widths, inter <= both areas,
// s >= 2 inter and u >= inter: iou lies in [0, 1], r in [0, 1], and c in [0, 1] (iou) or [0, 2] (giou), never negative
// and never -0.0.  Every finite cost is therefore an entry under the dense rule "v >= 0", and non-negative doubles
// order as their bit patterns, which is what the builder's keys rely on.
//
// What is not finite (the build has -fno-honor-nans): every coordinate is classified by an integer load
// of its bits (points_coord_bad) BEFORE it is used as a value.  With finite coordinates the first intermediate that is
// not finite is an infinity (a width, an area, iw or ih before the clamp, s, a hull side or the hull of float64
// boxes), never a NaN, so the check pass and the builder's key carry a flag over the intermediates tested as
// |v| == inf (box_mark, as whiten_mark does).  A box with x2 < x1 or y2 < y1 is a bad box: its comparison runs on
// values, and ranks behind the non-finite flag in the verdict, so what it gives on a NaN never decides anything.
#pragma once

namespace misslap {

constexpr int kBoxFlagBadBox = 4;  // PointsBatchCheck::flags bit 2: a box inside the shape has x2 < x1 or y2 < y1

// one box, widened, with its area
struct BoxRow {
    double x1, y1, x2, y2, area;
};

template <bool Flag>
__device__ __forceinline__ void box_mark(double v, bool &inf) {
    if constexpr (Flag) inf |= __builtin_fabs(v) == __builtin_huge_val();
}

// The box at p.  Flag: `inf` also gathers |v| == inf over its width, height and area.
template <class T, bool Flag>
__device__ __forceinline__ void box_load_as(const T *p, long long sD, BoxRow &r, bool &inf) {
    r.x1 = dense_widen(p[0]);
    r.y1 = dense_widen(p[(size_t)sD]);
    r.x2 = dense_widen(p[2 * (size_t)sD]);
    r.y2 = dense_widen(p[3 * (size_t)sD]);
    const double w = r.x2 - r.x1, h = r.y2 - r.y1;
    r.area = w * h;
    box_mark<Flag>(w, inf);
    box_mark<Flag>(h, inf);
    box_mark<Flag>(r.area, inf);
}
template <class T>
__device__ __forceinline__ void box_load(const T *p, long long sD, BoxRow &r) {
    bool unused = false;
    box_load_as<T, false>(p, sD, r, unused);
}

// Whether a coordinate of the box at p is a NaN or an infinity: integer loads (points_coord_bad)
template <class T>
__device__ __forceinline__ bool box_coords_bad(const T *p, long long sD) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) bad |= points_coord_bad(p + (size_t)k * (size_t)sD);
    return bad;
}

__device__ __forceinline__ bool box_inverted(const BoxRow &r) { return r.x2 < r.x1 || r.y2 < r.y1; }

__device__ __forceinline__ double box_min(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double box_max(double a, double b) { return a > b ? a : b; }

// The cost of (row box a, column box b): the definition's chain.  Flag: `inf` also gathers |v| == inf over the
// intermediates that can leave the finite numbers.
template <bool Giou, bool Flag>
__device__ __forceinline__ double box_cost_as(const BoxRow &a, const BoxRow &b, bool &inf) {
    double iw = box_min(a.x2, b.x2) - box_max(a.x1, b.x1);
    double ih = box_min(a.y2, b.y2) - box_max(a.y1, b.y1);
    box_mark<Flag>(iw, inf);
    box_mark<Flag>(ih, inf);
    iw = iw > 0.0 ? iw : 0.0;
    ih = ih > 0.0 ? ih : 0.0;
    const double inter = iw * ih;
    const double s = a.area + b.area;
    box_mark<Flag>(inter, inf);
    box_mark<Flag>(s, inf);
    const double u = s - inter;
    const double q = inter / u;
    const double iou = u > 0.0 ? q : 0.0;
    if constexpr (!Giou) {
        return 1.0 - iou;
    } else {
        const double cw = box_max(a.x2, b.x2) - box_min(a.x1, b.x1);
        const double ch = box_max(a.y2, b.y2) - box_min(a.y1, b.y1);
        const double hull = cw * ch;
        box_mark<Flag>(cw, inf);
        box_mark<Flag>(ch, inf);
        box_mark<Flag>(hull, inf);
        double e = hull - u;
        e = e > 0.0 ? e : 0.0;
        const double t = e / hull;
        const double r = hull > 0.0 ? t : 0.0;
        const double g = iou - r;
        return 1.0 - g;
    }
}
// ... with the column box loaded from p
template <class T, bool Giou>
__device__ __forceinline__ double box_cost(const BoxRow &a, const T *p, long long sD) {
    BoxRow b;
    box_load(p, sD, b);
    bool unused = false;
    return box_cost_as<Giou, false>(a, b, unused);
}

// The check pass of a boxes call: k_points_batch_check with the box cost and one more flag.  The flags:
// bit 0 (not finite) has three parts -- (1) the exponent bits of every coordinate inside the shape, loaded as integers;
// (2) |v| == inf over every box's width, height and area and over the chain's intermediates (see the head of this
// file); (3) the cost's own bits --, bit 1 is the outside values' under the dense rule, and bit 2 (kBoxFlagBadBox) a
// box inside the shape with x2 < x1 or y2 < y1.
template <class T, bool Out, bool Giou>
__global__ __launch_bounds__(256) void k_boxes_batch_check(PointsCheckArgs a) {
    const long long N = a.N, M = a.M;
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
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
    // (1) the coordinates of the n and the m boxes inside the shape; their widths, heights, areas and orientation
    for (int i = threadIdx.x; i < n + m; i += blockDim.x) {
        const T *p = i < n ? X + (size_t)i * (size_t)a.x.sP : Y + (size_t)(i - n) * (size_t)a.y.sP;
        const long long sD = i < n ? a.x.sD : a.y.sD;
        flags |= box_coords_bad(p, sD) ? 1 : 0;
        BoxRow r;
        bool inf = false;
        box_load_as<T, true>(p, sD, r, inf);
        flags |= inf ? 1 : 0;
        flags |= box_inverted(r) ? kBoxFlagBadBox : 0;
    }
    // (2), (3) the costs: the maximum, an infinity inside the chain, and the cost's own bits
    for (int r = wave; r < n; r += nw) {
        BoxRow row;
        box_load(X + (size_t)r * (size_t)a.x.sP, a.x.sD, row);
        for (int c = lane; c < m; c += kWave) {
            BoxRow col;
            box_load(Y + (size_t)c * (size_t)a.y.sP, a.y.sD, col);
            bool inf = false;
            const double cost = box_cost_as<Giou, true>(row, col, inf);
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

// The box row source of batch_solve: PointBatchRows with the box cost.  bid and ece_bad run one wavefront per row, so
// the row's four coordinates and its area come from an address that is uniform over the wavefront and may live in
// scalar registers; gather runs one thread per row.  Nothing is precomputed per column: a column's width, height and
// area are formed with its cost.  The order of every scan, the tie rule and the outside entry are PointBatchRows'.  The
// metric is a template parameter: the "iou" instances carry no hull arithmetic.
template <class T, bool Out, bool Giou>
struct BoxBatchRows {
    const T *X, *Y;
    long long xP, xD, yP, yD;  // element strides of box and coordinate
    int n, m, maximize;
    BatchOutside<Out> out;

    __device__ __forceinline__ const T *xp(int i) const { return X + (size_t)i * (size_t)xP; }
    __device__ __forceinline__ const T *yp(int c) const { return Y + (size_t)c * (size_t)yP; }

    __device__ __forceinline__ void take(Top2 &x, double &cb, double v, int c, const double *price) const {
        const double cost = maximize ? v : v * -1.0;  // :236-237
        const double vi = cost - price[c];
        if (top2_take(x, vi, c)) cb = cost;
    }

    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        i = __builtin_amdgcn_readfirstlane(i);  // (uniform already: the row's box may live in scalar registers)
        BoxRow r;
        box_load(xp(i), xD, r);
        Top2 x;
        x.v = -__builtin_huge_val();
        x.w = -__builtin_huge_val();
        x.g = -1;
        double cb = 0.0;
        for (int c = lane; c < m; c += kWave) take(x, cb, box_cost<T, Giou>(r, yp(c), yD), c, price);
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
        BoxRow r;
        box_load(xp(i), xD, r);
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : box_cost<T, Giou>(r, yp(j), yD);
        else vj = box_cost<T, Giou>(r, yp(j), yD);
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
            const double v = box_cost<T, Giou>(r, yp(c), yD);
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
                BoxRow r;
                box_load(xp(i), xD, r);
                v = box_cost<T, Giou>(r, yp(j), yD);
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

// The checks of a verdict ahead of the starting prices, in their order: points_batch_verdict with the bad box behind
// the non-finite flag.
template <bool Out>
__device__ __forceinline__ int boxes_batch_verdict(const PointsBatchCheck &c, int n, int m) {
    if (n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (Out && (c.flags & 2)) return MISSLAP_BATCH_STATUS_BAD_OUTSIDE;
    if (c.flags & 1) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    if (c.flags & kBoxFlagBadBox) return MISSLAP_BATCH_STATUS_BAD_BOX;
    if (!Out && n > m) return MISSLAP_BATCH_STATUS_INFEASIBLE;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve of a boxes call: k_points_batch_solve on the box row source.
template <class T, bool Out, bool Giou>
__global__ __launch_bounds__(1024) void k_boxes_batch_solve(PointsBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = a.shapes[2 * b], m = a.shapes[2 * b + 1];
    const PointsBatchCheck ck = a.chk[b];
    const int code = batch_verdict(boxes_batch_verdict<Out>(ck, n, m), false, -1, n, ck.bad_price);
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
    const BoxBatchRows<T, Out, Giou> rows{static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB,
                                          static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB,
                                          a.x.sP, a.x.sD, a.y.sP, a.y.sD, n, m, s.maximize, out};
    batch_solve(s, rows, n, mo, ck.absmax_bits);
    if constexpr (Out) batch_outside_outputs(s_raw, a.s, b, n, m, M, N, po, oo, tid, nt);
}

// ---- the candidate builder (kernels_points_candidates.hpp) on the box cost.  The limit key, the stored value, the
// order, the streaming pass and the truncated path are that file's, on box_candidate_key.

// The key of the column box at p for row box r (rbad: the row has a NaN or infinite coordinate, an infinite width,
// height or area, or is a bad box).  A column with any of those, or a chain with an infinite intermediate, has key 0:
// it is always a candidate, sorts first and is stored as +inf.
template <class T, bool Giou>
__device__ __forceinline__ unsigned long long box_candidate_key(const BoxRow &r, bool rbad, const T *p, long long sD) {
    bool bad = rbad | box_coords_bad(p, sD);
    BoxRow col;
    bool inf = false;
    box_load_as<T, true>(p, sD, col, inf);
    bad |= box_inverted(col);
    const unsigned long long bits = (unsigned long long)__double_as_longlong(box_cost_as<Giou, true>(r, col, inf));
    return bad || inf || bits >= kPointsKeyInf ? 0ull : bits + 1ull;
}

// One row of the builder: the streaming pass, and where it counted more than K candidates the truncated path; returns
// the count.
template <class T, bool Giou>
__device__ __forceinline__ int box_candidates_row(const BoxRow &r, bool rbad, const T *Y, long long yP, long long yD, int m,
                                                  unsigned long long lim, int K, int *cols, double *vals) {
    const int lane = lane_id();
    const unsigned long long below_me = lanemask_lt();
    int count = 0;
    for (int c0 = 0; c0 < m; c0 += kWave) {
        const int c = c0 + lane;
        unsigned long long key = ~0ull;  // (beyond m: no candidate under any limit)
        if (c < m) key = box_candidate_key<T, Giou>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
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
            if (c < m) key = box_candidate_key<T, Giou>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
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
        if (c < m) key = box_candidate_key<T, Giou>(r, rbad, Y + (size_t)c * (size_t)yP, yD);
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

template <class T, bool Giou>
__global__ __launch_bounds__(kPointsCandidatesThreads) void k_boxes_batch_candidates(PointsCandidatesArgs a) {
    const int lane = lane_id(), K = a.K, N = (int)a.N, M = (int)a.M;
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
            bool rbad = box_coords_bad(X, a.x.sD);
            BoxRow r;
            box_load_as<T, true>(X, a.x.sD, r, rbad);
            rbad |= box_inverted(r);
            const unsigned long long lim =
                points_limit_key(a.limit ? a.limit + (a.limit_ld ? (size_t)b * (size_t)a.limit_ld + (size_t)i : (size_t)b) : nullptr);
            count = box_candidates_row<T, Giou>(r, rbad, Y, a.y.sP, a.y.sD, m, lim, K, cols, vals);
        }
        for (int s = (count < K ? count : K) + lane; s < K; s += kWave) {
            cols[s] = -1;
            vals[s] = 0.0;
        }
        if (lane == 0) a.counts[row] = count;
    }
}

}  // namespace misslap
