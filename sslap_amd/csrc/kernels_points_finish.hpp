// kernels_points_finish.hpp -- the reverse-auction finish behind misslap_solve_points_batch
// (misslap_points_batch_reverse_finish, include/misslap.h; the host side is abi_points_finish.hpp).
//
// What the finish is and why a rectangular solve needs it is said at k_dense_reverse_finish (kernels_dense_batch.hpp);
// sslap_amd.points_reverse_finish states this one in numpy: dense_reverse_finish on points_to_dense(x, y, shapes).
// k_points_reverse_finish<T, Out> is that kernel with another value source and twice the reach.  Its structure and the
// order of every float64 operation are the dense kernel's: one workgroup of 256 per problem, the gate on status[b] and
// meta.n_assigned before anything of the problem is read, the state p, pi, o2p, p2o in LDS (12 Mo + 12 N bytes, 73 728
// at 2048 x 2048 with outside), the serial loop on wavefront 0 alone without a workgroup barrier, and the outputs, the
// eCE pass and the row-order objective shared by the four wavefronts behind it.
//
// The value of (i, j), j < m, is points_cost (kernels_points_batch.hpp) on x_i loaded by points_load: the definition's
// chain, not restated here.  Every pair inside the shape is an entry (a square is >= 0, and the finish only runs on
// status 0, where every cost inside the shape is finite): no holes, no NaN test.
//
// The column scan of one iteration (points_finish_scan): y_j is uniform over the wavefront and its D coordinates are
// loaded once, from a uniform address; lane l takes rows l, l + 64, ... in ascending order with strict ">".  At N = 2048
// a lane has 32 rows of D coordinates each; they are scanned in groups of kPointsFinishGroup rows -- the loads of a
// group are issued back to back under one latency, then its costs are formed -- so that a group's widened coordinates
// (16 registers a row at D = 8) stay in registers.  A row beyond n is clamped to row n - 1 for the loads (only elements
// of the view are read) and skipped by the comparison.  x is re-read through the caches by every iteration (at most
// 128 KB per problem; staging it in the remaining LDS was not built); nothing of the point sets is written.  No
// instance uses scratch (DESIGN 4.29 has the register record).
#pragma once

namespace misslap {

constexpr int kPointsFinishThreads = 256;
constexpr int kPointsFinishGroup = 4;  // rows of a lane whose coordinates are in flight together
static_assert(kPointsBatchMaxCoords == 8, "k_points_reverse_finish names every D in a switch");

struct PointsFinishArgs {
    PointsView x, y;
    long long N, M;          // the extents of the point sets
    int D;
    const int *shapes;       // [B][2] or null
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]; read when Out
    long long outside_ld;
    int maximize;
    long long max_iter;      // the finish's own budget of iterations
    const int *status;       // [B] the solve's verdicts
    int *sol;                // [B][N]
    double *prices;          // [B][M]
    double *outside_prices;  // [B][N]; read and written when Out
    misslap_dense_batch_meta *meta;  // [B]
    long long *its;          // [B] iterations made, -1: not run
    int *left;               // [B] unassigned objects still priced above lambda (0 unless the budget cut), -1: not run
};

// The running top two of one lane's rows: the larger w first, strict ">" (the dense kernel's)
struct PointsFinishTop {
    double bw, ow, ba;
    int bi;
};

// The column scan of one iteration at DD coordinates (a constant here, so that points_load and points_cost unroll to
// straight-line code and the loads of a group are issued together; with the run-time D every load sat in a block of its
// own behind a scalar branch and was waited for before the next was issued).  Y: the point y_j, its D coordinates loaded
// once from a uniform address into yj[], which points_cost reads at stride 1.
template <class T, int DD>
__device__ __forceinline__ void points_finish_scan(const T *X, long long xP, long long xD, const T *Y, long long yD, int n,
                                                   int lane, int maximize, const double *pi, PointsFinishTop &t) {
    T yj[kPointsBatchMaxCoords];
#pragma unroll
    for (int k = 0; k < DD; ++k) yj[k] = Y[(size_t)k * (size_t)yD];
    for (int q0 = 0; q0 * kWave < n; q0 += kPointsFinishGroup) {
        double xi[kPointsFinishGroup][kPointsBatchMaxCoords];
#pragma unroll
        for (int q = 0; q < kPointsFinishGroup; ++q) {
            const int i = lane + (q0 + q) * kWave;  // (a row beyond n: row n - 1 is loaded, and skipped below)
            points_load(X + (size_t)(i < n ? i : n - 1) * (size_t)xP, xD, DD, xi[q]);
        }
#pragma unroll
        for (int q = 0; q < kPointsFinishGroup; ++q) {
            if ((q0 + q) * kWave >= n) break;  // (uniform)
            const int i = lane + (q0 + q) * kWave;
            const double e = points_cost(xi[q], yj, 1, DD);
            if (i < n) {
                const double av = maximize ? e : e * -1.0;
                const double w = av - pi[i];
                if (w > t.bw) {
                    t.ow = t.bw;
                    t.bw = w;
                    t.bi = i;
                    t.ba = av;
                } else if (w > t.ow) {
                    t.ow = w;
                }
            }
        }
    }
}

template <class T, bool Out>
__global__ __launch_bounds__(kPointsFinishThreads) void k_points_reverse_finish(PointsFinishArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_min[kPointsFinishThreads / kWave];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = nt >> 6;
    const int N = (int)a.N, M = (int)a.M, D = a.D;
    bool run = a.status[b] == MISSLAP_BATCH_STATUS_OK;
    int n = 0, m = 0;
    if (run) {
        dense_batch_shape(a.shapes, a.N, a.M, b, n, m);
        run = n >= 1 && n <= N && m >= 1 && m <= M && a.meta[b].n_assigned == (int64_t)n;
    }
    if (!run) {  // (uniform: nothing of the problem is read or written)
        if (tid == 0) {
            a.its[b] = -1;
            a.left[b] = -1;
        }
        return;
    }
    const int mo = Out ? m + n : m;
    const int Mo = Out ? M + N : M;
    double *p = reinterpret_cast<double *>(s_raw);  // [Mo]
    double *pi = p + Mo;                            // [N]
    int *o2p = reinterpret_cast<int *>(pi + N);     // [Mo]
    int *p2o = o2p + Mo;                            // [N]
    const int maximize = a.maximize;
    BatchOutside<Out> out;
    if constexpr (Out) {
        out.O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
        out.stride = a.outside_ld ? 1 : 0;
    }
    // the eCE pass and the objective are the solve's own (PointBatchRows::ece_bad, gather, objective)
    const PointBatchRows<T, Out> rows{static_cast<const T *>(a.x.p) + (size_t)b * (size_t)a.x.sB,
                                      static_cast<const T *>(a.y.p) + (size_t)b * (size_t)a.y.sB,
                                      a.x.sP, a.x.sD, a.y.sP, a.y.sD, D, n, m, maximize, out};
    int *sol = a.sol + (size_t)b * (size_t)N;
    double *po = a.prices + (size_t)b * (size_t)M;
    double *oo = nullptr;
    if constexpr (Out) oo = a.outside_prices + (size_t)b * (size_t)N;
    // the maximised value of entry (i, j) of the augmented problem
    auto value = [&](int i, int j) -> double {
        double v;
        if constexpr (Out) {
            if (j >= m) {
                v = out.value(i);
                return maximize ? v : v * -1.0;
            }
        }
        double xi[kPointsBatchMaxCoords];
        points_load(rows.xp(i), rows.xD, D, xi);
        v = points_cost(xi, rows.yp(j), rows.yD, D);
        return maximize ? v : v * -1.0;
    };

    // ---- set-up: p, o2p, p2o, pi and lambda
    if (tid == 0) s_bad = 0;
    for (int j = tid; j < mo; j += nt) {
        double pj;
        if constexpr (Out) pj = j < m ? po[j] : oo[j - m];
        else pj = po[j];
        p[j] = pj;
        o2p[j] = -1;
    }
    __syncthreads();
    double lmin = __builtin_huge_val();
    for (int i = tid; i < n; i += nt) {
        int j = sol[i];
        if (Out && j == -1) j = m + i;
        if (j < 0 || j >= mo || (j >= m && j != m + i)) {  // (not a solve's output: leave it alone)
            atomicOr(&s_bad, 1);
            j = Out ? m + i : 0;
        }
        p2o[i] = j;
        o2p[j] = i;
        const double pj = p[j];
        pi[i] = value(i, j) - pj;
        lmin = pj < lmin ? pj : lmin;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(lmin, off);
        lmin = o < lmin ? o : lmin;
    }
    if (lane == 0) s_min[wave] = lmin;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) {
            a.its[b] = -1;
            a.left[b] = -1;
        }
        return;
    }
    double lam = s_min[0];
    for (int w = 1; w < nw; ++w) lam = s_min[w] < lam ? s_min[w] : lam;
    const double eps = (double)a.meta[b].final_eps;

    // ---- the loop, on wavefront 0
    if (wave == 0) {
        const double ninf = -__builtin_huge_val();
        long long its = 0;
        int left = 0, cursor = 0, next = -1;
        for (;;) {
            int j = -1;
            if (next >= 0) {
                j = next;
                next = -1;
            } else {
                for (int base = cursor; base < mo; base += kWave) {
                    const int c = base + lane;
                    const bool hit = c < mo && o2p[c] == -1 && p[c] > lam;
                    const unsigned long long bm = __ballot(hit);
                    if (bm) {
                        j = base + __ffsll((long long)bm) - 1;
                        break;
                    }
                }
                if (j < 0) break;  // left = 0
                cursor = j + 1;
            }
            if (its >= a.max_iter) {  // the budget: what is left, j included
                for (int base = 0; base < mo; base += kWave) {
                    const int c = base + lane;
                    left += __popcll(__ballot(c < mo && o2p[c] == -1 && p[c] > lam));
                }
                break;
            }
            ++its;
            // column j over the rows, ascending within a lane: the top two of w = a_ij - pi_i, strict ">"
            double bw = ninf, ow = ninf, ba = 0.0;
            int bi = -1;
            if (!Out || j < m) {
                const T *yj = rows.yp(__builtin_amdgcn_readfirstlane(j));  // (uniform already)
                PointsFinishTop t{ninf, ninf, 0.0, -1};
                switch (D) {  // (uniform; 1 .. kPointsBatchMaxCoords: the host has checked it)
#define MISSLAP_POINTS_FINISH_SCAN(DD)                                                                                  \
    case DD:                                                                                                           \
        points_finish_scan<T, DD>(rows.X, rows.xP, rows.xD, yj, rows.yD, n, lane, maximize, pi, t);                    \
        break;
                    MISSLAP_POINTS_FINISH_SCAN(1)
                    MISSLAP_POINTS_FINISH_SCAN(2)
                    MISSLAP_POINTS_FINISH_SCAN(3)
                    MISSLAP_POINTS_FINISH_SCAN(4)
                    MISSLAP_POINTS_FINISH_SCAN(5)
                    MISSLAP_POINTS_FINISH_SCAN(6)
                    MISSLAP_POINTS_FINISH_SCAN(7)
                    MISSLAP_POINTS_FINISH_SCAN(8)
#undef MISSLAP_POINTS_FINISH_SCAN
                    default: break;
                }
                bw = t.bw;
                ow = t.ow;
                ba = t.ba;
                bi = t.bi;
            } else if (lane == 0) {  // an outside object: the one entry of its row
                const int i = j - m;
                const double av = value(i, j);
                const double w = av - pi[i];
                if (w > bw) {
                    bw = w;
                    bi = i;
                    ba = av;
                }
            }
            // across lanes: the larger w, the smaller row on a tie (a lane without an entry holds row -1 = UINT_MAX);
            // the second is the largest of the two seconds and the smaller of the two bests.  Symmetric, so after the
            // butterfly every lane holds the same result.
            for (int off = 32; off >= 1; off >>= 1) {
                const double xb = __shfl_xor(bw, off), xo = __shfl_xor(ow, off), xa = __shfl_xor(ba, off);
                const int xi = __shfl_xor(bi, off);
                const bool take = xb > bw || (xb == bw && (unsigned)xi < (unsigned)bi);
                const double lo = take ? bw : xb;
                const double o2 = xo > ow ? xo : ow;
                ow = lo > o2 ? lo : o2;
                if (take) {
                    bw = xb;
                    bi = xi;
                    ba = xa;
                }
            }
            if (bi < 0 || lam >= bw - eps) {
                if (lane == 0) p[j] = lam;
            } else {
                const double t = ow - eps;
                const double pj = t > lam ? t : lam;
                if (!(ba - pj > pi[bi])) {  // a stall (uniform): eps is lost to rounding, the move would not raise the
                                            // row's profit.  Nothing is written; what is left, j included
                    for (int base = 0; base < mo; base += kWave) {
                        const int c = base + lane;
                        left += __popcll(__ballot(c < mo && o2p[c] == -1 && p[c] > lam));
                    }
                    break;
                }
                const int jo = p2o[bi];
                const double pjo = p[jo];
                if (lane == 0) {
                    p[j] = pj;
                    pi[bi] = ba - pj;
                    o2p[jo] = -1;
                    o2p[j] = bi;
                    p2o[bi] = j;
                }
                if (pjo > lam) next = jo;
            }
            dense_finish_wave_sync();
        }
        if (lane == 0) {
            a.its[b] = its;
            a.left[b] = left;
        }
    }
    if (tid == 0) s_bad = 0;  // (from here on: the eCE flag)
    __syncthreads();

    // ---- the outputs in the caller's terms, eCE at target eps, the chosen values (into pi, which the loop and then the
    // eCE pass are done with) and the objective in row order
    for (int i = tid; i < n; i += nt) sol[i] = p2o[i] < m ? p2o[i] : -1;
    for (int j = tid; j < m; j += nt) po[j] = p[j];
    if constexpr (Out)
        for (int i = tid; i < n; i += nt) oo[i] = p[m + i];
    const double tol = 1e-7, teps = (double)(float)(1.0 / (double)n);
    for (int i = wave; i < n; i += nw) {  // eCE_satisfied (auction_.pyx:443-485), as batch_ece makes it
        const bool bad = rows.ece_bad(i, p2o[i], p, tol, teps);
        if (__ballot(bad) && lane == 0) s_bad = 1;
    }
    __syncthreads();
    double *selv = pi;
    rows.gather(p2o, n, selv, nullptr);
    __syncthreads();
    if (tid == 0) {  // get_obj (:489-523) in row order
        const double obj = rows.objective(p2o, n, selv, nullptr);
        misslap_dense_batch_meta &r = a.meta[b];
        r.obj_f64 = obj;
        r.obj_f32 = (float)obj;
        r.eCE = s_bad ? 0 : 1;
    }
}

}  // namespace misslap
