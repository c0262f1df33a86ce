// kernels_list_finish.hpp -- the reverse-auction finish of the list batch solves (misslap_sparse_batch_reverse_finish,
// misslap_ell_batch_reverse_finish, include/misslap.h; the host side is abi_list_finish.hpp).
//
// What the finish is and why a rectangular solve needs it is said at k_dense_reverse_finish (kernels_dense_batch.hpp);
// its definition for the list families is sslap_amd.sparse_reverse_finish, which builds the dense image of a problem and
// runs the dense model's loop on it.  This kernel is that loop on the list row source of batch_solve (ListBatchRows,
// kernels_batch_solve.hpp) through its run accessors: SparseRuns<Src> (kernels_sparse_batch.hpp) and EllRuns<I, V>
// (kernels_ell_batch.hpp).  start / len / col / value / kHoles and the BatchOutside value access are theirs; the eCE test
// and the objective behind the loop are the row source's own ece_bad / gather / objective, so what the finish reports
// is what the forward solve would report for the final state.
//
// One workgroup of 256 threads per problem, its own launch behind the solve's.  status[b] is read first, then the
// record: n_b = n_rows, m_b = n_cols (minus n_rows with outside); a problem with status != 0 or n_assigned != n_rows is
// not touched, its = left = -1.
//
// THE COLUMN INDEX.  An iteration needs column j of a row-major list, at a cost that depends on the length of column j
// and not on the problem's entries.  So the workgroup first builds a column index of its problem:
//   1  count the entries per real column: an LDS histogram over the m_b real objects, holes skipped
//   2  an exclusive scan into col_start[m_b + 1], in LDS
//   3  scatter every entry into the problem's segment of the global workspace, through an LDS cursor per column (a
//      returning LDS atomicAdd).  What is stored per entry is (row, maximised value): 12 bytes, and an iteration then
//      makes ONE dependent global access (two loads issued together) where the stored index g would need three
//      (g, then the row and the value of g).
//   4  a barrier, then the loop.
// Outside objects need no index: object j >= m_b has the one row j - m_b.
// The sparse source also needs the row starts of its problem (start / len).  The solve kept them in its own workspace,
// which this call does not see; pass 1 finds them again (the rows ascend: the solve's verdict was 0) into rs[N + 1] in
// LDS, and SparseRuns reads them there.
//
// ORDER INDEPENDENCE.  Within a column the order of the index is whatever the atomics gave.  The top two are reduced
// under a total order -- larger w, then smaller row, then larger a -- and omega is taken over the entries of rows other
// than i*: merging two partials with the same best row keeps the larger beta (on a tie the larger a) and the larger
// omega; with different rows the loser's beta competes with the winner's omega (the loser's omega is at most its beta).
// That is the image's "largest value among the duplicates of an (i, j)": w = a - pi_i in float64 per entry, rounding is
// monotone, so the maximum over duplicates is the image's w; and two runs of one call give the same bits.
//
// The loop runs on wavefront 0 alone with the dense kernel's structure: the cursor / ballot pick of j, lanes over the
// column's entries in chunks of 64, the shuffle butterfly that leaves (beta, i*, a, omega) in every lane, lane 0 storing
// the changed cells, a wavefront-scope fence and no workgroup barrier inside an iteration, stall and budget as in the
// dense kernel with `left` counted by ballots.  Wavefronts 1-3 help build the index and load the state and wait at the
// one barrier behind the loop; then all four share the eCE test and the outputs.
//
// LDS, carved for the call's N rows, M real columns and Mo = M (+ N with outside) objects: p[Mo], pi[N], o2p[Mo],
// p2o[N], col_start[M + 1], and for the sparse source rs[N + 1]: 12 Mo + 12 N + 4 (M + 1) (+ 4 (N + 1)) bytes, 90 120 at
// 2048 x 2048 sparse with outside -- above 64 KiB, so the launch makes the dynamic-LDS opt-in.
#pragma once

namespace misslap {

constexpr int kListFinishThreads = 256;

// What a family's launch passes and how the kernel opens problem b of it: ListFinishSrc<Acc>.
//   kRowStarts          whether the accessor needs the problem's row starts found again (rs[N + 1] in LDS)
//   open(b, n, s, cnt)  the problem's first entry (added to a local index k by entry()) and its slots; false: unusable
//   runs(s, rs)         the accessor
//   entry(s, k)         the accessor's index of local slot k;  row(s, k, n) its row
template <class Acc>
struct ListFinishSrc;

template <class Src>
struct ListFinishSrc<SparseRuns<Src>> {
    static constexpr bool kRowStarts = true;
    Src w;
    const long long *offsets;  // [B + 1]
    long long nnz;             // the packed entries of the whole call

    __device__ __forceinline__ bool open(int b, int, long long &s, int &cnt) const {
        s = offsets[b];
        const long long e = offsets[b + 1];
        if (!sparse_view_slice_ok(s, e, nnz)) return false;
        cnt = (int)(e - s);
        return true;
    }
    __device__ __forceinline__ SparseRuns<Src> runs(long long s, const int *rs) const { return {w, offsets, s, rs, 0}; }
    __device__ __forceinline__ long long entry(long long s, int k) const { return s + k; }
    __device__ __forceinline__ int row(long long s, int k) const { return w.row(s + k); }
};

template <class I, class V>
struct ListFinishSrc<EllRuns<I, V>> {
    static constexpr bool kRowStarts = false;
    const void *cols, *vals;  // [B][N][K]
    long long N, K;

    __device__ __forceinline__ bool open(int b, int n, long long &s, int &cnt) const {
        s = (long long)((size_t)b * (size_t)N * (size_t)K);
        cnt = n * (int)K;  // (N * K <= INT_MAX - 128: the host's check)
        return true;
    }
    __device__ __forceinline__ EllRuns<I, V> runs(long long s, const int *) const {
        return {static_cast<const I *>(cols) + s, static_cast<const V *>(vals) + s, (int)K, 0ull};
    }
    __device__ __forceinline__ int entry(long long, int k) const { return k; }
    __device__ __forceinline__ int row(long long, int k) const { return k / (int)K; }
};

template <class Acc>
struct ListFinishArgs {
    ListFinishSrc<Acc> src;
    int N, M;                // the carve: the bound on the rows and on the real columns; sol_ld and prices_ld
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]; read when Out
    long long outside_ld;
    int maximize;
    long long max_iter;      // the finish's own budget of iterations
    double *index_a;         // the workspace: the column index's maximised values, one per entry of the call ...
    int *index_row;          // ... and their rows
    const int *status;       // [B] the solve's verdicts
    int *sol;                // [B][N]
    double *prices;          // [B][M]
    double *outside_prices;  // [B][N]; read and written when Out
    misslap_dense_batch_meta *meta;  // [B]
    long long *its;          // [B] iterations made, -1: not run
    int *left;               // [B] unassigned objects still priced above lambda, -1: not run
};

__host__ __device__ constexpr size_t list_finish_lds_bytes(long long N, long long M, bool out, bool row_starts) {
    const size_t Mo = (size_t)(out ? M + N : M);
    return Mo * (8 + 4) + (size_t)N * (8 + 4) + ((size_t)M + 1) * 4 + (row_starts ? ((size_t)N + 1) * 4 : 0);
}

// One entry (w, i, a) or one partial (xb, xi, xa, xo) into the running (bw, bi, ba, ow) under the total order: larger w,
// then smaller row (no row: -1 = UINT_MAX), then larger a; ow over the rows other than bi.  Commutative and
// associative, so neither the scatter order nor the butterfly's pairing shows in the result.
__device__ __forceinline__ void list_finish_merge(double &bw, int &bi, double &ba, double &ow, double xb, int xi,
                                                  double xa, double xo) {
    if (xi == bi) {
        ow = xo > ow ? xo : ow;
        if (xb > bw || (xb == bw && xa > ba)) {
            bw = xb;
            ba = xa;
        }
        return;
    }
    const bool take = xb > bw || (xb == bw && (unsigned)xi < (unsigned)bi);
    if (take) {
        ow = bw > xo ? bw : xo;
        bw = xb;
        bi = xi;
        ba = xa;
    } else {
        ow = xb > ow ? xb : ow;
    }
}

template <class Acc, bool Out>
__global__ __launch_bounds__(kListFinishThreads) void k_list_reverse_finish(ListFinishArgs<Acc> a) {
    using Src = ListFinishSrc<Acc>;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_min[kListFinishThreads / kWave];
    __shared__ int s_scan[kListFinishThreads / kWave];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = nt >> 6;
    const int N = a.N, M = a.M;
    auto not_run = [&] {
        if (tid == 0) {
            a.its[b] = -1;
            a.left[b] = -1;
        }
    };
    if (a.status[b] != MISSLAP_BATCH_STATUS_OK) {  // (uniform: nothing else of the problem is read or written)
        not_run();
        return;
    }
    const long long rec_n = a.meta[b].n_rows, rec_m = a.meta[b].n_cols - (Out ? a.meta[b].n_rows : 0);
    if (rec_n < 1 || rec_n > N || rec_m < (Out ? 0 : 1) || rec_m > M || a.meta[b].n_assigned != rec_n) {
        not_run();
        return;
    }
    const int n = (int)rec_n, m = (int)rec_m;
    long long s = 0;
    int cnt = 0;
    if (!a.src.open(b, n, s, cnt)) {
        not_run();
        return;
    }
    const int mo = Out ? m + n : m;
    const int Mo = Out ? M + N : M;
    double *p = reinterpret_cast<double *>(s_raw);  // [Mo]
    double *pi = p + Mo;                            // [N]
    int *o2p = reinterpret_cast<int *>(pi + N);     // [Mo]  (while the index is built: the columns' cursors)
    int *p2o = o2p + Mo;                            // [N]
    int *cs = p2o + N;                              // [M + 1]
    int *rs = cs + M + 1;                           // [N + 1], Src::kRowStarts only
    const double *O = nullptr;
    int ostride = 0;
    if constexpr (Out) {
        O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
        ostride = a.outside_ld ? 1 : 0;
    }
    const int maximize = a.maximize;
    int *sol = a.sol + (size_t)b * (size_t)N;
    double *po = a.prices + (size_t)b * (size_t)M;
    double *oo = Out ? a.outside_prices + (size_t)b * (size_t)N : nullptr;
    double *ia = a.index_a + s;  // the problem's segment of the index: its slots s .. s + cnt of the call's entries
    int *ir = a.index_row + s;
    BatchOutside<Out> out{};
    if constexpr (Out) out = BatchOutside<true>{O, ostride};
    const ListBatchRows<Acc, Out> rows{a.src.runs(s, rs), maximize, m, out};
    const Acc &acc = rows.a;

    // ---- the column index: count (and the sparse source's row starts), scan, scatter
    if (tid == 0) s_bad = 0;
    for (int j = tid; j <= m; j += nt) cs[j] = 0;
    __syncthreads();
    int bad = 0;
    for (int k = tid; k < cnt; k += nt) {
        const auto g = a.src.entry(s, k);
        const auto c = acc.col(g);
        if constexpr (Acc::kHoles)
            if (c < 0) continue;
        const int r = a.src.row(s, k);
        if (c < 0 || c >= (decltype(c))m || (unsigned)r >= (unsigned)n) {  // (not what a solve with status 0 read)
            bad = 1;
            continue;
        }
        if constexpr (Src::kRowStarts) {
            const int rp = k ? a.src.row(s, k - 1) : -1;
            if (r < rp) bad = 1;
            else
                for (int i = (rp < 0 ? 0 : rp + 1); i <= r; ++i) rs[i] = k;
        }
        atomicAdd(&cs[(int)c + 1], 1);
    }
    if constexpr (Src::kRowStarts) {
        if (tid == 0) {
            int last = cnt ? a.src.row(s, cnt - 1) : -1;
            last = last < -1 ? -1 : (last >= n ? n - 1 : last);
            for (int i = last + 1; i <= n; ++i) rs[i] = cnt;
        }
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (s_bad) {
        not_run();
        return;
    }
    {  // cs[j + 1] = the entries of columns 0 .. j: each thread a run of consecutive columns, the runs' sums scanned
        const int chunk = (m + nt - 1) / nt;
        const int lo = tid * chunk < m ? tid * chunk : m, hi = lo + chunk < m ? lo + chunk : m;
        int sum = 0;
        for (int j = lo; j < hi; ++j) sum += cs[j + 1];
        int x = sum;
        for (int d = 1; d < kWave; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == kWave - 1) s_scan[wave] = x;
        __syncthreads();
        int run = x - sum;
        for (int w = 0; w < wave; ++w) run += s_scan[w];
        for (int j = lo; j < hi; ++j) {
            run += cs[j + 1];
            cs[j + 1] = run;
        }
    }
    __syncthreads();
    for (int j = tid; j < m; j += nt) o2p[j] = cs[j];  // the cursors
    __syncthreads();
    for (int k = tid; k < cnt; k += nt) {
        const auto g = a.src.entry(s, k);
        const auto c = acc.col(g);
        if constexpr (Acc::kHoles)
            if (c < 0) continue;
        const double v = dense_widen(acc.value(g));
        const int at = atomicAdd(&o2p[(int)c], 1);  // (below cs[c + 1] <= cnt: the same entries were counted)
        ia[at] = maximize ? v : v * -1.0;
        ir[at] = a.src.row(s, k);
    }
    __syncthreads();  // (the index is read by wavefront 0 of this workgroup only)

    // ---- set-up: p, o2p, p2o, pi and lambda
    for (int j = tid; j < mo; j += nt) {
        p[j] = j < m ? po[j] : oo[j - m];
        o2p[j] = -1;
    }
    __syncthreads();
    const double ninf = -__builtin_huge_val();
    for (int i = wave; i < n; i += nw) {  // a wavefront per row: the image's value of (i, sol[i]), the largest duplicate
        int j = sol[i];
        if (Out && j == -1) j = m + i;
        double av = ninf;
        bool found = false;
        if (j >= 0 && j < m) {
            const auto g0 = acc.start(i);
            const int len = acc.len(i);
            for (int q = lane; q < len; q += kWave) {
                if (acc.col(g0 + q) != (typename Acc::Col)j) continue;
                const double v = dense_widen(acc.value(g0 + q));
                const double x = maximize ? v : v * -1.0;
                av = (!found || x > av) ? x : av;
                found = true;
            }
            found = __ballot(found) != 0ull;
            av = wave_max_f64(av);
        } else if (Out && j == m + i) {
            const double v = O[i * ostride];
            av = maximize ? v : v * -1.0;
            found = true;
        }
        if (lane == 0) {
            if (!found) {  // (not a solve's output: leave the problem alone)
                s_bad = 1;
                j = 0;
                av = 0.0;
            }
            p2o[i] = j;
            if (found && atomicExch(&o2p[j], i) != -1) s_bad = 1;  // (two rows on one object: no solve's output either)
            pi[i] = av - p[j];
        }
    }
    __syncthreads();
    if (s_bad) {
        not_run();
        return;
    }
    double lmin = __builtin_huge_val();
    for (int i = tid; i < n; i += nt) {
        const double pj = p[p2o[i]];
        lmin = pj < lmin ? pj : lmin;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(lmin, off);
        lmin = o < lmin ? o : lmin;
    }
    if (lane == 0) s_min[wave] = lmin;
    __syncthreads();
    double lam = s_min[0];
    for (int w = 1; w < nw; ++w) lam = s_min[w] < lam ? s_min[w] : lam;
    const double eps = (double)a.meta[b].final_eps;

    // ---- the loop, on wavefront 0
    if (wave == 0) {
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
            // column j through the index, in whatever order the scatter left: the top two of w = a_ij - pi_i
            double bw = ninf, ow = ninf, ba = 0.0;
            int bi = -1;
            if (!Out || j < m) {
                const int c1 = cs[j + 1];
                for (int q = cs[j] + lane; q < c1; q += kWave) {
                    const int i = ir[q];
                    const double av = ia[q];
                    const double w = av - pi[i];
                    if (w > ninf) list_finish_merge(bw, bi, ba, ow, w, i, av, ninf);
                }
            } else if (lane == 0) {  // an outside object: the one entry of its row
                const int i = j - m;
                const double v = O[i * ostride];
                const double av = maximize ? v : v * -1.0;
                const double w = av - pi[i];
                if (w > ninf) {
                    bw = w;
                    bi = i;
                    ba = av;
                }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const double xb = __shfl_xor(bw, off), xo = __shfl_xor(ow, off), xa = __shfl_xor(ba, off);
                const int xi = __shfl_xor(bi, off);
                list_finish_merge(bw, bi, ba, ow, xb, xi, xa, xo);
            }
            if (bi < 0 || lam >= bw - eps) {
                if (lane == 0) p[j] = lam;
            } else {
                const double t = ow - eps;
                const double pj = t > lam ? t : lam;
                if (!(ba - pj > pi[bi])) {  // a stall (uniform): nothing is written; what is left, j included
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

    // ---- the outputs in the caller's terms; eCE at target eps and the objective as the row source makes them
    for (int i = tid; i < n; i += nt) sol[i] = p2o[i] < m ? p2o[i] : -1;
    for (int j = tid; j < m; j += nt) po[j] = p[j];
    if constexpr (Out)
        for (int i = tid; i < n; i += nt) oo[i] = p[m + i];
    const double tol = 1e-7, teps = (double)(float)(1.0 / (double)n);
    for (int i = wave; i < n; i += nw) {
        const bool bad_row = rows.ece_bad(i, p2o[i], p, tol, teps);
        if (__ballot(bad_row) && lane == 0) s_bad = 1;
    }
    __syncthreads();  // (pi and o2p are done with: the objective's gather takes them)
    double *selv = pi;
    int *nsel = o2p;
    rows.gather(p2o, n, selv, nsel);
    __syncthreads();
    if (tid == 0) {
        const double obj = rows.objective(p2o, n, selv, nsel);
        misslap_dense_batch_meta &r = a.meta[b];
        r.obj_f64 = obj;
        r.obj_f32 = (float)obj;
        r.eCE = s_bad ? 0 : 1;
    }
}

}  // namespace misslap
