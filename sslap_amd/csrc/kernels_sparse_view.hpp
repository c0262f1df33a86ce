// kernels_sparse_view.hpp -- the sparse batch on a VIEW of the packed arrays, read where a device pipeline left them
// (misslap_solve_sparse_batch_status_view / _outside_view, include/misslap.h; the host side is abi_sparse_view.hpp):
// int32 or int64 indices with run-time strides, float64 or float32 values, and offsets that only the device has seen.
//
// A kernel family of its own next to kernels_sparse_batch.hpp, which it leaves untouched: the check pass, the row source
// of batch_solve and the two solve kernels, each an instance per index type I (int, long long) and value type V (double,
// float).  What differs from the contiguous family:
//   ACCESS   entry g is row loc[g * se], column loc[g * se + sc], value val[g] (SparseView); offsets are formed in 64
//            bits.  An int64 index outside the int32 range SATURATES to INT_MIN / INT_MAX as it is read, before any
//            check sees it: a value at or below -2^31 is a negative index whatever its low word is, one at or above 2^31
//            is beyond every carve, and nothing is ever truncated into a valid index.  A float32 value is widened to
//            double as it is read (exact); everything downstream is the float64 arithmetic of the contiguous family.
//   OFFSETS  nobody checked them on the host.  A problem whose slice is not 0 <= offsets[b] <= offsets[b + 1] <= nnz,
//            or holds 2^31 - 1 entries or more, gets kErrBadSlice from the check pass before anything of loc / val is
//            read; the solve kernels turn that into MISSLAP_BATCH_STATUS_BAD_SHAPE ahead of every other check, and the
//            guard skips the problem.
//   ROW STARTS  in a block of Ns + 1 ints per problem in both modes (the contiguous plain mode keeps them at
//            offsets[b] + b, which races between problems once the offsets are not monotone); every index written is
//            clamped to the block.
// Apart from that every verdict, output and record is the contiguous family's, bit for bit.
#pragma once

namespace misslap {

constexpr int kErrBadSlice = 1 << 12;  // SparseBatchCheck::err of the view family: offsets[b] .. offsets[b + 1] is unusable

// The packed arrays as the caller's view presents them.
template <class I, class V>
struct SparseView {
    const I *loc;      // entry g: row loc[g * se], column loc[g * se + sc]
    const V *val;      // [nnz], contiguous
    long long se, sc;  // >= 0, in elements of I

    __device__ __forceinline__ static int narrow(I v) {
        if constexpr (sizeof(I) == 8)
            return v < (I)INT_MIN ? INT_MIN : (v > (I)INT_MAX ? INT_MAX : (int)v);
        else
            return v;
    }
    __device__ __forceinline__ int row(long long g) const { return narrow(loc[g * se]); }
    __device__ __forceinline__ int col(long long g) const { return narrow(loc[g * se + sc]); }
    __device__ __forceinline__ double value(long long g) const { return (double)val[g]; }
};

// Whether offsets[b] .. offsets[b + 1] = s .. e is a slice of the nnz packed entries that a problem can be
__device__ __forceinline__ bool sparse_view_slice_ok(long long s, long long e, long long nnz) {
    return s >= 0 && s <= e && e <= nnz && e - s < (long long)INT_MAX;
}

// sparse_batch_check (kernels_sparse_batch.hpp) through a view: the same checks, maxima, C and row starts, in both
// modes.  rs is the problem's own block of Ns + 1 row starts.  A problem with an unusable slice leaves only its record.
template <class I, class V, bool Out>
__device__ __forceinline__ void sparse_view_check(const SparseView<I, V> &w, const long long *offsets, long long nnz_all,
                                                  const double *p0, long long p0_ld, int *rs, SparseBatchCheck *out,
                                                  const long long *sizes, const double *ov, long long ov_ld,
                                                  double *aug, long long aug_ld, int Ns, int Ms) {
    const int b = blockIdx.x;
    const long long s = offsets[b], e = offsets[b + 1];
    if (!sparse_view_slice_ok(s, e, nnz_all)) {  // (uniform)
        if (threadIdx.x == 0) {
            SparseBatchCheck c{};
            c.max_row = INT_MIN;
            c.max_col = INT_MIN;
            c.last_row = -1;
            c.err = kErrBadSlice;
            out[b] = c;
        }
        return;
    }
    const int nnz = (int)(e - s);
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
    const int last_row = nnz > 0 ? w.row(e - 1) : -1;
    int err = 0, mr = INT_MIN, mc = INT_MIN;
    unsigned long long am = 0ull;
    int n = 0;  // the outside mode's n_b
    if constexpr (Out) {
        if (sizes) {
            const long long v = sizes[2 * b + 1];
            n = (int)(v < -1 ? -1 : (v > INT_MAX ? INT_MAX : v));
        } else {
            n = last_row < 0 ? 0 : (last_row == INT_MAX ? INT_MAX : last_row + 1);
        }
        const int nr = n < Ns ? n : Ns;  // the rows whose outside value is read
        for (int i = threadIdx.x; i < (ov_ld ? nr : (nr > 0 ? 1 : 0)); i += blockDim.x) {
            const unsigned long long bits =
                (unsigned long long)__double_as_longlong(ov[ov_ld ? (size_t)b * (size_t)ov_ld + (size_t)i : (size_t)b]) &
                0x7fffffffffffffffull;
            if (bits >= 0x7ff0000000000000ull) err |= kErrNonFinite;
            am = bits > am ? bits : am;
        }
    }
    for (int k = threadIdx.x; k < nnz; k += blockDim.x) {
        const long long g = s + k;
        const int r = w.row(g), c = w.col(g);
        mr = r > mr ? r : mr;
        mc = c > mc ? c : mc;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(w.value(g)) & 0x7fffffffffffffffull;
        if (bits >= 0x7ff0000000000000ull) err |= kErrNonFinite;
        am = bits > am ? bits : am;
        if (r < 0 || c < 0) {
            err |= kErrColNegative;
            continue;
        }
        const int rp = k ? w.row(g - 1) : -1;
        if (r < rp) err |= kErrRowsUnsorted;
        else if (r > rp) {
            if constexpr (Out) {
                const int hi = r < Ns ? r : Ns;
                for (int i = rp < 0 ? 0 : rp + 1; i <= hi; ++i) rs[i] = k;
            } else {
                if (r != rp + 1 || r > last_row) err |= kErrRowGap;
                else if (r <= k && r <= Ns) rs[r] = k;  // (r > k implies a gap earlier in the problem)
            }
        }
    }
    if (err) atomicOr(&s_err, err);
    if (mr != INT_MIN) atomicMax(&s_maxr, mr);
    if (mc != INT_MIN) atomicMax(&s_maxc, mc);
    if (am) atomicMax(&s_abs, am);
    __syncthreads();
    if constexpr (Out) {
        const long long m = s_maxc < 0 ? 0 : (long long)s_maxc + 1;  // m_b (0 without an entry)
        if (p0 && s_err == 0 && m > 0)
            batch_check_prices(p0 + (size_t)b * (size_t)p0_ld, (int)(m < p0_ld ? m : p0_ld), &s_badp);
        if (p0 && s_err == 0 && n >= 1 && n <= Ns && m <= (long long)Ms && m <= p0_ld) {
            const double *src = p0 + (size_t)b * (size_t)p0_ld;
            double *dst = aug + (size_t)b * (size_t)aug_ld;
            for (int j = threadIdx.x; j < (int)m + n; j += blockDim.x) dst[j] = j < (int)m ? src[j] : 0.0;
        }
    } else {
        const long long m = s_maxc < 0 ? 0 : (long long)s_maxc + 1;  // n_cols (only meaningful without errors)
        if (p0 && s_err == 0 && m > 0)
            batch_check_prices(p0 + (size_t)b * (size_t)p0_ld, (int)(m < p0_ld ? m : p0_ld), &s_badp);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (Out) {
            const int hi = n < Ns ? n : Ns;
            for (int i = last_row < 0 ? 0 : (last_row < Ns ? last_row + 1 : Ns + 1); i <= hi; ++i) rs[i] = nnz;
        } else {
            if (last_row >= 0 && last_row < nnz && last_row < Ns) rs[last_row + 1] = nnz;  // :47
        }
        SparseBatchCheck c;
        c.absmax_bits = s_abs;
        c.max_row = s_maxr;
        c.max_col = s_maxc;
        c.last_row = last_row;
        c.err = s_err;
        c.bad_price = s_badp;
        c.n = n;
        out[b] = c;
    }
}

template <class I, class V>
struct SparseViewCheckArgs {
    SparseView<I, V> w;
    const long long *offsets, *sizes;  // sizes: [B][2] or null (read in the outside mode only)
    long long nnz;                     // the packed entries of the whole call
    const double *p0;
    long long p0_ld;
    int *row_start;  // [B][Nmax + 1]
    SparseBatchCheck *out;
    const double *outside;  // the outside mode: [B] (outside_ld == 0) or [B][outside_ld], outside_ld >= Nmax
    long long outside_ld;
    double *aug;            // the outside mode: [B][aug_ld] or null (no starting prices)
    long long aug_ld;       // Mmax + Nmax
    int Nmax, Mmax;
};

template <class I, class V, bool Out>
__global__ __launch_bounds__(256) void k_sparse_view_check(SparseViewCheckArgs<I, V> a) {
    sparse_view_check<I, V, Out>(a.w, a.offsets, a.nnz, a.p0, a.p0_ld,
                                 a.row_start + (size_t)blockIdx.x * ((size_t)a.Nmax + 1), a.out, a.sizes, a.outside,
                                 a.outside_ld, a.aug, a.aug_ld, a.Nmax, a.Mmax);
}

// SparseBatchRows (kernels_sparse_batch.hpp) through a view: the same lane map, tie keys and orders; only the reads of
// a column and of a value differ.
template <class I, class V, bool Out>
struct SparseViewRows {
    SparseView<I, V> w;
    const long long *offsets;
    long long s;
    const int *rs;
    int maximize;
    int m, n;  // the real columns and the rows (read in the outside mode only)
    BatchOutside<Out> out;

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
            const int c = w.col(g0 + q);
            const double v = w.value(g0 + q);
            const double cost = maximize ? v : v * -1.0;  // :236-237
            const double vi = cost - price[c];
            if (vi >= x.v) {  // :351
                x.w = x.v;
                x.v = vi;
                x.g = q;
                cb = cost;
                cj = c;
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
            if (w.col(g0 + q) == j) last = q;
        last = wave_max_i32(last);
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : w.value(g0 + (last < 0 ? 0 : last));  // (j < m: stored, last >= 0)
        else vj = w.value(g0 + last);
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
            const double v = w.value(g0 + q);
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[w.col(g0 + q)]) - eps) bad = true;  // :482
        }
        return bad;
    }

    // get_obj (:489-523) over EVERY entry of the chosen column, as SparseBatchRows::gather
    __device__ __forceinline__ void gather(const int *p2o, int n_, double *selv, int *nsel) const {
        const int lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int i = wave; i < n_; i += nw) {
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
            const long long g0 = s + rs[i];
            const int len = rs[i + 1] - rs[i];
            int cnt = 0, at = -1;
            for (int q = lane; q < len; q += kWave)
                if (w.col(g0 + q) == j) {
                    ++cnt;
                    at = q;
                }
            for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
            at = wave_max_i32(at);
            if (lane == 0) {
                nsel[i] = cnt;
                selv[i] = w.value(g0 + at);
            }
        }
    }

    // a double sum in row order, within a row in stored order
    __device__ __forceinline__ double objective(const int *p2o, int n_, const double *selv, const int *nsel) const {
        double obj = 0;
        for (int i = 0; i < n_; ++i) {
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
                if (w.col(g0 + q) == j) {
                    const double x = w.value(g0 + q);
                    const double v = maximize ? x : x * -1.0;
                    if (maximize) obj += v;
                    else obj -= v;
                }
        }
        return obj;
    }

    // (m_: batch_solve's object count, in the outside mode m + n)
    __device__ __forceinline__ int meta_cols(int m_) const { return m_; }
    __device__ __forceinline__ int64_t meta_nnz() const {
        return (int64_t)(offsets[blockIdx.x + 1] - s) + (Out ? (int64_t)n : 0);
    }
};

template <class I, class V>
struct SparseViewArgs {
    BatchSolveArgs s;             // Ns / Ms: the caller's bound (the LDS carve)
    SparseView<I, V> w;
    const long long *offsets;     // [B + 1]
    const int *row_start;         // [B][Ns + 1]
    const SparseBatchCheck *chk;  // [B]
};

template <class I, class V>
struct SparseViewStatusArgs {
    SparseViewArgs<I, V> d;  // d.s.Ns / Ms = Nmax / Mmax
    const long long *sizes;  // [B][2] or null
    const int *card;         // [B] the guard's cardinalities (-1: not matched), or null
    int fast;
    int *status;         // [B]
    int *matching_size;  // [B] or null
};

// k_sparse_batch_solve_status (kernels_sparse_batch.hpp) on a view.  An unusable slice is BAD_SHAPE before anything
// else: its offsets are not read again and its record is all zeros.
template <class I, class V>
__global__ __launch_bounds__(1024) void k_sparse_view_solve_status(SparseViewStatusArgs<I, V> a) {
    const int b = blockIdx.x;
    const SparseBatchCheck ck = a.d.chk[b];
    if (ck.err & kErrBadSlice) {
        batch_publish_verdict(a.status, a.matching_size, b, MISSLAP_BATCH_STATUS_BAD_SHAPE, -1);
        batch_condemn(a.d.s, 0, 0, 0);
        return;
    }
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
    const SparseViewRows<I, V, false> rows{a.d.w, a.d.offsets, s, a.d.row_start + (size_t)b * ((size_t)a.d.s.Ns + 1),
                                           bs.maximize, 0, 0, {}};
    batch_solve(bs, rows, ck.last_row + 1, ck.max_col + 1, ck.absmax_bits);
}

template <class I, class V>
struct SparseViewOutsideArgs {
    SparseViewArgs<I, V> d;  // d.s.Ns / Ms = Nmax / Mmax + Nmax (the carve), d.s.p0 / p0_ld the staged augmented prices,
                             // d.s.prices null
    const long long *sizes;  // [B][2] or null: n_b = sizes[b][1]
    int fast;
    int *status;             // [B]
    int *matching_size;      // [B] or null: always -1
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *prices;          // [B][Mmax] or null: the real columns
    double *outside_prices;  // [B][Nmax] or null
    int Mmax;                // the bound on the real columns
    long long p0_ld;         // of the caller's starting prices
};

// k_sparse_outside_solve (kernels_sparse_batch.hpp) on a view.
template <class I, class V>
__global__ __launch_bounds__(1024) void k_sparse_view_outside_solve(SparseViewOutsideArgs<I, V> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const SparseBatchCheck ck = a.d.chk[b];
    const int Nmax = a.d.s.Ns;
    double *po = a.prices ? a.prices + (size_t)b * (size_t)a.Mmax : nullptr;
    double *oo = a.outside_prices ? a.outside_prices + (size_t)b * (size_t)Nmax : nullptr;
    if (ck.err & kErrBadSlice) {
        batch_publish_verdict(a.status, a.matching_size, b, MISSLAP_BATCH_STATUS_BAD_SHAPE, -1);
        batch_condemn(a.d.s, 0, 0, 0);
        batch_outside_condemn(po, a.Mmax, oo, Nmax, tid, T);
        return;
    }
    const long long s = a.d.offsets[b];
    const long long nnz = a.d.offsets[b + 1] - s;
    const int own = sparse_outside_verdict(ck, nnz, a.sizes != nullptr, Nmax, a.Mmax, a.p0_ld, a.d.s.p0 != nullptr);
    const int code = batch_verdict(own, false, -1, 0, ck.bad_price);
    batch_publish_verdict(a.status, a.matching_size, b, code, -1);
    if (code != MISSLAP_BATCH_STATUS_OK) {
        const bool counted = code == MISSLAP_BATCH_STATUS_INFINITE_VALUE || code == MISSLAP_BATCH_STATUS_TOO_LARGE ||
                             code == MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW ||
                             code == MISSLAP_BATCH_STATUS_PRICE_NOT_FINITE || code == MISSLAP_BATCH_STATUS_PRICE_NEGATIVE;
        const long long mc = (long long)sparse_batch_count(ck.max_col) + ck.n;
        batch_condemn(a.d.s, counted ? ck.n : 0, counted ? (int)(mc < INT_MAX ? mc : INT_MAX) : 0,
                      counted ? nnz + ck.n : 0);
        batch_outside_condemn(po, a.Mmax, oo, Nmax, tid, T);
        return;
    }
    BatchSolveArgs bs = a.d.s;
    const int n = ck.n, m = ck.max_col < 0 ? 0 : ck.max_col + 1;
    if (a.fast) batch_fast_eps(bs, n);
    const double *O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
    const SparseViewRows<I, V, true> rows{a.d.w, a.d.offsets, s, a.d.row_start + (size_t)b * ((size_t)Nmax + 1),
                                          bs.maximize, m, n, {O, a.outside_ld ? 1 : 0}};
    batch_solve(bs, rows, n, m + n, ck.absmax_bits);
    batch_outside_outputs(s_raw, a.d.s, b, n, m, a.Mmax, Nmax, po, oo, tid, T);
}

}  // namespace misslap
