// kernels_ell_batch.hpp -- many small sparse problems given as padded candidate lists (ELL), one workgroup per problem
// for its whole solve (misslap_solve_ell_batch, include/misslap.h; the host side of both modes is abi_ell_batch.hpp).
//
// The round loop is batch_solve and the row source is its list row source (ListBatchRows, kernels_batch_solve.hpp);
// this file has the check pass, the runs that the row source walks (EllRuns) and the solve with its verdict.  The input
// is what a top-k, a gating step or a nearest-neighbour search leaves on the device: cols[B][N][K] (int32 or int64: the
// kernels' I) and vals[B][N][K] (double or float: V, widened where it is used by dense_widen, exact).  Problem b is rows 0 .. n_b - 1 of its slice; slot (i, k) is an entry iff cols[b][i][k] >= 0, a
// negative column is a hole in any position and the value stored in a hole is never interpreted.  The result is that of
// the packed problem with the holes dropped (rows in order, within a row in slot order) under
// from_sparse(loc_b, val_b, size=(m_b, n_b)): dropping holes keeps the order of the entries, and the bid's tie key is
// only ever compared (top2_wave_reduce), so the slot index k serves as the stored index.  In the bid lane l holds slots
// l, l + 64, ... of the row, so both loads are unit-stride.
//
// The outside mode (misslap_solve_ell_batch_outside; the <.., true> instances below): row i of problem b also holds one
// virtual entry (i, m_b + i), stored LAST in its row, whose value is the row's outside value -- a private object that
// only row i can bid for, so a row may stay unmatched.  The problem solved is the n_b x (m_b + n_b) packed problem; the
// round loop is batch_solve unchanged, on a carve of Mmax + N objects.  The row source presents the virtual entry (tie
// key K, above every slot), the check pass folds the outside values into C = max |v| and the non-finite flag and never
// reports an empty row, and the solve kernel rewrites the outputs behind batch_solve: an object >= m_b becomes -1 in
// sol, price[0 .. m_b) are the real prices and price[m_b .. m_b + n_b) the outside prices.
#pragma once

namespace misslap {

// per problem, from the check pass ahead of the guard and the solve
struct EllBatchCheck {
    unsigned long long nvalid;       // entries (valid slots) of rows 0 .. n - 1
    unsigned long long absmax_bits;  // max |v| over them, as bits
    int n;                           // rows[b], 0 where it lies outside 1 .. N (nothing of the problem is read then)
    int empty_row;                   // first row without an entry (INT_MAX: none)
    int max_col;                     // max column over the entries (-1: none), INT_MAX where it does not fit below that
    int nonfinite;                   // an entry's value is a NaN or an infinity
    int bad_price;                   // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
    int pad;
};

struct EllBatchArgs {
    BatchSolveArgs s;          // Ns / Ms = N / Mmax: the LDS carve, sol_ld and prices_ld
    const void *cols;          // [B][N][K] of the kernel's I
    const void *vals;          // [B][N][K] of the kernel's V
    long long N, K;
    const EllBatchCheck *chk;  // [B]
    const int *card;           // [B] the guard's cardinalities (-1: not matched), or null: no guard in this call
    int fast;                  // eps_start = 1 / n_b of each problem
    int *status;               // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;        // [B] or null
};

// What the check pass takes.  The plain mode leaves the outside fields unread.
struct EllCheckArgs {
    const void *cols, *vals;
    long long N, K;
    const int *rows;
    const double *p0;
    long long p0_ld;
    EllBatchCheck *out;
    const double *outside;  // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *aug;            // [B][aug_ld] or null (no starting prices)
    long long aug_ld;       // Mmax + N
    int Ms;                 // Mmax: the bound on the real columns
};

// Check pass, one workgroup per problem, a wavefront per row: the entries per row and in all, the first empty row, the
// largest column (compared in the index's own width: an int64 column at or above 2^31 is too large, not wrapped), NaN /
// infinity and C = max |v| among the entries only, and the starting prices of the problem's columns.
// Out (the outside mode): the outside value of every row < n_b counts as an entry's value does (outside[b] with
// outside_ld == 0, else outside[b * outside_ld + i]), no row is empty, and with starting prices the problem's augmented
// starting prices [p0[:m_b], zeros(n_b)] are staged at aug[b * aug_ld ..] (aug_ld = Ms + N) for batch_solve to load --
// only where the real columns fit both Ms and p0_ld, i.e. where the verdict can still be 0 (m_b + n_b <= aug_ld then).
template <class I, class V, bool Out>
__global__ __launch_bounds__(256) void k_ell_batch_check(EllCheckArgs a) {
    const I *cols = static_cast<const I *>(a.cols);
    const V *vals = static_cast<const V *>(a.vals);
    const long long N = a.N, K = a.K;
    const double *p0 = a.p0;
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int n = a.rows ? a.rows[b] : (int)N;
    if (n < 1 || n > N) n = 0;
    const size_t base = (size_t)b * (size_t)N * (size_t)K;
    __shared__ unsigned long long s_cnt, s_abs;
    __shared__ int s_empty, s_bad, s_maxc, s_badp;
    if (threadIdx.x == 0) {
        s_cnt = 0;
        s_abs = 0;
        s_empty = INT_MAX;
        s_bad = 0;
        s_maxc = -1;
        s_badp = 0;
    }
    __syncthreads();
    unsigned long long cnt = 0, am = 0;
    int bad = 0;
    I mc = -1;
    for (int r = wave; r < n; r += nw) {
        const size_t g0 = base + (size_t)r * (size_t)K;
        int rc = 0;
        for (long long q = lane; q < K; q += kWave) {
            const I c = cols[g0 + q];
            if (c < 0) continue;
            const unsigned long long bits =
                (unsigned long long)__double_as_longlong(dense_widen(vals[g0 + q])) & 0x7fffffffffffffffull;
            ++rc;
            am = bits > am ? bits : am;
            bad |= bits >= 0x7ff0000000000000ull;
            mc = c > mc ? c : mc;
        }
        for (int off = 32; off >= 1; off >>= 1) rc += __shfl_xor(rc, off);
        if constexpr (Out) {
            if (lane == 0) {
                const size_t at = a.outside_ld ? (size_t)b * (size_t)a.outside_ld + (size_t)r : (size_t)b;
                const unsigned long long bits =
                    (unsigned long long)__double_as_longlong(a.outside[at]) & 0x7fffffffffffffffull;
                am = bits > am ? bits : am;
                bad |= bits >= 0x7ff0000000000000ull;
            }
        } else {
            if (rc == 0 && lane == 0) atomicMin(&s_empty, r);
        }
        cnt += (unsigned long long)rc;  // (uniform; lane 0's copy is added below)
    }
    if (lane == 0) atomicAdd(&s_cnt, cnt);
    if (am) atomicMax(&s_abs, am);
    if (bad) atomicOr(&s_bad, 1);
    if (mc >= 0) atomicMax(&s_maxc, mc >= (I)INT_MAX ? INT_MAX : (int)mc);
    __syncthreads();
    if (p0 && s_maxc >= 0) {
        const long long m = (long long)s_maxc + 1;
        batch_check_prices(p0 + (size_t)b * (size_t)a.p0_ld, (int)(m < a.p0_ld ? m : a.p0_ld), &s_badp);
    }
    if constexpr (Out) {
        const long long m = (long long)s_maxc + 1;
        if (p0 && m <= (long long)a.Ms && m <= a.p0_ld) {
            const double *src = p0 + (size_t)b * (size_t)a.p0_ld;
            double *dst = a.aug + (size_t)b * (size_t)a.aug_ld;
            for (int j = threadIdx.x; j < (int)m + n; j += blockDim.x) dst[j] = j < (int)m ? src[j] : 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        EllBatchCheck r;
        r.nvalid = s_cnt;
        r.absmax_bits = s_abs;
        r.n = n;
        r.empty_row = s_empty;
        r.max_col = s_maxc;
        r.nonfinite = s_bad;
        r.bad_price = s_badp;
        r.pad = 0;
        a.out[b] = r;
    }
}

// The runs of the ELL row source (ListBatchRows, kernels_batch_solve.hpp): problem b's slices C / A (at
// (size_t)b * N * K, formed in 64 bits), row i the K slots from i * K of them (an int: the host caps N * K at
// INT_MAX - 128), a negative column a hole.  Every valid column is below the carve's Ms once the verdict is 0, so an
// int64 column narrows safely once it is known to be an entry.
template <class I, class V>
struct EllRuns {
    using Col = I;
    static constexpr bool kHoles = true;
    const I *C;
    const V *A;
    int K;
    unsigned long long nvalid;  // the entries of the problem, in the outside mode with its n virtual ones

    __device__ __forceinline__ int start(int i) const { return i * K; }
    __device__ __forceinline__ int len(int) const { return K; }
    __device__ __forceinline__ I col(int g) const { return C[g]; }
    __device__ __forceinline__ V value(int g) const { return A[g]; }
    __device__ __forceinline__ int64_t count() const { return (int64_t)nvalid; }
};

template <class I, class V, bool Out = false>
using EllBatchRows = ListBatchRows<EllRuns<I, V>, Out>;

// The ELL checks of a verdict ahead of the guard and the starting prices, in their order (include/misslap.h);
// batch_verdict adds those two.
__device__ __forceinline__ int ell_batch_verdict(const EllBatchCheck &c, int Ms, long long p0_ld, bool has_p0) {
    if (c.n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (c.empty_row != INT_MAX) return MISSLAP_BATCH_STATUS_EMPTY_ROW;
    if (c.nonfinite) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    if (c.max_col >= Ms) return MISSLAP_BATCH_STATUS_TOO_LARGE;
    if (has_p0 && c.max_col >= p0_ld) return MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve with the verdict formed here, from what the check pass and the guard left on the device.  A condemned
// problem's workgroup writes the defined outputs and leaves before any LDS state exists and before anything of cols or
// vals is read: a column beyond the carve never reaches the price array.  The others run batch_solve on the ELL source.
template <class I, class V>
__global__ __launch_bounds__(1024) void k_ell_batch_solve(EllBatchArgs a) {
    const int b = blockIdx.x;
    const EllBatchCheck ck = a.chk[b];
    const int card = a.card ? a.card[b] : -1;
    const int own = ell_batch_verdict(ck, a.s.Ms, a.s.p0_ld, a.s.p0 != nullptr);
    const int code = batch_verdict(own, a.card != nullptr, card, ck.n, ck.bad_price);
    batch_publish_verdict(a.status, a.matching_size, b, code, card);
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(a.s, ck.n, sparse_batch_count(ck.max_col), (long long)ck.nvalid);
        return;
    }
    BatchSolveArgs bs = a.s;
    if (a.fast) batch_fast_eps(bs, ck.n);
    const size_t base = (size_t)b * (size_t)a.N * (size_t)a.K;
    const I *C = static_cast<const I *>(a.cols) + base;
    const V *A = static_cast<const V *>(a.vals) + base;
    // (the two slice pointers as opaque scalars: left to itself the compiler also keeps base * sizeof(I) and
    // base * sizeof(V) alive for the objective's scalar re-walk, and those four registers are the ones that spill)
    asm volatile("" : "+s"(C), "+s"(A));
    const EllBatchRows<I, V> rows{{C, A, (int)a.K, ck.nvalid}, bs.maximize, ck.max_col + 1, {}};
    batch_solve(bs, rows, ck.n, ck.max_col + 1, ck.absmax_bits);
}


struct EllOutsideArgs {
    EllBatchArgs e;          // s.Ms = Mmax + N (the carve), s.p0 / p0_ld the staged augmented prices, s.prices null
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *prices;          // [B][Mmax] or null: the real columns
    double *outside_prices;  // [B][N] or null
    int Mmax;                // the bound on the real columns
    long long p0_ld;         // of the caller's starting prices (the PRICES_TOO_NARROW check)
};

// The solve of the outside mode: the verdict without EMPTY_ROW and INFEASIBLE (neither can occur), batch_solve on the
// n x (m + n) problem, then the outputs in the caller's terms (batch_outside_outputs).
template <class I, class V>
__global__ __launch_bounds__(1024) void k_ell_outside_solve(EllOutsideArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const EllBatchCheck ck = a.e.chk[b];
    const int own = ell_batch_verdict(ck, a.Mmax, a.p0_ld, a.e.s.p0 != nullptr);
    const int code = batch_verdict(own, false, -1, ck.n, ck.bad_price);
    batch_publish_verdict(a.e.status, a.e.matching_size, b, code, -1);
    const int N = (int)a.e.N;
    double *po = a.prices ? a.prices + (size_t)b * (size_t)a.Mmax : nullptr;
    double *oo = a.outside_prices ? a.outside_prices + (size_t)b * (size_t)N : nullptr;
    if (code != MISSLAP_BATCH_STATUS_OK) {
        const long long mc = (long long)sparse_batch_count(ck.max_col) + ck.n;
        batch_condemn(a.e.s, ck.n, (int)(mc < INT_MAX ? mc : INT_MAX), (long long)ck.nvalid + ck.n);
        batch_outside_condemn(po, a.Mmax, oo, N, tid, T);
        return;
    }
    BatchSolveArgs bs = a.e.s;
    if (a.e.fast) batch_fast_eps(bs, ck.n);
    const size_t base = (size_t)b * (size_t)a.e.N * (size_t)a.e.K;
    const I *C = static_cast<const I *>(a.e.cols) + base;
    const V *A = static_cast<const V *>(a.e.vals) + base;
    asm volatile("" : "+s"(C), "+s"(A));
    const int n = ck.n, m = ck.max_col + 1;
    const double *O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
    const EllBatchRows<I, V, true> rows{{C, A, (int)a.e.K, ck.nvalid + (unsigned long long)n}, bs.maximize, m,
                                        {O, a.outside_ld ? 1 : 0}};
    batch_solve(bs, rows, n, m + n, ck.absmax_bits);
    batch_outside_outputs(s_raw, a.e.s, b, n, m, a.Mmax, N, po, oo, tid, T);
}

}  // namespace misslap
