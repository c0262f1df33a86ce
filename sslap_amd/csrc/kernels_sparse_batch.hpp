// kernels_sparse_batch.hpp -- many small SPARSE problems, one workgroup per problem for its whole solve
// (misslap_solve_sparse_batch, include/misslap.h; the host side is abi_sparse_batch.hpp), and the same solve with a
// verdict per problem, on the packed arrays or on a view of them (misslap_solve_sparse_batch_status / _outside and their
// _view forms; abi_sparse_batch_status.hpp).
//
// ONE kernel family -- the check pass, the row source of batch_solve and the two solve kernels -- templated on an entry
// source Src, which says how entry g is read (row(g), col(g), value(g)) and whether the host has checked the offsets
// (Src::kHostOffsets).  Two sources:
//   SparsePacked      loc [nnz][2] int32 and val [nnz] float64, read as loc[2 * g], loc[2 * g + 1], val[g]; the host
//                     has validated the offsets (sparse_batch_offsets, abi_sparse_batch.hpp).
//   SparseView<I, V>  what a device pipeline left behind: int32 or int64 indices with run-time strides, float64 or
//                     float32 values, and offsets that only the device has seen.  What that changes:
//     ACCESS   entry g is row loc[g * se], column loc[g * se + sc], value val[g]; offsets are formed in 64 bits.  An
//              int64 index outside the int32 range SATURATES to INT_MIN / INT_MAX as it is read, before any check sees
//              it: a value at or below -2^31 is a negative index whatever its low word is, one at or above 2^31 is
//              beyond every carve, and nothing is ever truncated into a valid index.  A float32 value is widened to
//              double as it is read (exact); everything downstream is the float64 arithmetic of the packed source.
//     OFFSETS  nobody checked them on the host (!kHostOffsets).  A problem whose slice is not
//              0 <= offsets[b] <= offsets[b + 1] <= nnz, or holds 2^31 - 1 entries or more, gets kErrBadSlice from the
//              check pass before anything of loc / val is read; the solve kernels turn that into
//              MISSLAP_BATCH_STATUS_BAD_SHAPE ahead of every other check, and the guard skips the problem.
//     ROW STARTS  in a block of Ns + 1 ints per problem in both modes (with host-checked offsets the plain mode keeps
//              them at offsets[b] + b of an nnz + B array, which races between problems once the offsets are not
//              monotone); every index written is clamped to the block.  sparse_row_starts is the one place that knows.
// Apart from that every verdict, output and record is the same for both sources, bit for bit.
//
// The round loop is batch_solve and the row source is its list row source (ListBatchRows, kernels_batch_solve.hpp, which
// has the rules of the bid, the eCE test and the objective); this file has the check pass and the runs that the row
// source walks (SparseRuns).  Problem b is the entries offsets[b] .. offsets[b + 1] of the caller's loc / val, in their
// STORED order, and row i of it is the run row_start[i] .. row_start[i + 1] that the check pass found.
//
// The outside mode (misslap_solve_sparse_batch_outside; the Out instances below): row i of problem b also holds one
// virtual entry (i, m_b + i), stored LAST in its row, whose value is the row's outside value -- a private object that
// only row i can bid for, so a row may stay unmatched and a row may have no stored entry at all.  n_b is sizes[b][1] (without sizes the last stored row + 1), m_b the
// largest real column + 1; the problem solved is the n_b x (m_b + n_b) packed problem, the round loop is batch_solve
// unchanged on a carve of Mmax + Nmax objects.  The row starts live in a block of Nmax + 1 ints per problem (n_b may
// exceed nnz_b, so the plain mode's nnz_b + 1 slots do not fit) and a row gap is legal: the check pass fills the starts
// of the empty rows too.  The row source presents the virtual entry (tie key len, above every stored index), the check
// pass folds the outside values into C = max |v| and the non-finite flag, and the solve kernel rewrites the outputs
// behind batch_solve as the ELL outside mode does (batch_outside_outputs).
#pragma once

namespace misslap {

constexpr int kSparseBatchMaxDim = MISSLAP_SPARSE_BATCH_MAX_DIM;

// per problem, from the check pass ahead of the solve
struct SparseBatchCheck {
    unsigned long long absmax_bits;  // max |v| over the problem's values, as bits
    int max_row;    // max row index over every entry (the reference's N of :594 is this, without + 1)
    int max_col;    // max column index over every entry
    int last_row;   // row of the last stored entry (AuctionSolver's N - 1 with rows ascending, :209)
    int err;        // kErrColNegative / kErrRowsUnsorted / kErrRowGap / kErrNonFinite, as k_ingest_rows / _vals set them
    int bad_price;  // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
    int n;          // the outside mode: n_b = sizes[b][1] clamped to -1 .. INT_MAX, without sizes last_row + 1; else 0
};

constexpr int kErrBadSlice = 1 << 12;  // SparseBatchCheck::err without host-checked offsets: the slice is unusable

// The packed arrays as misslap_solve_sparse_batch and its status / outside forms take them.
struct SparsePacked {
    static constexpr bool kHostOffsets = true;
    const int *loc;     // [nnz][2]
    const double *val;  // [nnz]

    __device__ __forceinline__ int row(long long g) const { return loc[2 * g]; }
    __device__ __forceinline__ int col(long long g) const { return loc[2 * g + 1]; }
    __device__ __forceinline__ double value(long long g) const { return val[g]; }
};

// The packed arrays as the caller's view presents them.
template <class I, class V>
struct SparseView {
    static constexpr bool kHostOffsets = false;
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

// Where the row starts (local indices) of problem b, whose entries begin at s, live in row_start.  Plain mode with
// host-checked offsets: nnz_b + 1 slots at s + b of an nnz + B array (monotone offsets keep the problems apart).
// Otherwise -- the outside mode, where n_b may exceed nnz_b, and offsets nobody checked -- a block of Ns + 1 ints.
template <class Src, bool Out, class T>
__device__ __forceinline__ T *sparse_row_starts(T *row_start, long long s, int b, int Ns) {
    if constexpr (Src::kHostOffsets && !Out) return row_start + s + b;
    else return row_start + (size_t)b * ((size_t)Ns + 1);
}

template <class Src>
struct SparseBatchArgs {
    BatchSolveArgs s;             // Ns / Ms: the largest n_b / n_cols (the LDS carve; status modes: the caller's bound)
    Src w;
    const long long *offsets;     // [B + 1]
    const int *row_start;         // where sparse_row_starts finds problem b's
    const SparseBatchCheck *chk;  // [B]
};

template <class Src>
struct SparseCheckArgs {
    Src w;
    const long long *offsets, *sizes;  // sizes: [B][2] or null (read in the outside mode only)
    const double *p0;
    long long p0_ld;
    int *row_start;  // where sparse_row_starts finds problem b's
    SparseBatchCheck *out;
    const double *outside;  // the outside mode: [B] (outside_ld == 0) or [B][outside_ld], outside_ld >= Nmax
    long long outside_ld;
    double *aug;            // the outside mode: [B][aug_ld] or null (no starting prices)
    long long aug_ld;       // Mmax + Nmax
    int Nmax, Mmax;         // the bounds on the rows and on the real columns (no row-start block, not in the outside
                            // mode: unread)
    long long nnz;          // the packed entries of the whole call (read without host-checked offsets only)
};

// Check pass, one workgroup per problem: the checks of AuctionSolver.__init__ (k_ingest_rows / k_ingest_vals with the
// same rules), the maxima of from_sparse (:594-595) and of the guard (n_true, m_true), C = max |v|, the starting prices,
// and the row starts rs[0 .. rs_hi], which the calling kernel places (sparse_row_starts).  Without host-checked offsets
// a problem with an unusable slice leaves only its record.  Plain mode: a row start is written only where the rows seen
// so far are gap-free (r <= local index) and within rs_hi, so a malformed problem never writes outside its own slots.
// Out (the outside mode): rs is the problem's own block of Ns + 1 row starts (rs_hi = Ns).  The thread that sees the row
// change rp -> r at local index k fills rs[rp + 1 .. r] = k (the rows rp + 1 .. r - 1 are empty), thread 0 fills
// rs[last_row + 1 .. n_b] = nnz_b; every index written is clamped to 0 .. Ns, so a malformed or oversized problem stays
// within its block.  No row gap is reported.  The outside values of the rows < min(n_b, Ns) (outside[b] with
// outside_ld == 0, else outside[b * outside_ld + i]; outside_ld >= Ns) count as an entry's value does, and with starting
// prices the augmented start [p0[:m_b], zeros(n_b)] is staged at aug[b * aug_ld ..] (aug_ld = Ms + Ns) -- only where the
// verdict can still be 0 (no error, 1 <= n_b <= Ns, m_b <= Ms and m_b <= p0_ld, so m_b + n_b <= aug_ld).
template <class Src, bool Out>
__device__ __forceinline__ void sparse_batch_check(const SparseCheckArgs<Src> &a, int *rs, int rs_hi) {
    const Src &w = a.w;
    const double *p0 = a.p0;
    const long long p0_ld = a.p0_ld;
    const int Ns = a.Nmax, Ms = a.Mmax;  // (read in the outside mode only)
    const int b = blockIdx.x;
    const long long s = a.offsets[b], e = a.offsets[b + 1];
    if constexpr (!Src::kHostOffsets) {
        if (!sparse_view_slice_ok(s, e, a.nnz)) {  // (uniform)
            if (threadIdx.x == 0) {
                SparseBatchCheck c{};
                c.max_row = INT_MIN;
                c.max_col = INT_MIN;
                c.last_row = -1;
                c.err = kErrBadSlice;
                a.out[b] = c;
            }
            return;
        }
    }
    const int nnz = (int)(e - s);  // (fewer than 2^31 - 1 entries: the host's check of the offsets, or the slice test)
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
        const double *ov = a.outside;
        const long long ov_ld = a.outside_ld;
        if (a.sizes) {
            const long long v = a.sizes[2 * b + 1];
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
                const int hi = r < rs_hi ? r : rs_hi;
                for (int i = rp < 0 ? 0 : rp + 1; i <= hi; ++i) rs[i] = k;
            } else {
                if (r != rp + 1 || r > last_row) err |= kErrRowGap;
                else if (r <= k && r <= rs_hi) rs[r] = k;  // (r > k implies a gap earlier in the problem)
            }
        }
    }
    if (err) atomicOr(&s_err, err);
    if (mr != INT_MIN) atomicMax(&s_maxr, mr);
    if (mc != INT_MIN) atomicMax(&s_maxc, mc);
    if (am) atomicMax(&s_abs, am);
    __syncthreads();
    // m_b = n_cols (0 without an entry; only meaningful without errors), in 64 bits: a column may be INT_MAX
    const long long m = s_maxc < 0 ? 0 : (long long)s_maxc + 1;
    if (p0 && s_err == 0 && m > 0)
        batch_check_prices(p0 + (size_t)b * (size_t)p0_ld, (int)(m < p0_ld ? m : p0_ld), &s_badp);
    if constexpr (Out) {
        if (p0 && s_err == 0 && n >= 1 && n <= Ns && m <= (long long)Ms && m <= p0_ld) {
            const double *src = p0 + (size_t)b * (size_t)p0_ld;
            double *dst = a.aug + (size_t)b * (size_t)a.aug_ld;
            for (int j = threadIdx.x; j < (int)m + n; j += blockDim.x) dst[j] = j < (int)m ? src[j] : 0.0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (Out) {
            const int hi = n < rs_hi ? n : rs_hi;
            for (int i = last_row < 0 ? 0 : (last_row < rs_hi ? last_row + 1 : rs_hi + 1); i <= hi; ++i) rs[i] = nnz;
        } else {
            if (last_row >= 0 && last_row < nnz && last_row < rs_hi) rs[last_row + 1] = nnz;  // :47
        }
        SparseBatchCheck c;
        c.absmax_bits = s_abs;
        c.max_row = s_maxr;
        c.max_col = s_maxc;
        c.last_row = last_row;
        c.err = s_err;
        c.bad_price = s_badp;
        c.n = n;
        a.out[b] = c;
    }
}

// The check kernel of every sparse call.  It places the problem's row starts: rs[0 .. hi] may be written.
template <class Src, bool Out>
__global__ __launch_bounds__(256) void k_sparse_batch_check(SparseCheckArgs<Src> a) {
    const int b = blockIdx.x;
    const long long s = a.offsets[b];
    const int hi = Src::kHostOffsets && !Out ? (int)(a.offsets[b + 1] - s) : a.Nmax;  // (nnz_b + 1 slots, or the block)
    sparse_batch_check<Src, Out>(a, sparse_row_starts<Src, Out>(a.row_start, s, b, a.Nmax), hi);
}

// The runs of the sparse row source (ListBatchRows, kernels_batch_solve.hpp): problem b's entries from global index s,
// row i the run s + rs[i] .. s + rs[i + 1] that the check pass found, every stored entry an entry (no holes).  It
// serves both entry sources.  n: the rows whose virtual entries the outside mode counts into the meta record, else 0.
template <class Src>
struct SparseRuns {
    using Col = int;
    static constexpr bool kHoles = false;
    Src w;
    const long long *offsets;
    long long s;
    const int *rs;
    int n;

    __device__ __forceinline__ long long start(int i) const { return s + rs[i]; }
    __device__ __forceinline__ int len(int i) const { return rs[i + 1] - rs[i]; }
    __device__ __forceinline__ int col(long long g) const { return w.col(g); }
    __device__ __forceinline__ double value(long long g) const { return w.value(g); }
    __device__ __forceinline__ int64_t count() const { return (int64_t)(offsets[blockIdx.x + 1] - s) + (int64_t)n; }
};

template <class Src, bool Out>
using SparseBatchRows = ListBatchRows<SparseRuns<Src>, Out>;

// the all-or-nothing call (misslap_solve_sparse_batch): the host has read the check records and found every problem fit
__global__ __launch_bounds__(1024) void k_sparse_batch_solve(SparseBatchArgs<SparsePacked> a) {
    const int b = blockIdx.x;
    const SparseBatchCheck ck = a.chk[b];
    const long long s = a.offsets[b];
    const SparseBatchRows<SparsePacked, false> rows{
        {a.w, a.offsets, s, sparse_row_starts<SparsePacked, false>(a.row_start, s, b, a.s.Ns), 0}, a.s.maximize, 0, {}};
    batch_solve(a.s, rows, ck.last_row + 1, ck.max_col + 1, ck.absmax_bits);
}

// ---- status mode (misslap_solve_sparse_batch_status, _status_view): a verdict per problem instead of all or nothing

template <class Src>
struct SparseStatusArgs {
    SparseBatchArgs<Src> d;  // d.s.Ns / Ms = sol_ld / prices_ld: the caller's bound on every problem (dims), the LDS carve
    const long long *sizes;  // [B][2] or null: from_sparse's `size` of each problem (N = sizes[b][1], auction_.pyx:592)
    const int *card;         // [B] the guard's cardinalities (-1: not matched), or null: no guard in this call
    int fast;                // eps_start = 1 / N of each problem (:614-615)
    int *status;             // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;      // [B] or null: the guard's cardinality, -1 where it did not run
};

// a check record's maximum as a count: max + 1, 0 without a non-negative index, saturated at INT_MAX
__device__ __forceinline__ int sparse_batch_count(int mx) { return mx < 0 ? 0 : (mx == INT_MAX ? INT_MAX : mx + 1); }

// The sparse checks of a verdict ahead of the starting prices, in the order of misslap_solve_sparse_batch
// (abi_sparse_batch.hpp: pre_guard_error, the guard, AuctionSolver.__init__, the cap, the leading dimensions);
// batch_verdict adds the prices.  N: the reference's N of :592 / :594; card: the guard's cardinality, -1 without one.
__device__ __forceinline__ int sparse_batch_verdict(const SparseBatchCheck &c, long long nnz, long long N, int fast,
                                                    int card, int Ns, int Ms, long long p0_ld, bool has_p0) {
    if (nnz == 0) return MISSLAP_BATCH_STATUS_NO_ENTRIES;
    if (fast && N == 0) return MISSLAP_BATCH_STATUS_DIVISION_BY_ZERO;
    if (nnz < N) return MISSLAP_BATCH_STATUS_TOO_FEW_VALUES;
    if (card >= 0 && card < c.max_row + 1) return MISSLAP_BATCH_STATUS_INFEASIBLE;  // (matched: max_row + 1 <= the cap)
    if (c.last_row < 0 || (c.err & kErrColNegative)) return MISSLAP_BATCH_STATUS_NEGATIVE_INDEX;
    if (c.err & kErrRowsUnsorted) return MISSLAP_BATCH_STATUS_ROWS_UNSORTED;
    if (c.err & kErrRowGap) return MISSLAP_BATCH_STATUS_ROW_GAP;
    if (c.err & kErrNonFinite) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    // (from here on rows ascend from 0 without a gap and no index is negative: n = last_row + 1 = max_row + 1 <= nnz)
    // (Ns, Ms <= MISSLAP_SPARSE_BATCH_MAX_DIM: a column whose + 1 does not fit an int32 is beyond Ms too)
    if (c.last_row >= Ns || c.max_col >= Ms) return MISSLAP_BATCH_STATUS_TOO_LARGE;
    if (has_p0 && c.max_col >= p0_ld) return MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW;
    return MISSLAP_BATCH_STATUS_OK;
}

// k_sparse_batch_solve with the verdict formed here, from what the check pass and the guard left on the device.  A
// condemned problem's workgroup writes the defined outputs and leaves before any LDS state exists and before anything of
// loc, val or the row starts is read: an index beyond the carve never reaches the price array.  The others run the same
// batch_solve on the same row source.  Without host-checked offsets an unusable slice is BAD_SHAPE before anything
// else: its offsets are not read again and its record is all zeros.
template <class Src>
__global__ __launch_bounds__(1024) void k_sparse_batch_solve_status(SparseStatusArgs<Src> a) {
    const int b = blockIdx.x;
    const SparseBatchCheck ck = a.d.chk[b];
    if constexpr (!Src::kHostOffsets) {
        if (ck.err & kErrBadSlice) {
            batch_publish_verdict(a.status, a.matching_size, b, MISSLAP_BATCH_STATUS_BAD_SHAPE, -1);
            batch_condemn(a.d.s, 0, 0, 0);
            return;
        }
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
    const SparseBatchRows<Src, false> rows{
        {a.d.w, a.d.offsets, s, sparse_row_starts<Src, false>(a.d.row_start, s, b, a.d.s.Ns), 0}, bs.maximize, 0, {}};
    batch_solve(bs, rows, ck.last_row + 1, ck.max_col + 1, ck.absmax_bits);
}

// ---- outside mode (misslap_solve_sparse_batch_outside, _outside_view): an outside option per row, for partial assignments

template <class Src>
struct SparseOutsideArgs {
    SparseBatchArgs<Src> d;  // d.s.Ns / Ms = Nmax / Mmax + Nmax (the carve), d.s.p0 / p0_ld the staged augmented prices,
                             // d.s.prices null
    const long long *sizes;  // [B][2] or null: n_b = sizes[b][1] (sizes[b][0] is not read)
    int fast;                // eps_start = 1 / n_b of each problem
    int *status;             // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;      // [B] or null: always -1 (no guard in this mode)
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *prices;          // [B][Mmax] or null: the real columns
    double *outside_prices;  // [B][Nmax] or null
    int Mmax;                // the bound on the real columns
    long long p0_ld;         // of the caller's starting prices (the PRICES_TOO_NARROW check)
};

// The checks of an outside-mode verdict ahead of the starting prices, in their order (include/misslap.h); batch_verdict
// adds the prices.  A row gap is legal, a problem without entries too once sizes names its rows; TOO_FEW_VALUES,
// EMPTY_ROW, INFEASIBLE, DIVISION_BY_ZERO, ROW_GAP and BAD_OUTSIDE never occur.
__device__ __forceinline__ int sparse_outside_verdict(const SparseBatchCheck &c, long long nnz, bool has_sizes, int Ns,
                                                      int Ms, long long p0_ld, bool has_p0) {
    if (nnz == 0 && !has_sizes) return MISSLAP_BATCH_STATUS_NO_ENTRIES;
    if (c.err & kErrColNegative) return MISSLAP_BATCH_STATUS_NEGATIVE_INDEX;
    if (c.err & kErrRowsUnsorted) return MISSLAP_BATCH_STATUS_ROWS_UNSORTED;
    // (from here on no index is negative and the rows ascend: last_row = max_row >= -1)
    if (has_sizes && (c.n < 1 || (long long)c.n < (long long)c.last_row + 1)) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (c.err & kErrNonFinite) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    if (c.n > Ns || sparse_batch_count(c.max_col) > Ms) return MISSLAP_BATCH_STATUS_TOO_LARGE;
    if (has_p0 && sparse_batch_count(c.max_col) > p0_ld) return MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve of the outside mode: the verdict from what the check pass left on the device, batch_solve on the
// n x (m + n) problem, then the outputs in the caller's terms (batch_outside_outputs).  A condemned problem's workgroup
// writes the defined outputs and leaves before any LDS state exists and before a row start, a loc or a val of its
// problem is read.  Its record holds n_b, m_b + n_b and nnz_b + n_b where the verdict is one behind which they are
// defined (3, 13, 14, 5, 6), and zeros otherwise.  Without host-checked offsets an unusable slice is BAD_SHAPE before
// anything else, as in the status solve.
template <class Src>
__global__ __launch_bounds__(1024) void k_sparse_outside_solve(SparseOutsideArgs<Src> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const SparseBatchCheck ck = a.d.chk[b];
    const int Nmax = a.d.s.Ns;
    double *po = a.prices ? a.prices + (size_t)b * (size_t)a.Mmax : nullptr;
    double *oo = a.outside_prices ? a.outside_prices + (size_t)b * (size_t)Nmax : nullptr;
    if constexpr (!Src::kHostOffsets) {
        if (ck.err & kErrBadSlice) {
            batch_publish_verdict(a.status, a.matching_size, b, MISSLAP_BATCH_STATUS_BAD_SHAPE, -1);
            batch_condemn(a.d.s, 0, 0, 0);
            batch_outside_condemn(po, a.Mmax, oo, Nmax, tid, T);
            return;
        }
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
    const SparseBatchRows<Src, true> rows{
        {a.d.w, a.d.offsets, s, sparse_row_starts<Src, true>(a.d.row_start, s, b, Nmax), n}, bs.maximize, m,
        {O, a.outside_ld ? 1 : 0}};
    batch_solve(bs, rows, n, m + n, ck.absmax_bits);
    batch_outside_outputs(s_raw, a.d.s, b, n, m, a.Mmax, Nmax, po, oo, tid, T);
}

}  // namespace misslap
