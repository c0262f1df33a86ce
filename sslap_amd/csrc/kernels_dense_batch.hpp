// kernels_dense_batch.hpp -- many small dense problems, one workgroup per problem for its whole solve
// (misslap_solve_dense_batch and the stream-ordered calls with a verdict per problem, include/misslap.h; the host side
// is abi_dense_batch.hpp and abi_dense_batch_status.hpp).
//
// The round loop is batch_solve (kernels_batch_solve.hpp); this file has the check pass, the dense row source and the
// solve kernels, each once: k_dense_batch_check<T, Lay, Out>, DenseBatchRows<T, Lay, Out>, k_dense_batch_solve<T>,
// k_dense_batch_solve_status<T, Lay> and k_dense_outside_solve<T, Lay>; behind them, as a launch of its own, the reverse
// finish k_dense_reverse_finish<T, Lay, Out> (at the end of the file).  Values are read from the caller's stack in
// global memory, where a small problem stays in L2:
//   BID      lanes scan the row in column order (lane l holds columns l, l + 64, ...), staged in registers with up to
//            kDenseBatchCols loads in flight; the object is the winning column r.g.
//   eCE      every column is stored once, so choice_cost -- never reset per row in the reference -- is the cost of the
//            row's own column.
//   get_obj  the selected values are gathered into LDS, then one lane adds them in row order.
//
// Element type T (double, float, F16, Bf16: misslap_options.mat_dtype).  The rows are read in the caller's type, every
// value is widened to double where it is used (dense_widen, exact), and batch_solve only ever sees doubles.
//
// Layout Lay: where element (b, i, j) lies.  DenseContig is the compact stack: problem stride N * M, row stride M and
// column step 1, all known at compile time, so it holds nothing.  DenseView<Fin> holds DenseStrides: the element lies
// at mat[b * sB + i * sN + j * sM] for run-time strides >= 0 -- a transposed view, a slice of a wider buffer, an
// expanded matrix (sB = 0).  Every entry plays the role it plays in the compact copy, so the results are those of the
// copy bit for bit; offsets are formed in 64 bits, loads are one element each, and only elements of the view are read.
// A view whose rows run along the unit stride (sN == 1) also has a second bid mapping, bid_lanes below, for rounds of
// many bidders.
//
// Entry rule, the layout's second fact.  DenseContig and DenseView<false> take the reference's "v >= 0".
// DenseView<true> (MISSLAP_DENSE_ENTRIES_FINITE in misslap_options.mat_dtype) is a signed cost stack: an element is an
// entry iff it is not a NaN in its own type, so negative values, -0.0 and subnormals are entries and NaN alone says
// "no edge"; an entry of either infinity condemns the problem.  A compact stack under this rule is a view with its
// natural strides (N * M, M, 1).
//
// Outside mode Out (misslap_solve_dense_batch_outside): row i of problem b also holds one virtual entry (i, m_b + i)
// whose value is the row's outside value -- a private object that only row i can bid for, so a row may stay unmatched.
// The problem solved is the dense n_b x (m_b + n_b) matrix hstack([slice, D_b]) with D_b the outside values on its
// diagonal and no entry elsewhere; the round loop is batch_solve unchanged, on a carve of M + N objects.  The row source
// presents the virtual entry (column m_b + i, above every real column), the check pass folds the outside values into
// C = max |v| and the +inf flag, flags one that is no entry and never reports an empty row, and the solve kernel
// rewrites the outputs behind batch_solve: an object >= m_b becomes -1 in sol, price[0 .. m_b) are the real prices and
// price[m_b .. m_b + n_b) the outside prices.
#pragma once

namespace misslap {

constexpr int kDenseBatchMaxDim = MISSLAP_DENSE_BATCH_MAX_DIM;
constexpr int kDenseBatchCols = kDenseBatchMaxDim / kWave;  // columns per lane in a row scan

// per problem, from the validation pass ahead of the solve
struct DenseBatchCheck {
    unsigned long long nvalid;       // valid entries of the slice
    unsigned long long absmax_bits;  // max |v| over them, as bits (non-negative doubles order like their bit patterns)
    int empty_row;                   // first row without a valid entry (INT_MAX: none)
    int has_inf;                     // bit 0: a valid entry is +inf (outside mode: or the outside value of a row < n;
                                     // finite mode: or -inf); bit 1 (outside mode only): the outside value of a row < n
                                     // is no entry (negative or a NaN; finite mode: a NaN)
    int mref;                        // max valid column + 1 (auction_.pyx:209-212)
    int bad_price;                   // starting prices: bit 0 NaN / infinity, bit 1 sign bit set
};

struct DenseBatchArgs {
    BatchSolveArgs s;         // p0_ld = prices_ld = M, sol_ld = Ns = N, Ms = M
    const void *mat;          // elements of the kernel's T
    long long N, M;           // the extents of the stack (DenseContig: row stride M, problem stride N * M, in elements)
    const int *shapes;        // [B][2] (n_b, m_b) or null
    const DenseBatchCheck *chk;
};

// The element strides of a view (all >= 0, the host has checked that the extent fits 62 bits), and the smallest round
// that bids one lane per person (bid_lanes; INT_MAX: no round does).
struct DenseStrides {
    long long sB, sN, sM;
    int lane_min_K;
};

// A layout: where problem b, its row i and the row's column c lie, in elements, and which elements are entries.
// It is all the contiguous, strided and finite kernels differ in.
struct DenseContig {
    static constexpr bool kView = false, kUnitCol = true, kFinite = false;
    __device__ __forceinline__ size_t problem(int b, long long N, long long M) const {
        return (size_t)b * (size_t)N * (size_t)M;
    }
    __device__ __forceinline__ long long row_stride(long long M) const { return M; }
    __device__ __forceinline__ size_t col(int c) const { return (size_t)c; }
};
// Fin: the entry rule is "not a NaN".  Unit: sM == 1 is known where the code is compiled -- the solve kernels branch
// on it once per workgroup (MISSLAP_DENSE_BATCH_RUN) and the row source then steps its columns as DenseContig does.
template <bool Fin, bool Unit = false>
struct DenseView {
    static constexpr bool kView = true, kUnitCol = Unit, kFinite = Fin;
    DenseStrides str;
    __device__ __forceinline__ size_t problem(int b, long long, long long) const { return (size_t)b * (size_t)str.sB; }
    __device__ __forceinline__ long long row_stride(long long) const { return str.sN; }
    __device__ __forceinline__ size_t col(int c) const {
        if constexpr (Unit) return (size_t)c;
        else return (size_t)c * (size_t)str.sM;
    }
    __device__ __forceinline__ DenseView<Fin, true> unit() const { return {str}; }
};

__device__ __forceinline__ void dense_batch_shape(const int *shapes, long long N, long long M, int b, int &n, int &m) {
    n = shapes ? shapes[2 * b] : (int)N;
    m = shapes ? shapes[2 * b + 1] : (int)M;
}

// Validation, one workgroup per problem: valid count, empty rows, +inf, C = max |v|, the reference's M, prices.
// With shapes_out (status mode: `shapes` may be a caller's device array that no host has seen) a shape outside
// 1 .. N x 1 .. M becomes (0, 0), nothing of that problem is read, and the shape every later kernel uses is written
// to shapes_out[b]: the guard and the solve read those, never the caller's.  The all-or-nothing call, whose host has
// checked the shapes, passes null.
// Out (the outside mode): the outside value of every row < n_b counts as an entry's value does (outside[b] with
// outside_ld == 0, else outside[b * outside_ld + i]; one that is no entry raises bit 1 of has_inf instead), no row is
// empty, and with starting prices the problem's augmented starting prices [p0[:m_b], zeros(n_b)] are staged at
// aug[b * (M + N) ..] for batch_solve to load.  Otherwise outside and aug are not read.
// Under the finite rule max |v| and the infinity flag mask the sign, so -inf is caught as +inf is; an outside value is
// an entry under the layout's rule too (a NaN raises bit 1, either infinity bit 0).
template <class Lay>
struct DenseCheckArgs {
    const void *mat;        // elements of the kernel's T
    long long N, M;
    const int *shapes;      // [B][2] or null
    const double *p0;       // [B][M] or null
    DenseBatchCheck *out;   // [B]
    int *shapes_out;        // [B][2]: the sanitised shapes, or null
    const double *outside;  // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *aug;            // [B][M + N] or null (no starting prices)
    [[no_unique_address]] Lay lay;
};

template <class T, class Lay, bool Out>
__device__ __forceinline__ void dense_batch_check(const DenseCheckArgs<Lay> &a) {
    const long long N = a.N, M = a.M;
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int n, m;
    dense_batch_shape(a.shapes, N, M, b, n, m);
    if (int *shapes_out = a.shapes_out) {
        if (n < 1 || n > N || m < 1 || m > M) n = m = 0;
        if (threadIdx.x == 0) {
            shapes_out[2 * b] = n;
            shapes_out[2 * b + 1] = m;
        }
    }
    const T *A = static_cast<const T *>(a.mat) + a.lay.problem(b, N, M);
    __shared__ unsigned long long s_cnt, s_abs;
    __shared__ int s_empty, s_inf, s_mref, s_badp;
    if (threadIdx.x == 0) {
        s_cnt = 0;
        s_abs = 0;
        s_empty = 0x7fffffff;
        s_inf = 0;
        s_mref = 0;
        s_badp = 0;
    }
    __syncthreads();
    unsigned long long cnt = 0, am = 0;
    int inf = 0, mx = -1;
    for (int r = wave; r < n; r += nw) {
        const T *row = A + (size_t)r * (size_t)a.lay.row_stride(M);
        int rc = 0;
        for (int c = lane; c < m; c += kWave) {
            const T v = row[a.lay.col(c)];
            if (dense_entry_is<Lay::kFinite>(v)) {
                const unsigned long long bits =
                    (unsigned long long)__double_as_longlong(dense_widen(v)) & 0x7fffffffffffffffull;
                ++rc;
                am = bits > am ? bits : am;
                inf |= bits == 0x7ff0000000000000ull;
                mx = c > mx ? c : mx;
            }
        }
        for (int off = 32; off >= 1; off >>= 1) rc += __shfl_xor(rc, off);
        if constexpr (Out) {
            if (lane == 0) {
                const double o = a.outside[a.outside_ld ? (size_t)b * (size_t)a.outside_ld + (size_t)r : (size_t)b];
                if (dense_entry_is<Lay::kFinite>(o)) {
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(o) & 0x7fffffffffffffffull;
                    am = bits > am ? bits : am;
                    inf |= bits == 0x7ff0000000000000ull;
                } else {
                    inf |= 2;
                }
            }
        } else {
            if (rc == 0 && lane == 0) atomicMin(&s_empty, r);
        }
        cnt += (unsigned long long)rc;  // (uniform; lane 0's copy is added below)
    }
    if (lane == 0) atomicAdd(&s_cnt, cnt);
    if (am) atomicMax(&s_abs, am);
    if (inf) atomicOr(&s_inf, Out ? inf : 1);
    if (mx >= 0) atomicMax(&s_mref, mx + 1);
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
        DenseBatchCheck r;
        r.nvalid = s_cnt;
        r.absmax_bits = s_abs;
        r.empty_row = s_empty;
        r.has_inf = s_inf;
        r.mref = s_mref;
        r.bad_price = s_badp;
        a.out[b] = r;
    }
}

// (the body stays a function of its own: written into the kernel, the double instances of DenseView<true> take another
// register allocation)
template <class T, class Lay, bool Out>
__global__ __launch_bounds__(256) void k_dense_batch_check(DenseCheckArgs<Lay> a) {
    dense_batch_check<T, Lay, Out>(a);
}

// The dense row source of batch_solve: problem b's slice A of n x m, its reference M and valid count.  Entry (i, c)
// lies at A[i * M + lay.col(c)], M being the layout's row stride (MISSLAP_DENSE_BATCH_RUN fills both in).
// The bid's staging array `vals` belongs to the solve kernel: declared in bid() it is promoted to a vector while bid()
// is optimised on its own, and every staging step then zeroes the rest of it (measured: 3.8 % more kernel time at
// 64 x 1000).  Declared in the kernel, it becomes 16 register pairs as in a hand-inlined scan.  The row is staged in its
// own type T -- 16 registers for float and for the 16-bit types, one element per lane per load with the same
// column-to-lane map -- and widened where the scan uses it.
// Out: row i's virtual last entry (i, m + i) with the row's outside value; mref and nvalid then count the augmented
// problem (m + n columns, n more entries).  Column m + i is above every real column, and lane (m + i) & 63 takes it AFTER
// its own real columns, so every lane still scans in ascending column order and the winner's lane is r.g & 63 as before.
// A chosen object j >= m is that entry: nothing of the slice is read for it.
// The wavefront scan keeps its lane map (lane l holds columns l, l + 64, ...) whatever the strides are, with loads of
// one element each: nothing wider than the element is assumed of the base or of a stride.
// Under the finite rule a staging slot beyond the row still holds dense_hole, which is then an entry, and is still
// never tested: every scan asks c < m first.
template <class T, class Lay, bool Out>
struct DenseBatchRows {
    const T *A;
    long long M;
    int m, maximize, mref;
    unsigned long long nvalid;
    T *vals;  // [kDenseBatchCols]
    BatchOutside<Out> out;
    [[no_unique_address]] Lay lay;

    // one candidate of a scan: value v of object c, against the best two so far
    __device__ __forceinline__ void take(Top2 &x, double &cb, double v, int c, const double *price) const {
        const double cost = maximize ? v : v * -1.0;  // :236-237
        const double vi = cost - price[c];
        if (top2_take(x, vi, c)) cb = cost;
    }

    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        const T *row = A + (size_t)i * (size_t)M;
        Top2 x;
        double cb;
        if constexpr (Lay::kUnitCol) {
#pragma unroll
            for (int q = 0; q < kDenseBatchCols; ++q) {
                if (q * kWave >= m) break;
                const int c = lane + q * kWave;
                vals[q] = c < m ? row[c] : dense_hole<T>();
            }
            x.v = -__builtin_huge_val();
            x.w = -__builtin_huge_val();
            x.g = -1;
            cb = 0.0;
#pragma unroll
            for (int q = 0; q < kDenseBatchCols; ++q) {
                if (q * kWave >= m) break;
                const int c = lane + q * kWave;
                if (c < m && dense_entry_is<Lay::kFinite>(vals[q])) take(x, cb, dense_widen(vals[q]), c, price);
            }
        } else {
            // a column stride other than 1 (a view's sM == 1 takes the scan above): one pointer stepped from load to
            // load, staged and scanned in two halves of 8 slots, in ascending order -- 16 addresses next to 16 staged
            // doubles do not fit the 128 registers of a 1024-thread workgroup
            x.v = -__builtin_huge_val();
            x.w = -__builtin_huge_val();
            x.g = -1;
            cb = 0.0;
            const T *p = row + (size_t)lane * (size_t)lay.str.sM;
            const size_t step = (size_t)kWave * (size_t)lay.str.sM;
            constexpr int kHalf = kDenseBatchCols / 2;
            for (int h = 0; h < kDenseBatchCols && h * kWave < m; h += kHalf) {
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    vals[q] = lane + (h + q) * kWave < m ? *p : dense_hole<T>();
                    p += step;
                }
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    const int c = lane + (h + q) * kWave;
                    if (c < m && dense_entry_is<Lay::kFinite>(vals[q])) take(x, cb, dense_widen(vals[q]), c, price);
                }
            }
        }
        if constexpr (Out) {
            if (lane == ((m + i) & (kWave - 1))) take(x, cb, out.value(i), m + i, price);
        }
        const Top2 r = top2_wave_reduce(x);
        costbest = readlane_f64(cb, r.g & (kWave - 1));  // the lane that holds column r.g
        obj = r.g;
        return r;
    }

    // The second bid mapping of a view's row source, for a whole round: one LANE per list position, 64 persons per
    // wavefront.  On a stack whose rows run along the unit stride (M == sN == 1: a transposed view) a wavefront that
    // scans one person's row touches 64 cache lines per load; here lane l scans the row of person U[k0 + l] in column
    // order, so one load instruction reads column c of 64 persons, and in the first round of every eps-phase
    // (U = 0 .. n - 1) those are 64 adjacent elements.  price[c] is one LDS address for the whole wavefront (a
    // broadcast).  The scan is the reference's sequential one (:339-365) with its ">=" rule, so (v, w, g) and the
    // winner's cost are those of bid(); eight loads are in flight per lane.  Returns false, having done nothing, for
    // a round the wavefront scan serves better: fewer than lane_min_K bidders (one lane would run m dependent steps
    // for one bidder) or another layout.  The branch is uniform.
    __device__ __forceinline__ bool bid_lanes(const int *U, int K, const double *price, float eps,
                                              unsigned long long *bid_key, int *bid_obj, unsigned long long *bkey) const {
        static_assert(Lay::kView && !Lay::kUnitCol, "only a view's row source has the lane-per-person bid");
        if (K < lay.str.lane_min_K || M != 1) return false;
        constexpr int kFly = 8;
        for (int k = threadIdx.x; k < K; k += blockDim.x) {
            const int i = U[k];
            const T *row = A + (size_t)i * (size_t)M;
            Top2 x;
            x.v = -__builtin_huge_val();
            x.w = -__builtin_huge_val();
            x.g = -1;
            double cb = 0.0;
            for (int c0 = 0; c0 < m; c0 += kFly) {
                T v8[kFly];
#pragma unroll
                for (int q = 0; q < kFly; ++q) v8[q] = c0 + q < m ? row[lay.col(c0 + q)] : dense_hole<T>();
#pragma unroll
                for (int q = 0; q < kFly; ++q) {
                    const int c = c0 + q;
                    if (c < m && dense_entry_is<Lay::kFinite>(v8[q])) take(x, cb, dense_widen(v8[q]), c, price);
                }
            }
            if constexpr (Out) take(x, cb, out.value(i), m + i, price);
            const unsigned long long key = bid_to_key(cb - x.w + (double)eps);  // :360
            bid_key[k] = key;
            bid_obj[k] = x.g;
            atomicMax(&bkey[x.g], key);
        }
        return true;
    }

    // eCE_satisfied (auction_.pyx:443-485) for row i: choice_cost is the cost of column j, every valid column is tested
    __device__ __forceinline__ bool ece_bad(int i, int j, const double *price, double tol, double eps) const {
        const T *row = A + (size_t)i * (size_t)M;
        double vj;
        if constexpr (Out) vj = j >= m ? out.value(i) : dense_widen(row[lay.col(j)]);
        else vj = dense_widen(row[lay.col(j)]);
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
            const T e = row[lay.col(c)];
            if (!dense_entry_is<Lay::kFinite>(e)) continue;
            const double v = dense_widen(e);
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - price[c]) - eps) bad = true;  // :482
        }
        return bad;
    }

    // get_obj (:489-523): one thread per row gathers its chosen value
    __device__ __forceinline__ void gather(const int *p2o, int n, double *selv, int *) const {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int j = p2o[i];
            if constexpr (Out) {
                if (j >= m) {  // the row's outside entry
                    selv[i] = out.value(i);
                    continue;
                }
            }
            selv[i] = j >= 0 ? dense_widen(A[(size_t)i * (size_t)M + lay.col(j)]) : 0.0;
        }
    }

    // a double sum in row order
    __device__ __forceinline__ double objective(const int *p2o, int n, const double *selv, const int *) const {
        double obj = 0;
        for (int i = 0; i < n; ++i) {
            if (p2o[i] == -1) continue;
            const double val = maximize ? selv[i] : selv[i] * -1.0;
            if (maximize) obj += val;
            else obj -= val;
        }
        return obj;
    }

    __device__ __forceinline__ int meta_cols(int) const { return mref; }
    __device__ __forceinline__ int64_t meta_nnz() const { return (int64_t)nvalid; }
};

template <class T, bool Fin, bool Out>
struct RowsBidLanes<DenseBatchRows<T, DenseView<Fin>, Out>> {
    static constexpr bool value = true;
};

// batch_solve on the accepted problem b (n x m) of a kernel's stack, written once: the one place that forms the
// problem's base pointer and row stride from the layout `lay`, builds the row source and holds a view's branch.
// d: the kernel's DenseBatchArgs, s: its BatchSolveArgs, vals: its staging array, out: a BatchOutside<Out> (the
// outside mode counts the augmented problem: m + n columns, n more entries).  A view with a unit column stride takes
// the scan of the contiguous row source with sN for its row stride (the same bid, instruction for instruction); any
// other takes the two-half scan.  That branch is uniform, and a view's kernel holds both solves.
// A macro, because the sequence has to be compiled as part of the kernel that declares `vals`.  A callee is optimised
// on its own before it is inlined: one that builds the row source around a `vals` it only has a pointer to forwards
// the staged values past the array (all 34 solve instances then move, by 2 VGPRs at double); one that declares `vals`
// itself leaves the contiguous instances alone but the view instances allocate their scalar registers anew; and even a
// function that only returns the row source moves the contiguous instances by a register.
#define MISSLAP_DENSE_BATCH_RUN(T, Lay, Out, d, lay, s, b, n, m, ck, vals, out)                                           \
    do {                                                                                                                  \
        const T *A = static_cast<const T *>(d.mat) + lay.problem(b, d.N, d.M);                                            \
        const unsigned long long nv = Out ? ck.nvalid + (unsigned long long)n : ck.nvalid;                                \
        if constexpr (Lay::kView) {                                                                                       \
            if (lay.str.sM == 1) {                                                                                        \
                const DenseBatchRows<T, DenseView<Lay::kFinite, true>, Out> rows{                                         \
                    A, lay.row_stride(d.M), m, s.maximize, Out ? m + n : ck.mref, nv, vals, out, lay.unit()};             \
                batch_solve(s, rows, n, Out ? m + n : m, ck.absmax_bits);                                                 \
            } else {                                                                                                      \
                const DenseBatchRows<T, Lay, Out> rows{                                                                   \
                    A, lay.row_stride(d.M), m, s.maximize, Out ? m + n : ck.mref, nv, vals, out, lay};                    \
                batch_solve(s, rows, n, Out ? m + n : m, ck.absmax_bits);                                                 \
            }                                                                                                             \
        } else {                                                                                                          \
            const DenseBatchRows<T, Lay, Out> rows{                                                                       \
                A, lay.row_stride(d.M), m, s.maximize, Out ? m + n : ck.mref, nv, vals, out, lay};                        \
            batch_solve(s, rows, n, Out ? m + n : m, ck.absmax_bits);                                                     \
        }                                                                                                                 \
    } while (0)

template <class T, class Lay = DenseContig>
__global__ __launch_bounds__(1024) void k_dense_batch_solve(DenseBatchArgs a) {
    const int b = blockIdx.x;
    int n, m;
    dense_batch_shape(a.shapes, a.N, a.M, b, n, m);
    const DenseBatchCheck ck = a.chk[b];
    T vals[kDenseBatchCols];
    const Lay lay{};
    MISSLAP_DENSE_BATCH_RUN(T, Lay, false, a, lay, a.s, b, n, m, ck, vals, BatchOutside<false>{});
}

// ---- status mode (misslap_solve_dense_batch_status): a verdict per problem instead of all or nothing

// what the two solves with a verdict share
struct DenseVerdictArgs {
    DenseBatchArgs d;      // d.shapes: the check pass's sanitised shapes (never null); d.mat: the stack's first element
    const int *card;       // [B] the guard's cardinalities, or null: no guard in this call
    int fast;              // eps_start = 1 / n_b of each problem (auction_.pyx:568-569)
    int *status;           // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;    // [B] or null: the guard's cardinality, -1 where it did not run
};

template <class Lay>
struct DenseStatusArgs {
    DenseVerdictArgs t;
    [[no_unique_address]] Lay lay;
};

// The dense checks of a verdict, in first_error's order (abi_dense_batch.hpp); batch_verdict adds the shared rest.
__device__ __forceinline__ int dense_batch_verdict(const DenseBatchCheck &c, int n) {
    if (n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (c.nvalid < (unsigned long long)n) return MISSLAP_BATCH_STATUS_TOO_FEW_VALUES;
    if (c.empty_row != 0x7fffffff) return MISSLAP_BATCH_STATUS_EMPTY_ROW;
    if (c.has_inf) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    return MISSLAP_BATCH_STATUS_OK;
}

// k_dense_batch_solve with the verdict formed here, from what the check pass and the guard left on the device.  A
// condemned problem's workgroup writes the defined outputs and leaves before any LDS state exists; the others run the
// same batch_solve on the same row source.
template <class T, class Lay>
__global__ __launch_bounds__(1024) void k_dense_batch_solve_status(DenseStatusArgs<Lay> a) {
    const int b = blockIdx.x;
    const DenseBatchArgs &d = a.t.d;
    const int n = d.shapes[2 * b], m = d.shapes[2 * b + 1];
    const DenseBatchCheck ck = d.chk[b];
    const int card = a.t.card && n >= 1 ? a.t.card[b] : -1;
    const int code = batch_verdict(dense_batch_verdict(ck, n), a.t.card != nullptr, card, n, ck.bad_price);
    batch_publish_verdict(a.t.status, a.t.matching_size, b, code, card);
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(d.s, n, ck.mref, (long long)ck.nvalid);
        return;
    }
    BatchSolveArgs s = d.s;
    if (a.t.fast) batch_fast_eps(s, n);
    T vals[kDenseBatchCols];
    MISSLAP_DENSE_BATCH_RUN(T, Lay, false, d, a.lay, s, b, n, m, ck, vals, BatchOutside<false>{});
}

// ---- outside mode (misslap_solve_dense_batch_outside): an outside option per row, for partial assignments

template <class Lay>
struct DenseOutsideArgs {
    DenseVerdictArgs t;      // t.d.s: Ms = M + N (the carve), p0 / p0_ld the staged augmented prices, prices null;
                             // t.card null: no guard in this call
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *prices;          // [B][M] or null: the real columns
    double *outside_prices;  // [B][N] or null
    [[no_unique_address]] Lay lay;
};

// The checks of an outside verdict in their order; EMPTY_ROW, TOO_FEW_VALUES and INFEASIBLE cannot occur.
__device__ __forceinline__ int dense_outside_verdict(const DenseBatchCheck &c, int n) {
    if (n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (c.has_inf & 2) return MISSLAP_BATCH_STATUS_BAD_OUTSIDE;
    if (c.has_inf & 1) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve of the outside mode: the verdict, batch_solve on the n x (m + n) problem, then the outputs in the caller's
// terms (batch_outside_outputs).
template <class T, class Lay>
__global__ __launch_bounds__(1024) void k_dense_outside_solve(DenseOutsideArgs<Lay> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const DenseBatchArgs &d = a.t.d;
    const int n = d.shapes[2 * b], m = d.shapes[2 * b + 1];
    const DenseBatchCheck ck = d.chk[b];
    const int code = batch_verdict(dense_outside_verdict(ck, n), false, -1, n, ck.bad_price);
    batch_publish_verdict(a.t.status, a.t.matching_size, b, code, -1);
    const int N = (int)d.N, M = (int)d.M;
    double *po = a.prices ? a.prices + (size_t)b * (size_t)M : nullptr;
    double *oo = a.outside_prices ? a.outside_prices + (size_t)b * (size_t)N : nullptr;
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(d.s, n, m + n, (long long)ck.nvalid + n);
        batch_outside_condemn(po, M, oo, N, tid, nt);
        return;
    }
    BatchSolveArgs s = d.s;
    if (a.t.fast) batch_fast_eps(s, n);
    T vals[kDenseBatchCols];
    const double *O = a.outside + (a.outside_ld ? (size_t)b * (size_t)a.outside_ld : (size_t)b);
    MISSLAP_DENSE_BATCH_RUN(T, Lay, true, d, a.lay, s, b, n, m, ck, vals, (BatchOutside<true>{O, a.outside_ld ? 1 : 0}));
    batch_outside_outputs(s_raw, d.s, b, n, m, M, N, po, oo, tid, nt);
}

// ---- reverse finish (misslap_dense_batch_reverse_finish): the reverse-auction clean-up behind a forward solve
//
// A forward auction on a rectangular problem (n rows, more than n objects) that did not start from zero prices ends
// with eps-CS and, in general, far from the optimum: objects that were bid up and then abandoned keep prices above
// those of the objects in use.  The modified reverse auction with a fixed lambda (Bertsekas, Network Optimization, 7.2)
// repairs exactly that: lambda = the smallest price of an assigned object, and every unassigned object priced above it
// either takes the row that values it most (at a price that keeps eps-CS) or drops to lambda.  Afterwards eps-CS still
// holds at the solve's final eps and no unassigned object is priced above lambda: optimal within n * eps.
// Every move raises the moving row's profit by at least eps, which ends the loop; where eps is lost to rounding
// (outside max(|a|, |p|) * 2^-52 < eps) a move can leave it unchanged, so an iteration whose move would not raise it
// ends the finish with left > 0 (the stall rule of sslap_amd.dense_reverse_finish).
//
// One workgroup per problem, its own launch behind the solve's, reading the solve's outputs: status first (a problem
// whose status is not 0 is not touched, so a caller's bad device shape is never read), then meta.n_assigned (a solve
// cut by max_iter is not touched either).  State in LDS, carved for the stack's N rows and Mo = M (+ N outside) objects:
// p[Mo], pi[N] (the rows' profits a_ij - p_j), o2p[Mo], p2o[N]: 12 Mo + 12 N bytes, 36 864 at 1024 x 1024 with outside.
//
// The loop is serial by definition (sslap_amd.dense_reverse_finish is its statement in numpy; the two agree operation
// for operation in float64) and each iteration is a chain of dependent latencies: pick j, read column j of the n rows
// (strided global loads), reduce the rows' top two of a_ij - pi_i, update a few scalars.  It runs on wavefront 0 ALONE:
// lane l holds rows l, l + 64, ... (up to 16 loads in flight, issued back to back under one latency), the top two are
// reduced with lane shuffles so that every lane ends with the same (beta, row, omega) and takes the same branch, and
// lane 0 stores the few changed cells.  Nothing in the iteration crosses a wavefront, so there is no LDS exchange and no
// workgroup barrier in it: LDS operations of one wavefront complete in order, and a wavefront-scope fence keeps the
// compiler from moving them.  The other three wavefronts wait at the one barrier behind the loop; they load the state
// before it and share the eCE test (n rows x m columns) and the outputs after it.
constexpr int kDenseFinishThreads = 256;
constexpr int kDenseFinishRows = kDenseBatchMaxDim / kWave;  // rows per lane in a column scan

template <class Lay>
struct DenseFinishArgs {
    const void *mat;         // elements of the kernel's T
    long long N, M;          // the extents of the stack
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
    [[no_unique_address]] Lay lay;
};

__host__ __device__ constexpr size_t dense_finish_lds_bytes(long long N, long long Mo) {
    return (size_t)Mo * (8 + 4) + (size_t)N * (8 + 4);
}

// LDS stores of this wavefront before, its LDS loads behind: in order (one wavefront's LDS operations complete in the
// order they were issued; the fences bind the compiler)
__device__ __forceinline__ void dense_finish_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class T, class Lay, bool Out>
__global__ __launch_bounds__(kDenseFinishThreads) void k_dense_reverse_finish(DenseFinishArgs<Lay> a) {
    static_assert(Lay::kView, "the finish reads every stack as a view (a compact one has its natural strides)");
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ double s_min[kDenseFinishThreads / kWave];
    __shared__ int s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = nt >> 6;
    const int N = (int)a.N, M = (int)a.M;
    int n, m;
    dense_batch_shape(a.shapes, a.N, a.M, b, n, m);
    const bool run = a.status[b] == MISSLAP_BATCH_STATUS_OK && n >= 1 && n <= N && m >= 1 && m <= M &&
                     a.meta[b].n_assigned == (int64_t)n;
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
    const T *A = static_cast<const T *>(a.mat) + a.lay.problem(b, a.N, a.M);
    const size_t sN = (size_t)a.lay.row_stride(a.M);
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
    // the maximised value of entry (i, j) of the augmented problem (an entry: the caller knows)
    auto value = [&](int i, int j) -> double {
        double v;
        if (Out && j >= m) v = O[i * ostride];
        else v = dense_widen(A[(size_t)i * sN + a.lay.col(j)]);
        return maximize ? v : v * -1.0;
    };

    // ---- set-up: p, o2p, p2o, pi and lambda
    if (tid == 0) s_bad = 0;
    for (int j = tid; j < mo; j += nt) {
        p[j] = j < m ? po[j] : oo[j - m];
        o2p[j] = -1;
    }
    __syncthreads();
    double lmin = __builtin_huge_val();
    for (int i = tid; i < n; i += nt) {
        int j = sol[i];
        if (Out && j == -1) j = m + i;
        if (j < 0 || j >= m + (Out ? n : 0) || (j >= m && j != m + i)) {  // (not a solve's output: leave it alone)
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
                const T *col = A + a.lay.col(j);
                T v[kDenseFinishRows];
#pragma unroll
                for (int q = 0; q < kDenseFinishRows; ++q) {
                    if (q * kWave >= n) break;
                    const int i = lane + q * kWave;
                    v[q] = i < n ? col[(size_t)i * sN] : dense_hole<T>();
                }
#pragma unroll
                for (int q = 0; q < kDenseFinishRows; ++q) {
                    if (q * kWave >= n) break;
                    const int i = lane + q * kWave;
                    if (i < n && dense_entry_is<Lay::kFinite>(v[q])) {
                        const double e = dense_widen(v[q]);
                        const double av = maximize ? e : e * -1.0;
                        const double w = av - pi[i];
                        if (w > bw) {
                            ow = bw;
                            bw = w;
                            bi = i;
                            ba = av;
                        } else if (w > ow) {
                            ow = w;
                        }
                    }
                }
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

    // ---- the outputs in the caller's terms, the chosen values (into pi, which the loop is done with), eCE at target eps
    for (int i = tid; i < n; i += nt) sol[i] = p2o[i] < m ? p2o[i] : -1;
    for (int j = tid; j < m; j += nt) po[j] = p[j];
    if constexpr (Out)
        for (int i = tid; i < n; i += nt) oo[i] = p[m + i];
    double *selv = pi;
    const double tol = 1e-7, teps = (double)(float)(1.0 / (double)n);
    for (int i = wave; i < n; i += nw) {  // eCE_satisfied (auction_.pyx:443-485), as batch_ece makes it
        const int j = p2o[i];
        double vj;
        if (Out && j >= m) vj = O[i * ostride];
        else vj = dense_widen(A[(size_t)i * sN + a.lay.col(j)]);
        const double choice_cost = maximize ? vj : vj * -1.0;
        const double LHS = choice_cost - p[j] + tol;
        bool bad = false;
        if constexpr (Out) {
            if (lane == 0 && LHS < (value(i, m + i) - p[m + i]) - teps) bad = true;
        }
        const T *row = A + (size_t)i * sN;
        for (int c = lane; c < m; c += kWave) {
            const T e = row[a.lay.col(c)];
            if (!dense_entry_is<Lay::kFinite>(e)) continue;
            const double v = dense_widen(e);
            const double cost = maximize ? v : v * -1.0;
            if (LHS < (cost - p[c]) - teps) bad = true;
        }
        if (__ballot(bad) && lane == 0) s_bad = 1;
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) selv[i] = vj;
    }
    __syncthreads();
    if (tid == 0) {  // get_obj (:489-523) in row order
        double obj = 0;
        for (int i = 0; i < n; ++i) {
            const double val = maximize ? selv[i] : selv[i] * -1.0;
            if (maximize) obj += val;
            else obj -= val;
        }
        misslap_dense_batch_meta &r = a.meta[b];
        r.obj_f64 = obj;
        r.obj_f32 = (float)obj;
        r.eCE = s_bad ? 0 : 1;
    }
}

}  // namespace misslap
