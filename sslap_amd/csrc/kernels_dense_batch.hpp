// kernels_dense_batch.hpp -- many small dense problems, one workgroup per problem for its whole solve
// (misslap_solve_dense_batch, include/misslap.h; the host side is abi_dense_batch.hpp).
//
// The round loop is batch_solve (kernels_batch_solve.hpp); this file has the check pass and the dense row source.
// Values are read from the caller's dense rows (row stride = the stack's M) in global memory, where a small problem
// stays in L2.  The rows have the caller's element type T (double, float, F16, Bf16: misslap_options.mat_dtype); the
// three kernels that read them are templates on T, every value is widened to double where it is used (dense_widen,
// exact), and batch_solve only ever sees doubles:
//   BID      lanes scan the row in column order (lane l holds columns l, l + 64, ...), staged in registers with up to
//            kDenseBatchCols loads in flight; the object is the winning column r.g.
//   eCE      every column is stored once, so choice_cost -- never reset per row in the reference -- is the cost of the
//            row's own column.
//   get_obj  the selected values are gathered into LDS, then one lane adds them in row order.
//
// The outside mode (misslap_solve_dense_batch_outside; the <T, true> instances below): row i of problem b also holds one
// virtual entry (i, m_b + i) whose value is the row's outside value -- a private object that only row i can bid for, so
// a row may stay unmatched.  The problem solved is the dense n_b x (m_b + n_b) matrix hstack([slice, D_b]) with D_b the
// outside values on its diagonal and -1 elsewhere; the round loop is batch_solve unchanged, on a carve of M + N objects.
// The row source presents the virtual entry (column m_b + i, above every real column), the check pass folds the outside
// values into C = max |v| and the +inf flag, flags a negative or NaN one and never reports an empty row, and the solve
// kernel rewrites the outputs behind batch_solve: an object >= m_b becomes -1 in sol, price[0 .. m_b) are the real
// prices and price[m_b .. m_b + n_b) the outside prices.
//
// The strided family (misslap_solve_dense_batch_status_strided / _outside_strided; the instances on DenseStrided*Args
// and k_dense_strided_check): the same check pass, row source and solve kernels on a stack whose element (b, i, j) lies
// at mat[b * sB + i * sN + j * sM] for run-time strides >= 0 -- a transposed view, a slice of a wider buffer, an
// expanded matrix (sB = 0).  Every entry plays the role it plays in the contiguous stack, so the results are those of
// the compact copy bit for bit; offsets are formed in 64 bits and only elements of the view are read.  The contiguous
// instances take no stride: theirs are compile-time (DenseColStride<false> is empty), and their code is what it was.
// A strided row source also has a second bid mapping, bid_lanes below, for rounds of many bidders on a stack whose
// rows run along the unit stride (sN == 1).
//
// Finite mode (MISSLAP_DENSE_ENTRIES_FINITE in misslap_options.mat_dtype; the instances on DenseFinite*Args and
// k_dense_finite_check): signed cost stacks.  An element is an entry iff it is not a NaN in its own type, so negative
// values, -0.0 and subnormals are entries and NaN alone says "no edge"; an entry of either infinity condemns the
// problem.  One compile-time flag (Fin) on everything that asks "is this an entry", default off; it is instantiated in
// the strided family only, and a contiguous stack in this mode runs these kernels with its natural strides.
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
    long long N, M;           // the stack: row stride M, problem stride N * M, in elements
    const int *shapes;        // [B][2] (n_b, m_b) or null
    const DenseBatchCheck *chk;
};

// The element strides of a strided stack (all >= 0, the host has checked that the extent fits 62 bits), and the
// smallest round that bids one lane per person (bid_lanes; INT_MAX: no round does).
struct DenseStrides {
    long long sB, sN, sM;
    int lane_min_K;
};

// The column step of a row source: 1 at compile time in a contiguous stack, the stack's sM in a strided one.
template <bool Str>
struct DenseColStride {
    __device__ __forceinline__ size_t at(int c) const { return (size_t)c; }
};
template <>
struct DenseColStride<true> {
    long long sM;
    int lane_min_K;
    __device__ __forceinline__ size_t at(int c) const { return (size_t)c * (size_t)sM; }
};

__device__ __forceinline__ void dense_batch_shape(const int *shapes, long long N, long long M, int b, int &n, int &m) {
    n = shapes ? shapes[2 * b] : (int)N;
    m = shapes ? shapes[2 * b + 1] : (int)M;
}

// Validation, one workgroup per problem: valid count, empty rows, +inf, C = max |v|, the reference's M, prices.
// With shapes_out (status mode: `shapes` may be a caller's device array that no host has seen) a shape outside
// 1 .. N x 1 .. M becomes (0, 0), nothing of that problem is read, and the shape every later kernel uses is written
// to shapes_out[b]: the guard and the solve read those, never the caller's.
// Out (the outside mode): the outside value of every row < n_b counts as an entry's value does (ov: outside[b] with
// ov_ld == 0, else outside[b * ov_ld + i]; a negative one or a NaN raises bit 1 of has_inf instead), no row is empty,
// and with starting prices the problem's augmented starting prices [p0[:m_b], zeros(n_b)] are staged at
// aug[b * (M + N) ..] for batch_solve to load.
// Str (the strided family): element (b, r, c) lies at mat[b * str.sB + r * str.sN + c * str.sM]; else str is not read.
// Fin (finite mode, below): an element is an entry iff it is not a NaN; max |v| and the infinity flag mask the sign, so
// -inf is caught as +inf is; an outside value is an entry under the same rule (a NaN raises bit 1, either infinity bit 0).
template <class T, bool Out, bool Str = false, bool Fin = false>
__device__ __forceinline__ void dense_batch_check(const T *mat, long long N, long long M, const int *shapes,
                                                  const double *p0, DenseBatchCheck *out, int *shapes_out,
                                                  const double *ov, long long ov_ld, double *aug,
                                                  const DenseStrides &str = {}) {
    const int b = blockIdx.x, lane = lane_id(), wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int n, m;
    dense_batch_shape(shapes, N, M, b, n, m);
    if (shapes_out) {
        if (n < 1 || n > N || m < 1 || m > M) n = m = 0;
        if (threadIdx.x == 0) {
            shapes_out[2 * b] = n;
            shapes_out[2 * b + 1] = m;
        }
    }
    const T *A = mat + (Str ? (size_t)b * (size_t)str.sB : (size_t)b * (size_t)N * (size_t)M);
    DenseColStride<Str> col{};
    if constexpr (Str) col.sM = str.sM;
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
        const T *row = A + (size_t)r * (size_t)(Str ? str.sN : M);
        int rc = 0;
        for (int c = lane; c < m; c += kWave) {
            const T v = row[col.at(c)];
            if (dense_entry_is<Fin>(v)) {
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
                const double o = ov[ov_ld ? (size_t)b * (size_t)ov_ld + (size_t)r : (size_t)b];
                if (dense_entry_is<Fin>(o)) {
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
    if (p0) batch_check_prices(p0 + (size_t)b * (size_t)M, m, &s_badp);
    if constexpr (Out) {
        if (p0) {
            const double *src = p0 + (size_t)b * (size_t)M;
            double *dst = aug + (size_t)b * (size_t)(M + N);
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
        out[b] = r;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_dense_batch_check(const T *mat, long long N, long long M, const int *shapes,
                                                           const double *p0, DenseBatchCheck *out, int *shapes_out) {
    dense_batch_check<T, false>(mat, N, M, shapes, p0, out, shapes_out, nullptr, 0, nullptr);
}

struct DenseOutsideCheckArgs {
    const void *mat;        // elements of the kernel's T
    long long N, M;
    const int *shapes;      // [B][2] or null
    const double *p0;       // [B][M] or null
    DenseBatchCheck *out;   // [B]
    int *shapes_out;        // [B][2]: the sanitised shapes (never null)
    const double *outside;  // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *aug;            // [B][M + N] or null (no starting prices)
};

template <class T>
__global__ __launch_bounds__(256) void k_dense_outside_check(DenseOutsideCheckArgs a) {
    dense_batch_check<T, true>(static_cast<const T *>(a.mat), a.N, a.M, a.shapes, a.p0, a.out, a.shapes_out, a.outside,
                               a.outside_ld, a.aug);
}

// the check pass of the strided family, in either mode (Out false: a.outside and a.aug are not read)
template <class T, bool Out>
__global__ __launch_bounds__(256) void k_dense_strided_check(DenseOutsideCheckArgs a, DenseStrides str) {
    dense_batch_check<T, Out, true>(static_cast<const T *>(a.mat), a.N, a.M, a.shapes, a.p0, a.out, a.shapes_out,
                                    a.outside, a.outside_ld, a.aug, str);
}

// ... and of a finite-mode call (a kernel of its own name: k_dense_strided_check's instances are what they were)
template <class T, bool Out>
__global__ __launch_bounds__(256) void k_dense_finite_check(DenseOutsideCheckArgs a, DenseStrides str) {
    dense_batch_check<T, Out, true, true>(static_cast<const T *>(a.mat), a.N, a.M, a.shapes, a.p0, a.out, a.shapes_out,
                                          a.outside, a.outside_ld, a.aug, str);
}

// The dense row source of batch_solve: problem b's slice A (row stride M) of n x m, its reference M and valid count.
// The bid's staging array `vals` belongs to k_dense_batch_solve: declared in bid() it is promoted to a vector while bid()
// is optimised on its own, and every staging step then zeroes the rest of it (measured: 3.8 % more kernel time at
// 64 x 1000).  Declared in the kernel, it becomes 16 register pairs as in a hand-inlined scan.  The row is staged in its
// own type T -- 16 registers for float and for the 16-bit types, one element per lane per load with the same
// column-to-lane map -- and widened where the scan uses it.
// Out: row i's virtual last entry (i, m + i) with the row's outside value; mref and nvalid then count the augmented
// problem (m + n columns, n more entries).  Column m + i is above every real column, and lane (m + i) & 63 takes it AFTER
// its own real columns, so every lane still scans in ascending column order and the winner's lane is r.g & 63 as before.
// A chosen object j >= m is that entry: nothing of the slice is read for it.
// Str (the strided family): M is the row stride sN and col holds the column stride sM; entry (i, c) lies at
// A[i * M + c * sM].  The wavefront scan keeps its lane map (lane l holds columns l, l + 64, ...) whatever the strides
// are, with loads of one element each: nothing wider than the element is assumed of the base or of a stride.
// Fin (finite mode): the entry test of the three bid mappings and of the eCE walk is "not a NaN" (dense_entry_is); a
// staging slot beyond the row still holds dense_hole, which is an entry under this rule, and is still never tested:
// every scan asks c < m first.  Resolved at compile time: the <.., false> instances are the code they were.
template <class T, bool Out = false, bool Str = false, bool Fin = false>
struct DenseBatchRows {
    const T *A;
    long long M;
    int m, maximize, mref;
    unsigned long long nvalid;
    T *vals;  // [kDenseBatchCols]
    BatchOutside<Out> out{};
    DenseColStride<Str> col{};

    __device__ __forceinline__ Top2 bid(int i, const double *price, double &costbest, int &obj) const {
        const int lane = lane_id();
        const T *row = A + (size_t)i * (size_t)M;
        Top2 x;
        double cb;
        if constexpr (!Str) {
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
                if (c < m && dense_entry_is<Fin>(vals[q])) {
                    const double v = dense_widen(vals[q]);
                    const double cost = maximize ? v : v * -1.0;  // :236-237
                    const double vi = cost - price[c];
                    if (top2_take(x, vi, c)) cb = cost;
                }
            }
        } else {
            // a column stride other than 1 (a strided kernel gives sM == 1 to the contiguous row source): one pointer
            // stepped from load to load, staged and scanned in two halves of 8 slots, in ascending order -- 16
            // addresses next to 16 staged doubles do not fit the 128 registers of a 1024-thread workgroup
            x.v = -__builtin_huge_val();
            x.w = -__builtin_huge_val();
            x.g = -1;
            cb = 0.0;
            const T *p = row + (size_t)lane * (size_t)col.sM;
            const size_t step = (size_t)kWave * (size_t)col.sM;
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
                    if (c < m && dense_entry_is<Fin>(vals[q])) {
                        const double v = dense_widen(vals[q]);
                        const double cost = maximize ? v : v * -1.0;
                        const double vi = cost - price[c];
                        if (top2_take(x, vi, c)) cb = cost;
                    }
                }
            }
        }
        if constexpr (Out) {
            if (lane == ((m + i) & (kWave - 1))) {
                const double v = out.value(i);
                const double cost = maximize ? v : v * -1.0;
                const double vi = cost - price[m + i];
                if (top2_take(x, vi, m + i)) cb = cost;
            }
        }
        const Top2 r = top2_wave_reduce(x);
        costbest = readlane_f64(cb, r.g & (kWave - 1));  // the lane that holds column r.g
        obj = r.g;
        return r;
    }

    // The second bid mapping of a strided row source, for a whole round: one LANE per list position, 64 persons per
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
        static_assert(Str, "only a strided row source has the lane-per-person bid");
        if (K < col.lane_min_K || M != 1) return false;
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
                for (int q = 0; q < kFly; ++q) v8[q] = c0 + q < m ? row[col.at(c0 + q)] : dense_hole<T>();
#pragma unroll
                for (int q = 0; q < kFly; ++q) {
                    const int c = c0 + q;
                    if (c < m && dense_entry_is<Fin>(v8[q])) {
                        const double v = dense_widen(v8[q]);
                        const double cost = maximize ? v : v * -1.0;  // :236-237
                        const double vi = cost - price[c];
                        if (top2_take(x, vi, c)) cb = cost;
                    }
                }
            }
            if constexpr (Out) {
                const double v = out.value(i);
                const double cost = maximize ? v : v * -1.0;
                const double vi = cost - price[m + i];
                if (top2_take(x, vi, m + i)) cb = cost;
            }
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
        if constexpr (Out) vj = j >= m ? out.value(i) : dense_widen(row[col.at(j)]);
        else vj = dense_widen(row[col.at(j)]);
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
            const T e = row[col.at(c)];
            if (!dense_entry_is<Fin>(e)) continue;
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
            selv[i] = j >= 0 ? dense_widen(A[(size_t)i * (size_t)M + col.at(j)]) : 0.0;
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

template <class T, bool Out, bool Fin>
struct RowsBidLanes<DenseBatchRows<T, Out, true, Fin>> {
    static constexpr bool value = true;
};

template <class T>
__global__ __launch_bounds__(1024) void k_dense_batch_solve(DenseBatchArgs a) {
    const int b = blockIdx.x;
    int n, m;
    dense_batch_shape(a.shapes, a.N, a.M, b, n, m);
    const DenseBatchCheck ck = a.chk[b];
    T vals[kDenseBatchCols];
    const DenseBatchRows<T> rows{static_cast<const T *>(a.mat) + (size_t)b * (size_t)a.N * (size_t)a.M, a.M, m, a.s.maximize,
                                 ck.mref, ck.nvalid, vals};
    batch_solve(a.s, rows, n, m, ck.absmax_bits);
}

// ---- status mode (misslap_solve_dense_batch_status): a verdict per problem instead of all or nothing

struct DenseBatchStatusArgs {
    static constexpr bool kStrided = false;
    static constexpr bool kFinite = false;  // the entry rule of the kernel's instance (finite mode: below)
    DenseBatchArgs d;      // d.shapes: the check pass's sanitised shapes (never null)
    const int *card;       // [B] the guard's cardinalities, or null: no guard in this call
    int fast;              // eps_start = 1 / n_b of each problem (auction_.pyx:568-569)
    int *status;           // [B] MISSLAP_BATCH_STATUS_*
    int *matching_size;    // [B] or null: the guard's cardinality, -1 where it did not run
};

// ... and of the strided family: d.mat is the view's first element, d.N / d.M its extents
struct DenseStridedStatusArgs : DenseBatchStatusArgs {
    static constexpr bool kStrided = true;
    DenseStrides str;
};

// ... and of a finite-mode call (MISSLAP_DENSE_ENTRIES_FINITE): the strided family with "not a NaN" for its entry test.
// A contiguous stack comes here with its natural strides (N * M, M, 1).
struct DenseFiniteStatusArgs : DenseStridedStatusArgs {
    static constexpr bool kFinite = true;
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
// same batch_solve on the same row source.  Args: DenseBatchStatusArgs, or DenseStridedStatusArgs for the strided family.
template <class T, class Args = DenseBatchStatusArgs>
__global__ __launch_bounds__(1024) void k_dense_batch_solve_status(Args a) {
    const int b = blockIdx.x;
    const int n = a.d.shapes[2 * b], m = a.d.shapes[2 * b + 1];
    const DenseBatchCheck ck = a.d.chk[b];
    const int card = a.card && n >= 1 ? a.card[b] : -1;
    const int code = batch_verdict(dense_batch_verdict(ck, n), a.card != nullptr, card, n, ck.bad_price);
    batch_publish_verdict(a.status, a.matching_size, b, code, card);
    if (code != MISSLAP_BATCH_STATUS_OK) {
        batch_condemn(a.d.s, n, ck.mref, (long long)ck.nvalid);
        return;
    }
    BatchSolveArgs s = a.d.s;
    if (a.fast) batch_fast_eps(s, n);
    T vals[kDenseBatchCols];
    if constexpr (Args::kStrided) {
        // a unit column stride is the contiguous row source with sN for its row stride (the same bid, instruction for
        // instruction); any other takes the strided one.  The branch is uniform.
        constexpr bool kFin = Args::kFinite;
        const T *A = static_cast<const T *>(a.d.mat) + (size_t)b * (size_t)a.str.sB;
        if (a.str.sM == 1) {
            const DenseBatchRows<T, false, false, kFin> rows{A, a.str.sN, m, s.maximize, ck.mref, ck.nvalid, vals};
            batch_solve(s, rows, n, m, ck.absmax_bits);
        } else {
            const DenseBatchRows<T, false, true, kFin> rows{A, a.str.sN, m, s.maximize, ck.mref, ck.nvalid, vals, {},
                                                            {a.str.sM, a.str.lane_min_K}};
            batch_solve(s, rows, n, m, ck.absmax_bits);
        }
    } else {
        const DenseBatchRows<T> rows{static_cast<const T *>(a.d.mat) + (size_t)b * (size_t)a.d.N * (size_t)a.d.M, a.d.M, m,
                                     s.maximize, ck.mref, ck.nvalid, vals};
        batch_solve(s, rows, n, m, ck.absmax_bits);
    }
}


// ---- outside mode (misslap_solve_dense_batch_outside): an outside option per row, for partial assignments

struct DenseOutsideArgs {
    static constexpr bool kStrided = false;
    static constexpr bool kFinite = false;
    DenseBatchStatusArgs t;  // t.d.s: Ms = M + N (the carve), p0 / p0_ld the staged augmented prices, prices null;
                             // t.card null: no guard in this call
    const double *outside;   // [B] (outside_ld == 0) or [B][outside_ld]
    long long outside_ld;
    double *prices;          // [B][M] or null: the real columns
    double *outside_prices;  // [B][N] or null
};

struct DenseStridedOutsideArgs : DenseOutsideArgs {
    static constexpr bool kStrided = true;
    DenseStrides str;
};

struct DenseFiniteOutsideArgs : DenseStridedOutsideArgs {  // (finite mode, as DenseFiniteStatusArgs)
    static constexpr bool kFinite = true;
};

// The checks of an outside verdict in their order; EMPTY_ROW, TOO_FEW_VALUES and INFEASIBLE cannot occur.
__device__ __forceinline__ int dense_outside_verdict(const DenseBatchCheck &c, int n) {
    if (n < 1) return MISSLAP_BATCH_STATUS_BAD_SHAPE;
    if (c.has_inf & 2) return MISSLAP_BATCH_STATUS_BAD_OUTSIDE;
    if (c.has_inf & 1) return MISSLAP_BATCH_STATUS_INFINITE_VALUE;
    return MISSLAP_BATCH_STATUS_OK;
}

// The solve of the outside mode: the verdict, batch_solve on the n x (m + n) problem, then the outputs in the caller's
// terms (batch_outside_outputs).  Args: DenseOutsideArgs, or DenseStridedOutsideArgs for the strided family.
template <class T, class Args = DenseOutsideArgs>
__global__ __launch_bounds__(1024) void k_dense_outside_solve(Args a) {
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
    if constexpr (Args::kStrided) {  // (as in k_dense_batch_solve_status)
        constexpr bool kFin = Args::kFinite;
        const T *A = static_cast<const T *>(d.mat) + (size_t)b * (size_t)a.str.sB;
        const unsigned long long nv = ck.nvalid + (unsigned long long)n;
        if (a.str.sM == 1) {
            const DenseBatchRows<T, true, false, kFin> rows{A, a.str.sN, m, s.maximize, m + n, nv, vals,
                                                            {O, a.outside_ld ? 1 : 0}};
            batch_solve(s, rows, n, m + n, ck.absmax_bits);
        } else {
            const DenseBatchRows<T, true, true, kFin> rows{A, a.str.sN, m, s.maximize, m + n, nv, vals,
                                                           {O, a.outside_ld ? 1 : 0}, {a.str.sM, a.str.lane_min_K}};
            batch_solve(s, rows, n, m + n, ck.absmax_bits);
        }
    } else {
        const DenseBatchRows<T, true> rows{static_cast<const T *>(d.mat) + (size_t)b * (size_t)d.N * (size_t)d.M,
                                           d.M,
                                           m,
                                           s.maximize,
                                           m + n,
                                           ck.nvalid + (unsigned long long)n,
                                           vals,
                                           {O, a.outside_ld ? 1 : 0}};
        batch_solve(s, rows, n, m + n, ck.absmax_bits);
    }
    batch_outside_outputs(s_raw, d.s, b, n, m, M, N, po, oo, tid, nt);
}

}  // namespace misslap
