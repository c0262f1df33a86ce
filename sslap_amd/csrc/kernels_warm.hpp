// kernels_warm.hpp -- warm-started re-solve: check a starting price vector, and replace the values of a handle's entries in
// place (the row-major edge layout, the tile-major copy and its overflow lists).  No counterpart in the reference, whose
// AuctionSolver starts every solve from zero prices (auction_.pyx:220); a warm start is its solve loop (:268-306) entered
// with other prices and every person unassigned.  All passes are streaming passes; the host reads back one small block.
#pragma once
#include "device_common.hpp"
#include "kernels_ingest.hpp"
#include "kernels_tiled.hpp"

namespace misslap {

struct WarmStats {
    unsigned long long max_bits;    // bits of max |new value| (value update) / max price (price check)
    unsigned long long delta_bits;  // bits of max |new - old| (value update)
    int err;                        // kErrNonFinite / kErrNegativePrice / kErrNotF32 / kErrPattern
    int pad;
};
constexpr int kErrNegativePrice = 1 << 8;  // a starting price is negative (sign bit set, -0.0 included)
constexpr int kErrNotF32 = 1 << 9;         // a new value is not exact in fp32 on a handle with the 8 B/edge fp32 layout
constexpr int kErrPattern = 1 << 10;       // dense update: the v >= 0 pattern of a row differs from the handle's

// wave max of a non-negative double's bit pattern, then one atomic per wavefront (non-negative doubles order like integers)
__device__ __forceinline__ void warm_max_bits(unsigned long long *dst, unsigned long long b) {
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)(b & 0xffffffffull), off);
        const unsigned hi = __shfl_xor((unsigned)(b >> 32), off);
        const unsigned long long b2 = ((unsigned long long)hi << 32) | lo;
        b = b2 > b ? b2 : b;
    }
    if ((threadIdx.x & 63) == 0 && b > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(dst, b);
}
__device__ __forceinline__ void warm_or_err(int *dst, int err) {
    for (int off = 32; off >= 1; off >>= 1) err |= __shfl_xor(err, off);
    if ((threadIdx.x & 63) == 0 && err) atomicOr(dst, err);
}

// Starting prices: finite and >= 0 with the sign bit clear (bids are ordered by atomicMax on their bit patterns, which is
// the numeric order for non-negative doubles only), and their maximum.
__global__ __launch_bounds__(256) void k_check_prices(const double *p, int n, WarmStats *st) {
    unsigned long long mx = 0ull;
    int err = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(p[j]);
        if (b >> 63) err |= kErrNegativePrice;
        if ((b & 0x7fffffffffffffffull) >= 0x7ff0000000000000ull) err |= kErrNonFinite;
        else if (!(b >> 63)) mx = b > mx ? b : mx;
    }
    warm_max_bits(&st->max_bits, mx);
    warm_or_err(&st->err, err);
}

// Phase 1 of a value update, nothing written but the statistics: every new value finite (and fp32-exact where the handle
// keeps fp32 values), max |new| (eps0 = C / 2, auction_.pyx:242-246), max |new - old|.  `val` is in the caller's sign; the
// handle stores -val for 'min' (:236-237), and so does phase 2.
template <class E>
__global__ __launch_bounds__(256) void k_update_check(E ed, const double *val, long long nnz, int flip, int need_f32,
                                                      WarmStats *st) {
    unsigned long long mx = 0ull, dx = 0ull;
    int err = 0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < nnz; g += stride) {
        const double v = stored_cost(val[g], flip);
        const unsigned long long b = (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
        if (b >= 0x7ff0000000000000ull) {
            err |= kErrNonFinite;
            continue;
        }
        if (need_f32 && (double)(float)v != v) err |= kErrNotF32;
        int c;
        double old;
        ed.load((int)g, c, old);
        const double d = __builtin_fabs(v - old);
        const unsigned long long db = (unsigned long long)__double_as_longlong(d);
        mx = b > mx ? b : mx;
        dx = db > dx ? db : dx;  // (|inf| from an overflowing difference: reported as it is)
    }
    warm_max_bits(&st->max_bits, mx);
    warm_max_bits(&st->delta_bits, dx);
    warm_or_err(&st->err, err);
}

// Phase 2: the row-major layout (create's k_build_edges_f32 / _f64 for the values alone: columns stay).
__global__ __launch_bounds__(256) void k_update_edges_f32(const double *val, long long nnz, int flip, int2 *edges) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < nnz; g += stride) {
        const double v = stored_cost(val[g], flip);
        edges[g].y = __float_as_int((float)v);
    }
}
__global__ __launch_bounds__(256) void k_update_edges_f64(const double *val, long long nnz, int flip, double *v64) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < nnz; g += stride)
        v64[g] = stored_cost(val[g], flip);
}

// Phase 2, tile-major copy: the values of every (person, tile) segment rewritten from the (already updated) row-major
// layout, walking the segment table create built -- nothing of the mapping is derived again.  One thread per segment, in
// table order (adjacent threads: adjacent persons of one tile, i.e. adjacent records).  Where an edge came from:
//   formats 2 / 3: the stored index travels in the record;
//   formats 0 / 1 (ascending columns): the segment holds the row's edges of that tile in stored order, from the first edge
//   with column >= tile * tile_cols on (the binary search of k_tile_count, on the row's own columns).
// Real length of segment k: the next segment's start minus this one's, less the pad of an odd length (k_pack_seg4).
template <class E, int kFmt>
__global__ __launch_bounds__(256) void k_tile_revalue(E ed, const int *cols, int cs, const int *row_ptr, int n_rows, int T,
                                                      int tile_cols, int rb, const int *seg4, long long L, unsigned *tpk) {
    typedef TileFmt<kFmt> F;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < L; k += stride) {
        const int w0 = seg4[k], w1 = seg4[k + 1];
        const int S = w0 & ~1, n = (w1 & ~1) - S - (w0 & 1);
        if (n <= 0) continue;
        const int kk = (int)k;
        const int t = (kk / rb) % T;
        const int i = (kk / rb / T) * rb + kk % rb;
        if (i >= n_rows) continue;
        const int s = row_ptr[i];
        int first = 0;
        if (!F::kG) {  // first stored index of the tile
            const int bound = t * tile_cols;
            int lo = 0, hi = row_ptr[i + 1] - s;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cols[(size_t)cs * (s + mid)] < bound) lo = mid + 1;
                else hi = mid;
            }
            first = lo;
        }
        for (int j = 0; j < n; ++j) {
            const int pos = S + j;
            unsigned *rec = tpk + (size_t)(pos >> 1) * (F::kRec / 4);
            const int gi = F::kG ? (int)reinterpret_cast<const unsigned short *>(rec)[2 + (pos & 1)] : first + j;
            int c;
            double val;
            ed.load(s + gi, c, val);
            if (F::kF64) {
                rec[F::kValOff / 4 + 2 * (pos & 1)] = (unsigned)__double2loint(val);
                rec[F::kValOff / 4 + 2 * (pos & 1) + 1] = (unsigned)__double2hiint(val);
            } else {
                rec[F::kValOff / 4 + (pos & 1)] = (unsigned)__float_as_int((float)val);  // exact: the fp32 layout
            }
        }
    }
}

// ... and the overflow lists (k_ovf_fill's entries {position or stored index, column, value dwords}): formats 0 / 1 copy
// from the rewritten tile-major record at the entry's position, formats 2 / 3 from the row-major layout at the stored index.
template <class E>
__global__ __launch_bounds__(256) void k_ovf_revalue(E ed, const int *row_ptr, int n_rows, const int *ovf_ptr,
                                                     const unsigned *tpk, int fmt, int4 *ovf) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += gridDim.x * blockDim.x) {
        const int a0 = ovf_ptr[i], a1 = ovf_ptr[i + 1];
        for (int a = a0; a < a1; ++a) {
            int4 q = ovf[a];
            unsigned vlo, vhi;
            if (fmt >= 2) {
                int c;
                double v;
                ed.load(row_ptr[i] + q.x, c, v);
                if (fmt & 1) {
                    vlo = (unsigned)__double2loint(v);
                    vhi = (unsigned)__double2hiint(v);
                } else {
                    vlo = (unsigned)__float_as_int((float)v);
                    vhi = 0u;
                }
            } else {
                int g;
                tile_entry(tpk, fmt, q.x, vlo, vhi, g);
            }
            q.z = (int)vlo;
            q.w = (int)vhi;
            ovf[a] = q;
        }
    }
}

// Dense update (the handle was made by misslap_create_dense): one wavefront per row proves that the row's v >= 0 pattern is
// the handle's -- as many valid entries as the row stores, and every stored column still valid (the stored columns of a
// dense row are distinct) -- and gathers mat[row * M + col] into the entry order.
__global__ __launch_bounds__(256) void k_dense_gather(const double *mat, int n_rows, int n_cols, const int *row_ptr,
                                                      const int *cols, int cs, double *val, WarmStats *st) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int err = 0;
    for (int r = blockIdx.x * 4 + wave; r < n_rows; r += gridDim.x * 4) {
        const double *row = mat + (size_t)r * n_cols;
        int cnt = 0;
        for (int c = lane; c < n_cols; c += kWave) cnt += dense_entry_valid(row[c]);
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
        const int s = row_ptr[r], e = row_ptr[r + 1];
        if (cnt != e - s) err |= kErrPattern;
        for (int g = s + lane; g < e; g += kWave) {
            const double v = row[cols[(size_t)cs * g]];
            if (!dense_entry_valid(v)) err |= kErrPattern;
            val[g] = v;
        }
    }
    warm_or_err(&st->err, err);
}

// Candidate lines invalidated after a value update (clear_lines_body, kernels_ingest.hpp).
__global__ __launch_bounds__(256) void k_clear_lines(int2 *cand, int n_rows) { clear_lines_body(cand, n_rows); }

}  // namespace misslap
