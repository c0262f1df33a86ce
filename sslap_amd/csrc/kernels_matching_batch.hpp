// kernels_matching_batch.hpp -- the reference's Hopcroft-Karp on many small bipartite graphs at once, one workgroup per
// graph (misslap_matching_batch / misslap_matching_dense_batch, include/misslap.h; host side abi_matching_batch.hpp).
// Also the device form of the batch solves' feasibility guard (abi_dense_batch.hpp, abi_sparse_batch.hpp).
//
// The pairings are those of HopcroftKarpSolverCython.solve() (feasibility_.pyx:95-225), i.e. of host_matching.hpp,
// not just some maximum matching:
//   BFS  (:128-168) layer by layer on all wavefronts.  The Dist labels do not depend on the queue order, only on the
//        layers: a row is labelled L + 1 by the first layer L that reaches it (an LDS compare-and-swap from INF picks
//        the one writer that enqueues it).  After the layer in which a free column is first seen the search stops,
//        dist_nil = L + 1; the rows that layer reached keep Dist = dist_nil and are not expanded (`Dist[u] < Dist_nil`).
//   DFS  (:170-211) wavefront 0 alone, for each row free at the start of the phase in ascending order, on an explicit
//        stack of (row, resume position).  The one parallel part is the neighbour scan: the 64 lanes test the stored
//        entries resume .. resume + 63 against `Dist[Pair_V[v]] == Dist[u] + 1` (a free v reads dist_nil) and the
//        lowest qualifying stored index wins.  Nothing the test reads changes until a child fails (its Dist becomes
//        INF, the parent rescans from the entry after the child's) or the whole path succeeds, so the entries are
//        visited in the reference's order.  On a path the row at depth d has Dist d, so Dist[u] is the depth.
// Adjacency is read in stored order from (a) a slice of a packed loc, rows ascending (gaps allowed: an absent row has
// no entries, as cumulative_idxs gives it, :22-46), or (b) the rows of a dense stack of element type E (double, float,
// F16, Bf16: misslap_options.mat_dtype), entry iff v >= 0 by bit pattern in that type (dense_entry_valid: NaN is not an
// entry, -0.0 and +inf are), or (c) the padded candidate lists of the ELL batch (kernels_ell_batch.hpp): the loc source
// with implicit row bounds u * K .. (u + 1) * K and a unit-stride column read of index type E (int, long long), a
// negative column being a hole that no step visits, or (d) a strided dense stack: source (b) with entry (b, i, j) at
// mat[b * sB + i * sN + j * sM] for run-time strides >= 0 (the guard of the strided dense solves and
// misslap_matching_dense_batch_strided; with MISSLAP_DENSE_ENTRIES_FINITE an entry iff the element is not a NaN, the
// rule of a finite-mode solve and of its guard), or (e) a view of a packed loc (the guard of the sparse view solves,
// SparseView of kernels_sparse_batch.hpp): source (a) with entry g of the packed arrays at row mat[g * sN], column
// mat[g * sN + sM], of index type E (int, long long; an int64 index saturates into the int32 range as it is read), for
// graphs the view's check pass found clean.  No value is ever widened here: only the pattern is read.
#pragma once

namespace misslap {

constexpr int kMatchBatchMaxDim = MISSLAP_MATCHING_BATCH_MAX_DIM;
constexpr int kMatchBatchThreads = 256;
constexpr int kMatchInf = INT_MAX;  // the reference's inf of Dist
constexpr int kMatchBatchMaxEntries = INT_MAX - 2 * kWave;  // entries of one graph
// where k_matching_batch reads its adjacency from (DenseStridedFinite: source (d) with the finite-mode entry rule)
enum class MatchSrc { Loc, Dense, Ell, DenseStrided, LocView, DenseStridedFinite };

// per graph of a packed loc, from k_matching_batch_check
struct MatchBatchCheck {
    int max_row;    // INT_MIN: no entries
    int max_col;
    int first_bad;  // first local k failing misslap_hopcroft_karp's entry checks with n / m = max + 1 (-1: none)
    int bad_i, bad_j, bad_prev;  // loc[first_bad] and the row before it
};

struct MatchBatchArgs {
    // source (a): packed loc, graph b = entries offsets[b] .. offsets[b + 1]
    const int *loc;
    const long long *offsets;
    const MatchBatchCheck *mchk;   // misslap_matching_batch: every graph was accepted by the host
    const SparseBatchCheck *schk;  // the sparse solve's guard: only clean problems within the carve are matched
    // source (b): dense stack [B][N][M], graph b = mat[b][:n_b][:m_b]
    // source (c): ELL columns [B][N][M] (M = the K slots of a row), graph b = rows 0 .. n_b - 1 of mat[b]
    const void *mat;               // elements of the kernel's E
    long long N, M;
    const EllBatchCheck *echk;     // source (c): only problems the check pass found clean are matched
    const int *shapes;             // [B][2] or null
    int Ns, Ms;                    // the LDS carve: largest n_b / m_b the launch takes
    int *size;                     // [B] cardinality; -1: not matched by this launch (the host guards it)
    int *left;                     // [B][left_ld] or null
    long long left_ld;
    int *right;                    // [B][right_ld] or null
    long long right_ld;
    long long sB, sN, sM;          // source (d): the element strides of the stack; source (e): sN / sM the strides of an
                                   // entry / of its column in `mat` (the other sources do not read them)
};

// Per graph: the maxima (n = max row + 1, m = max column + 1, feasibility_.pyx:245-246) and the first entry that
// misslap_hopcroft_karp would reject with those n and m (a negative index, or a row below the one before it).
__global__ __launch_bounds__(256) void k_matching_batch_check(const int *loc, const long long *offsets,
                                                              MatchBatchCheck *out) {
    const int b = blockIdx.x;
    const long long s = offsets[b];
    const int nnz = (int)(offsets[b + 1] - s);  // (the host rejects graphs of 2^31 - 1 entries or more)
    __shared__ int s_maxr, s_maxc, s_bad;
    if (threadIdx.x == 0) {
        s_maxr = INT_MIN;
        s_maxc = INT_MIN;
        s_bad = INT_MAX;
    }
    __syncthreads();
    int mr = INT_MIN, mc = INT_MIN, kb = INT_MAX;
    for (int k = threadIdx.x; k < nnz; k += blockDim.x) {
        const long long g = s + k;
        const int r = loc[2 * g], c = loc[2 * g + 1];
        mr = r > mr ? r : mr;
        mc = c > mc ? c : mc;
        if ((r < 0 || c < 0 || (k && r < loc[2 * (g - 1)])) && k < kb) kb = k;
    }
    if (mr != INT_MIN) atomicMax(&s_maxr, mr);
    if (mc != INT_MIN) atomicMax(&s_maxc, mc);
    if (kb != INT_MAX) atomicMin(&s_bad, kb);
    __syncthreads();
    if (threadIdx.x == 0) {
        MatchBatchCheck c;
        c.max_row = s_maxr;
        c.max_col = s_maxc;
        c.first_bad = s_bad == INT_MAX ? -1 : s_bad;
        c.bad_i = c.bad_j = c.bad_prev = 0;
        if (s_bad != INT_MAX) {
            const long long g = s + s_bad;
            c.bad_i = loc[2 * g];
            c.bad_j = loc[2 * g + 1];
            c.bad_prev = s_bad ? loc[2 * (g - 1)] : 0;
        }
        out[b] = c;
    }
}

// LDS of one graph, carved from the dynamic allocation: pair_u, dist, queue (= the DFS stack's rows), the stack's
// resume positions [Ns] each, pair_v [Ms], and for loc input the row starts [Ns + 1].  40 KB at 2048 x 2048 dense,
// 48 KB (49 156 B) from loc.
__host__ __device__ constexpr size_t matching_batch_lds_bytes(long long Ns, long long Ms, bool dense) {
    return sizeof(int) * ((size_t)Ns * 4 + (size_t)Ms + (dense ? 0 : (size_t)Ns + 1));
}

// one BFS edge out of a row of layer L: a free column ends the search after this layer, an unlabelled row joins L + 1
__device__ __forceinline__ void match_bfs_visit(int v, int L, const int *pair_v, int *dist, int *queue, int *s_tail,
                                                bool &found) {
    const int pu = pair_v[v];
    if (pu == -1) {
        found = true;
    } else if (dist[pu] == kMatchInf && atomicCAS(&dist[pu], kMatchInf, L + 1) == kMatchInf) {
        queue[atomicAdd(s_tail, 1)] = pu;
    }
}

template <MatchSrc kSrc, class E = double>
__global__ __launch_bounds__(kMatchBatchThreads) void k_matching_batch(MatchBatchArgs a) {
    constexpr bool kFinite = kSrc == MatchSrc::DenseStridedFinite;  // an edge iff the element is not a NaN
    constexpr bool kStrided = kSrc == MatchSrc::DenseStrided || kFinite, kDense = kSrc == MatchSrc::Dense || kStrided;
    constexpr bool kEll = kSrc == MatchSrc::Ell, kView = kSrc == MatchSrc::LocView;
    constexpr bool kLoc = kSrc == MatchSrc::Loc || kView;  // row starts in LDS, from a packed loc
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x, lane = lane_id(), wave = tid >> 6, nw = T >> 6;
    int n = 0, m = 0;
    long long s = 0;
    int nnz = 0;
    const E *A = nullptr;
    if (kDense) {
        n = a.shapes ? a.shapes[2 * b] : (int)a.N;
        m = a.shapes ? a.shapes[2 * b + 1] : (int)a.M;
        A = static_cast<const E *>(a.mat) + (kStrided ? (size_t)b * (size_t)a.sB : (size_t)b * (size_t)a.N * (size_t)a.M);
    } else if (kEll) {
        // clean: n_b within the stack, no empty row, every column within the carve (none negative: those are holes)
        const EllBatchCheck c = a.echk[b];
        const bool clean = c.n >= 1 && c.empty_row == INT_MAX && c.max_col < a.Ms;
        n = clean ? c.n : 0;
        m = clean ? c.max_col + 1 : 0;
        nnz = (int)(a.N * a.M);  // slots, holes included (the host caps N * K at kMatchBatchMaxEntries)
        A = static_cast<const E *>(a.mat) + (size_t)b * (size_t)a.N * (size_t)a.M;
    } else if (kView) {
        // clean as below, and the slice itself usable (the view's offsets were never seen by the host)
        const SparseBatchCheck c = a.schk[b];
        const bool ok = !(c.err & kErrBadSlice);
        s = ok ? a.offsets[b] : 0;
        nnz = ok ? (int)(a.offsets[b + 1] - s) : 0;
        const bool clean = nnz > 0 && !(c.err & (kErrColNegative | kErrRowsUnsorted | kErrRowGap)) &&
                           c.last_row >= 0 && c.max_row == c.last_row;
        n = clean ? sparse_batch_count(c.max_row) : 0;
        m = clean ? sparse_batch_count(c.max_col) : 0;
        A = static_cast<const E *>(a.mat);
    } else {
        s = a.offsets[b];
        nnz = (int)(a.offsets[b + 1] - s);
        if (a.schk) {
            // clean: rows ascending from 0 without a gap, no negative index -- then n = last row + 1 = max row + 1
            const SparseBatchCheck c = a.schk[b];
            const bool clean = nnz > 0 && !(c.err & (kErrColNegative | kErrRowsUnsorted | kErrRowGap)) &&
                               c.last_row >= 0 && c.max_row == c.last_row;
            n = clean ? c.max_row + 1 : 0;
            m = clean ? c.max_col + 1 : 0;
        } else {
            n = a.mchk[b].max_row + 1;
            m = a.mchk[b].max_col + 1;
        }
    }
    // (kMatchBatchMaxEntries: a stored index plus a wavefront's 64 lanes stays an int)
    if (n < 1 || m < 1 || n > a.Ns || m > a.Ms || nnz > kMatchBatchMaxEntries) {  // not this launch's graph (uniform)
        if (tid == 0) a.size[b] = -1;
        return;
    }
    extern __shared__ __align__(16) unsigned char smem[];
    int *pair_u = reinterpret_cast<int *>(smem);
    int *dist = pair_u + a.Ns;
    int *queue = dist + a.Ns;   // the BFS queue; in the DFS the stack's rows
    int *st_g = queue + a.Ns;   // the stack's resume positions
    int *pair_v = st_g + a.Ns;
    int *row_ptr = pair_v + a.Ms;  // loc input only
    __shared__ int s_tail, s_found, s_cnt;
    // the graph's entries: row and column of local index k (64-bit offsets: 2k overflows an int above 2^30 entries)
    const int *lc = kLoc && !kView ? a.loc + 2 * s : nullptr;
    const int ek = kEll ? (int)a.M : 0;
    auto view_at = [=](int k, long long at) {  // (source (e): entry s + k of the view, saturated into an int)
        if constexpr (kView) {
            const E v = A[(s + k) * a.sN + at];
            return v < (E)INT_MIN ? INT_MIN : (v > (E)INT_MAX ? INT_MAX : (int)v);
        } else {
            return 0;
        }
    };
    auto row_of = [=](int k) {
        if constexpr (kView) return view_at(k, 0);
        else return lc[2 * (long long)k];
    };
    auto col_of = [=](int k) {  // (ELL: a hole reads as -1; a clean graph's columns are below Ms and narrow safely)
        if constexpr (kView) {
            return view_at(k, a.sM);
        } else if constexpr (kEll) {
            const E c = A[k];
            return c < 0 ? -1 : (int)c;
        } else {
            return lc[2 * (long long)k + 1];
        }
    };
    // the stored entries (ELL: the slots) of row u: g_begin(u) .. g_end(u)
    auto g_begin = [=](int u) { return kDense ? 0 : kEll ? u * ek : row_ptr[u]; };
    auto g_end = [=](int u) { return kDense ? m : kEll ? (u + 1) * ek : row_ptr[u + 1]; };
    // a dense stack's entry (u, c), in 64 bits
    const size_t row_stride = kStrided ? (size_t)a.sN : (size_t)a.M;
    auto dense_at = [=](int u, int c) {
        return A[(size_t)u * row_stride + (kStrided ? (size_t)c * (size_t)a.sM : (size_t)c)];
    };

    for (int i = tid; i < n; i += T) pair_u[i] = -1;
    for (int j = tid; j < m; j += T) pair_v[j] = -1;
    if (kLoc) {  // row starts of cumulative_idxs (:22-46): an absent row is an empty run
        for (int k = tid; k < nnz; k += T) {
            const int r = row_of(k), rp = k ? row_of(k - 1) : -1;
            for (int q = rp + 1; q <= r; ++q) row_ptr[q] = k;
        }
        if (tid == 0) row_ptr[n] = nnz;  // (the last entry's row is n - 1)
    }
    // loc rows this short (ELL: rows of at most 16 slots) are expanded one per lane in the BFS, longer ones one per
    // wavefront
    const bool lane_rows = kLoc ? nnz <= 16 * n : kEll && ek <= 16;
    __syncthreads();

    for (int phase = 0;; ++phase) {
        // ---- breadth_first_search (:128-168)
        if (tid == 0) {
            s_tail = 0;
            s_found = 0;
        }
        __syncthreads();
        for (int u = tid; u < n; u += T) {
            if (pair_u[u] == -1) {
                dist[u] = 0;
                queue[atomicAdd(&s_tail, 1)] = u;
            } else {
                dist[u] = kMatchInf;
            }
        }
        __syncthreads();
        int qs = 0, qe = s_tail, nil = kMatchInf;
        for (int L = 0; qs < qe; ++L) {
            bool found = false;
            if constexpr (kDense) {
                for (int x = qs + wave; x < qe; x += nw) {
                    const int u = queue[x];
                    for (int c = lane; c < m; c += kWave)
                        if (dense_entry_is<kFinite>(dense_at(u, c))) match_bfs_visit(c, L, pair_v, dist, queue, &s_tail, found);
                }
            } else if (lane_rows) {
                for (int x = qs + tid; x < qe; x += T) {
                    const int u = queue[x];
                    for (int g = g_begin(u); g < g_end(u); ++g) {
                        const int v = col_of(g);
                        if (!kEll || v >= 0) match_bfs_visit(v, L, pair_v, dist, queue, &s_tail, found);
                    }
                }
            } else {
                for (int x = qs + wave; x < qe; x += nw) {
                    const int u = queue[x], g1 = g_end(u);
                    for (int g = g_begin(u) + lane; g < g1; g += kWave) {
                        const int v = col_of(g);
                        if (!kEll || v >= 0) match_bfs_visit(v, L, pair_v, dist, queue, &s_tail, found);
                    }
                }
            }
            if (found) s_found = 1;
            __syncthreads();
            const int tail = s_tail, any = s_found;
            __syncthreads();  // (everybody has read both before the next layer appends)
            if (any) {
                nil = L + 1;
                break;
            }
            qs = qe;
            qe = tail;
        }
        if (nil == kMatchInf) break;  // no augmenting path left (:205)

        // ---- depth_first_search from every free row, ascending (:199-211), on wavefront 0
        if (wave == 0) {
            int augmented = 0;
            for (int base = 0; base < n; base += kWave) {
                // (a DFS matches its own root and rows that were matched already: the free rows of this chunk stay free
                // until their own turn)
                unsigned long long roots = __ballot(base + lane < n && pair_u[base + lane] == -1);
                while (roots) {
                    const int root = base + __ffsll((long long)roots) - 1;
                    roots &= roots - 1;
                    int depth = 0, u = root;
                    int g = g_begin(u), g1 = g_end(u);
                    for (;;) {
                        int v = -1, pu = -1, k = -1;
                        for (; g < g1; g += kWave) {
                            const int pos = g + lane;
                            int cv = -1;
                            if (pos < g1) {
                                if constexpr (kDense) cv = dense_entry_is<kFinite>(dense_at(u, pos)) ? pos : -1;
                                else cv = col_of(pos);
                            }
                            int cp = -1;
                            bool q = false;
                            if (cv >= 0) {
                                cp = pair_v[cv];
                                const int d = cp == -1 ? nil : dist[cp];
                                q = d != kMatchInf && d == depth + 1;  // :186 (inf == finite + 1 is never true)
                            }
                            const unsigned long long hit = __ballot(q);
                            if (hit) {
                                k = __ffsll((long long)hit) - 1;
                                v = __shfl(cv, k);
                                pu = __shfl(cp, k);
                                g += k + 1;  // resume after the chosen entry
                                break;
                            }
                        }
                        if (k >= 0 && pu != -1) {  // recurse into the column's row (Dist[pu] = depth + 1)
                            queue[depth] = u;
                            st_g[depth] = g;
                            ++depth;
                            u = pu;
                            g = g_begin(u);
                            g1 = g_end(u);
                            continue;
                        }
                        if (k >= 0) {  // a free column: the path succeeds, every level takes its chosen column
                            pair_v[v] = u;
                            pair_u[u] = v;
                            for (int d = lane; d < depth; d += kWave) {
                                const int uu = queue[d], pos = st_g[d] - 1;
                                const int vv = kDense ? pos : col_of(pos);
                                pair_v[vv] = uu;
                                pair_u[uu] = vv;
                            }
                            ++augmented;
                            break;
                        }
                        dist[u] = kMatchInf;  // :197
                        if (depth == 0) break;
                        --depth;  // the parent goes on after the child's entry
                        u = queue[depth];
                        g = st_g[depth];
                        g1 = g_end(u);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                }
            }
            if (lane == 0) s_found = augmented;
        }
        __syncthreads();
        // (a finite dist_nil always admits an augmenting path; this only guarantees the loop ends)
        if (s_found == 0 || phase > n) break;
        __syncthreads();
    }

    // ---- result (:213-225)
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int c = 0;
    for (int i = tid; i < n; i += T) c += pair_u[i] != -1;
    if (c) atomicAdd(&s_cnt, c);
    if (a.left)
        for (long long i = tid; i < a.left_ld; i += T) a.left[(size_t)b * (size_t)a.left_ld + i] = i < n ? pair_u[i] : -1;
    if (a.right)
        for (long long j = tid; j < a.right_ld; j += T)
            a.right[(size_t)b * (size_t)a.right_ld + j] = j < m ? pair_v[j] : -1;
    __syncthreads();
    if (tid == 0) a.size[b] = s_cnt;
}

}  // namespace misslap
