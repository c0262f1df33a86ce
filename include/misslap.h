/*
 * misslap.h -- C ABI of libmisslap.so, the MI355X (gfx950) auction LAP solver.
 *
 * This is the drop-in boundary for the reference's bid/assign hot path
 * (OllieBoyne/sslap v0.2.5).  The reference has no C ABI: its boundary is the
 * Python -> Cython `cpdef` layer.  Each entry point below names the reference
 * interface it replaces (file:line relative to the reference checkout).  Plain
 * pointers and sizes only; no torch / numpy types.  All functions return
 * MISSLAP_OK (0) or an error code; misslap_last_error() gives the text.
 *
 * Threading: a handle is single-owner (not thread-safe); distinct handles are
 * independent.  Host arrays are borrowed for the duration of a call only.
 * There is NO CPU fallback: every entry point that computes needs a gfx950 GPU
 * and fails with MISSLAP_ERR_NO_DEVICE / MISSLAP_ERR_HIP otherwise.
 */
#ifndef MISSLAP_H
#define MISSLAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MISSLAP_ABI_VERSION 2
/* ABI history.
 *   1  (rounds 1-2) misslap_options = 88 bytes: the tuning knobs travelled in `reserved[8]`; misslap_meta had no size
 *      field.  Still ACCEPTED: a caller that passes struct_size == 88 to misslap_create* is served with the version-1
 *      meaning of reserved[] and receives the version-1 misslap_meta layout (376 bytes) from misslap_solve /
 *      misslap_finish / misslap_solve_sharded on that handle (INTEGRATION.md section 5 lists both layouts).
 *   2  the knobs are named fields, misslap_meta starts with `struct_size` (the library writes min(struct_size,
 *      sizeof) bytes: a caller built against a shorter version-2 header keeps working when fields are appended),
 *      validity flags of the assignment, misslap_trim_caches.  Additions since: the warm-start entry points,
 *      misslap_solve_dense_batch, misslap_solve_sparse_batch, misslap_solve_dense_batch_status,
 *      misslap_dense_batch_workspace_bytes, misslap_solve_sparse_batch_status, misslap_sparse_batch_workspace_bytes
 *      (with MISSLAP_BATCH_STATUS_NO_ENTRIES .. MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW, codes 8 .. 14),
 *      misslap_options.mat_dtype with MISSLAP_DTYPE_F64 .. MISSLAP_DTYPE_BF16 (the first word of reserved[], which
 *      had to be 0 = MISSLAP_DTYPE_F64 until then; size and offsets of the struct did not change),
 *      misslap_solve_ell_batch, misslap_ell_batch_workspace_bytes, misslap_solve_ell_batch_outside,
 *      misslap_ell_batch_outside_workspace_bytes, misslap_solve_dense_batch_outside,
 *      misslap_dense_batch_outside_workspace_bytes (with MISSLAP_BATCH_STATUS_BAD_OUTSIDE, code 15),
 *      misslap_solve_sparse_batch_outside, misslap_sparse_batch_outside_workspace_bytes,
 *      misslap_solve_dense_batch_status_strided, misslap_solve_dense_batch_outside_strided,
 *      misslap_matching_dense_batch_strided, misslap_solve_sparse_batch_status_view,
 *      misslap_solve_sparse_batch_outside_view, misslap_sparse_batch_view_workspace_bytes,
 *      MISSLAP_DENSE_ENTRIES_FINITE in misslap_options.mat_dtype (no new entry point),
 *      misslap_dense_batch_reverse_finish, misslap_sparse_batch_reverse_finish, misslap_ell_batch_reverse_finish,
 *      misslap_list_batch_finish_workspace_bytes, misslap_solve_points_batch,
 *      misslap_points_batch_workspace_bytes, misslap_points_batch_reverse_finish,
 *      misslap_points_batch_candidates, misslap_solve_points_batch_whitened,
 *      misslap_points_batch_candidates_whitened (with MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS),
 *      misslap_solve_boxes_batch, misslap_boxes_batch_candidates (with MISSLAP_BOXES_METRIC_IOU / _GIOU and
 *      MISSLAP_BATCH_STATUS_BAD_BOX, code 16). */

/* misslap_options.mat_dtype: the element type of a dense stack */
#define MISSLAP_DTYPE_F64 0   /* double */
#define MISSLAP_DTYPE_F32 1   /* float */
#define MISSLAP_DTYPE_F16 2   /* IEEE binary16 */
#define MISSLAP_DTYPE_BF16 3  /* bfloat16: the upper 16 bits of a float */
/* OR-ed into mat_dtype: the entry rule of a dense stack of signed costs (misslap_solve_dense_batch_status has the text).
 * The valid values of mat_dtype are 0 .. 3 and 0x100 .. 0x103; any other bit pattern is MISSLAP_ERR_INVALID. */
#define MISSLAP_DENSE_ENTRIES_FINITE 0x100

#define MISSLAP_OK 0
#define MISSLAP_ERR_INVALID 1    /* malformed arguments / input contract violated */
#define MISSLAP_ERR_HIP 2        /* a HIP runtime call failed */
#define MISSLAP_ERR_NO_DEVICE 3  /* no usable GPU */
#define MISSLAP_ERR_STATE 4      /* call not valid in the handle's current state */

typedef struct misslap_solver misslap_solver;

/* an anonymous union is C11 and C++; this lets a strict C99 build of a GNU-compatible compiler take it as well */
#if defined(__GNUC__) && !defined(__cplusplus) && (!defined(__STDC_VERSION__) || __STDC_VERSION__ < 201112L)
#define MISSLAP_ANONYMOUS __extension__
#else
#define MISSLAP_ANONYMOUS
#endif

/* Options of misslap_create.  Zero-initialise, set struct_size = sizeof, then fill. */
typedef struct misslap_options {
    int32_t struct_size;
    int32_t device;          /* HIP device ordinal */
    int32_t maximize;        /* 1 = problem 'max', 0 = 'min' (auction_.pyx:236-237) */
    float eps_start;         /* > 0 overrides eps0 = C/2 (auction_.pyx:251-252) */
    int64_t max_iter;        /* rounds, auction_.pyx:204,:308 */
    int32_t input_on_device; /* loc / val are device pointers already resident in HBM */
    int32_t tail_threshold;  /* rounds with K <= this run in the persistent one-workgroup kernels (launched once per
                                eps-phase: > 16 bidders, 3..16, <= 2); < 0 = library default (192; 40 without candidate lines); 0 = grid kernels
                                only; max 512 */
    int32_t force_f64_values;/* keep 12 B/edge (int32 col + fp64 val) even when values are fp32-exact */
    int32_t profile;         /* 1: record HIP events around the full-scan bid launches, every launch of the full-scan
                                engine and every tail-kernel launch; 2 / 3: around every bid-kernel launch as well */
    int32_t shard_rank;      /* multi-GPU: this process bids for U positions of its shard only */
    int32_t shard_world;     /* number of shards (1 = single GPU) */
    int32_t rounds_per_sync; /* grid rounds enqueued between host status reads; <= 0 = default */
    /* ---- tuning knobs (all 0 = library default; none of them changes a single bit of the result) ---- */
    int32_t tiled_min_K;     /* LDS-tiled full-scan bid kernel: 0 = default threshold (0.7 N where the rows keep candidate
                                lines, 0.3 N otherwise), < 0 = never, > 0 = minimum K */
    int32_t tiled_shape;     /* its launch shape: 0 = chosen from the average (person, tile) segment length, k + 1 =
                                shape k of misslap.hip:kTiledShapes */
    int32_t tiled_force;     /* != 0 together with tiled_min_K > 0: build the tile-major copy whatever the size and
                                density of the problem (tests) */
    int32_t shard_min_K;     /* multi-GPU shard threshold: 0 = default (the full-scan threshold), > 0 = minimum K of a
                                sharded round, < 0 = shard every grid round */
    int32_t cand_mode;       /* candidate lines: 0 = on, 1 = off (every bid scans its whole row; A/B timing, parity
                                tests), 2 = on, but no maintenance pass ahead of the tail kernels (k_refresh_lines) */
    int32_t partial_in_list_order; /* ignored since round 6 (partial rounds of the full-scan engine always take their bidders
                                in person order: the list-order form lost every A/B); the slot keeps the layout */
    int32_t nnz_limit;       /* > 0 lowers the entry limit of a handle (default 2^31 - 1: int32 row pointers), for
                                tests of that guard */
    int32_t cand_build_max_K;/* > 0: k_bid (re)builds lines only in rounds with at most so many bidders */
    int32_t cand_refresh_min;/* r + 1: a line hit with fewer than r live candidates is rebuilt by k_bid (0 = library
                                default, 1 = never) */
    MISSLAP_ANONYMOUS union { /* seven words that had to be zero; the first one now has a name, and nothing moved */
        int32_t mat_dtype;   /* MISSLAP_DTYPE_*: the element type of `mat` in misslap_solve_dense_batch,
                                misslap_solve_dense_batch_status and misslap_matching_dense_batch (see there); every
                                other entry point takes float64 only and rejects a non-zero value.  An ABI-1 struct
                                and a shorter ABI-2 struct mean 0 */
        int32_t reserved[7]; /* reserved[0] is mat_dtype; reserved[1..6] must be zero */
    };
    void *input_stream;      /* input_on_device only: the hipStream_t the caller's buffers were produced on.  The library
                                then orders its own stream behind that one with an event instead of waiting for the
                                whole device (NULL: hipDeviceSynchronize before the inputs are read -- always safe, but
                                it serialises every other stream of the caller) */
} misslap_options;

/* Result block of misslap_finish: the reference's `meta` dict (auction_.pyx:264,:297-304)
 * plus GPU-side measurements.  The caller sets struct_size first (see the ABI history above). */
typedef struct misslap_meta {
    int32_t struct_size; /* IN: set to sizeof(misslap_meta) before the call; the library writes that many bytes at most */
    int32_t abi_version; /* OUT: MISSLAP_ABI_VERSION of the library */
    float start_eps;     /* auction_.pyx:264 (unrounded fp32) */
    float final_eps;     /* :303 */
    float target_eps;    /* :247 */
    int32_t eCE;         /* :297 */
    int32_t soln_found;  /* :300 */
    int32_t nreductions; /* :299 */
    int64_t its;         /* :298 */
    int64_t n_assigned;  /* :301 */
    int64_t n_rows, n_cols, nnz;
    float obj_f32;       /* get_obj() returns a C float, :489 */
    double obj_f64;      /* the same sum before the cast */
    double setup_ms;     /* :206-207,:265 */
    double solve_ms;     /* :270,:294 */
    /* GPU-side counters */
    uint64_t edges_scanned;      /* sum over all bids of the bidder's row length */
    uint64_t bids_made;
    int64_t grid_rounds;         /* rounds executed by grid kernels */
    int64_t tail_rounds;         /* rounds executed inside the persistent kernel */
    int32_t bytes_per_edge;      /* 8 (int32 col + fp32 val) or 12 (int32 col + fp64 val) */
    int32_t profiled;
    /* valid when options.profile != 0 (HIP-event timings, ms) */
    int64_t bid_launches;        /* grid bid-kernel launches (no-op launches past the end of a phase included) */
    double bid_ms;               /* their summed duration */
    uint64_t bid_edges;          /* edges they scanned */
    int64_t fullscan_launches;   /* of which K == n_rows (every row scanned) */
    double fullscan_ms;
    uint64_t fullscan_edges;
    int64_t tail_launches;
    double tail_ms;
    uint64_t tail_edges;
    int64_t tiled_launches;      /* launches of the LDS-tiled bid kernel (k_bid_tiled), no-ops included */
    double tiled_ms;
    uint64_t tiled_edges;
    int32_t tiled_active;        /* full-scan engine for big rounds: 0 none (k_bid only), 1 k_bid_tiled */
    int32_t tiled_min_K;         /* rounds with K >= this use it */
    uint64_t bid_edges_read;     /* of bid_edges: edges of the rows those launches actually streamed -- the rest are rows a
                                    candidate line answered, counted like the reference counts them but never read.
                                    (These two 8-byte fields were merge_launches / merge_ms, always 0, until round 5.) */
    uint64_t fullscan_edges_read;/* the same for fullscan_edges (the LDS-tiled engine reads every edge it counts) */
    uint64_t shard_edges;        /* multi-GPU: edges scanned in sharded rounds (this rank's share); the rest of
                                    edges_scanned is replicated work, identical on every rank */
    uint64_t cand_hits;          /* bids answered from the person's candidate line (exactly the same bid, no row scan) */
    uint64_t cand_edges;         /* edges of those bidders' rows: part of edges_scanned (reference-equivalent count),
                                    never read from memory */
    double tail_stats[12];       /* tail kernel accounting: [0..2] rounds in chain+solo / team / block mode, [3..5] their
                                    duration in 10-ns ticks, [6] bids, [7] bids answered by candidate lines, [8] line
                                    (re)builds, [9] edges of the rows those lines answered, [10] block rounds finished on
                                    the clean path (no object bid on twice, none unowned), [11] reserved */
    /* validity of the returned assignment, reduced on the device so that `sol` is the only O(N) copy-out (the flags
     * the reference's benchmark harness forms on the host, benchmarking.py:56-64, with size = n_rows and numpy's
     * wrap-around for sol = -1):
     *   complete_assignment  bit 0: np.unique(sol).size == n_rows, bit 1: (sol >= 0).all(), bit 2: (sol < n_rows).all()
     *   valid_assignment     1 if every selected entry (i, sol[i]) exists and its value -- in the caller's sign -- is >= 0 */
    int32_t complete_assignment;
    int32_t valid_assignment;
    int32_t lines_active;        /* 1 = the handle kept candidate lines (0: switched off by option, by row length, or
                                    because eps could fall below the rounding error of a price update, see create) */
    int32_t reserved_i;
    int64_t sharded_rounds;      /* multi-GPU: rounds whose bidders were sharded over the ranks -- each of them issued the
                                    two all-reduces of the exchange step on this rank (0 on a single GPU) */
    /* appended in round 5 */
    int32_t tiled_format;        /* record format of the full-scan engine's tile-major copy (tiled_active = 1): 0 = 6 B/edge
                                    {u16 price slot, f32 value}, 1 = 10 B/edge {slot, f64 value}, 2 / 3 = the same + the u16
                                    stored index of every edge (rows whose columns are not ascending) */
    int32_t phases_with_lines;   /* eps-phases of the solve that ran WITH candidate lines (all of them unless eps fell below
                                    the rounding error of a price update on the way: see misslap_create) */
    int32_t eps_phases;          /* eps-phases of the solve (nreductions + 1 when it ran to its end) */
    int32_t filter_undecided;    /* full scans of the wave-per-row kernel that its fp32 filter could not decide (ties and
                                    near-ties among a row's three best values: answered by the exact scan), saturating;
                                    -1 where this solve ran without the filter: the handle has none, or the current values
                                    or starting prices are outside its range (up to round 6 the slot was always -1) */
} misslap_meta;

/* Snapshot of the round state (tests / multi-GPU driver). */
typedef struct misslap_status {
    int64_t its;          /* rounds done (auction_.pyx:273) */
    int32_t K;            /* num_unassigned (auction_.pyx:198) */
    int32_t nreductions;
    float eps;
    float target_eps;
    int32_t finished;     /* solve loop has broken out (auction_.pyx:275-281) */
    int32_t error_bits;   /* device-side invariant violations (0 = none) */
    int32_t tail_threshold;   /* effective value (library default resolved) */
    int32_t rounds_per_sync;  /* effective value */
    int32_t shard_min_K;      /* multi-GPU: rounds with K >= this are sharded + exchanged, smaller ones replicated */
    int32_t reserved;
} misslap_status;

/* ---- construction: replaces AuctionSolver.__init__ (auction_.pyx:202-265) as reached through
 * _from_sparse (auction_.pyx:575-617) / _from_matrix (:528-571).
 * loc: int32[nnz][2] (row, col), rows ascending with no empty row (the input contract of
 * cumulative_idxs, auction_.pyx:33-48; violations -> MISSLAP_ERR_INVALID instead of the reference's
 * silent garbage); val: double[nnz].  N = max row + 1, M = max col + 1 (:209-210).  The CSR build,
 * |val| maximum (eps0), sign flip for 'min' and the (col, val) edge layout are done on the GPU.
 * The caller's arrays are never written (the Python front-end reproduces the reference's in-place
 * negation of `val` itself). */
int misslap_create(misslap_solver **out, int64_t nnz, const int32_t *loc, const double *val,
                   const misslap_options *opt);

/* ---- dense ingest: replaces the row-major `v >= 0` scan of _from_matrix (auction_.pyx:546-557).
 * mat: double[n_rows][n_cols] on the host; entries < 0 (and NaN) are invalid.  The scan / stream
 * compaction runs on the GPU.  *nnz_out receives the number of valid entries (for the
 * "Fewer than N valid values" guard of :559 the caller compares it with n_rows BEFORE solving;
 * create fails with MISSLAP_ERR_INVALID when a row is empty, or when the matrix holds 2^31 - 1 or more valid
 * entries -- they are counted in 64 bits on the device, *nnz_out is exact).
 * options.input_on_device: `mat` (here) / `loc`, `val` (misslap_create) are device pointers.  The library then
 * waits for the whole device (hipDeviceSynchronize) before reading them, so buffers still being produced on any
 * stream of the caller are safe to pass -- or, with options.input_stream set, only for the work already enqueued on
 * that stream (an event the solver's stream waits for). */
int misslap_create_dense(misslap_solver **out, int64_t n_rows, int64_t n_cols, const double *mat,
                         const misslap_options *opt, int64_t *nnz_out);

int misslap_destroy(misslap_solver *h);

/* N, M, nnz as the solver sees them (auction_.pyx:209-212). */
int misslap_dims(const misslap_solver *h, int64_t *n_rows, int64_t *n_cols, int64_t *nnz);

/* ---- the whole solve loop: replaces AuctionSolver.solve() (auction_.pyx:268-306).
 * person_to_object_out: int32[n_rows] on the host (-1 = unassigned), may be NULL. */
int misslap_solve(misslap_solver *h, int32_t *person_to_object_out, misslap_meta *meta);

/* ---- stepwise interface (multi-GPU driver, round-level parity tests).  One grid round is
 *   misslap_round_bid      bid phase (auction_.pyx:339-365) over this shard's bidders + per-object
 *                          maximum of the shard's bids (first half of :375-385).  Only rounds with
 *                          K >= status.shard_min_K are sharded (and need the two exchanges); in smaller
 *                          rounds every rank bids for every list position and no exchange is needed.
 *   [exchange: all-reduce MAX over the best-key buffer, see misslap_exchange_buffers]
 *   misslap_round_tiebreak earliest bidder in list order wins equal bids (strict '>' of :379)
 *   [exchange: all-reduce MIN over the best-position buffer]
 *   misslap_round_apply    assignment phase (:388-429) + push_all_left (:137-162, :430); its += 1
 * Every call is a no-op once K == 0, K <= tail_threshold or its >= max_iter, so a driver may
 * enqueue rounds blindly and read the status afterwards. */
int misslap_round_bid(misslap_solver *h);
int misslap_round_tiebreak(misslap_solver *h);
int misslap_round_apply(misslap_solver *h);
/* All remaining rounds with 0 < K <= tail_threshold, inside the persistent kernels (no host round trip until K == 0). */
int misslap_run_tail(misslap_solver *h);
/* Synchronise and read the round state. */
int misslap_get_status(misslap_solver *h, misslap_status *st);
/* Loop control of solve() after a round (auction_.pyx:275-292): terminate(), eps reduction and
 * assignment reset.  Sets *finished. */
int misslap_phase_end(misslap_solver *h, int32_t *finished);
/* eps-complementary-slackness test, eCE_satisfied (auction_.pyx:443-485), on the current state. */
int misslap_check_ece(misslap_solver *h, float eps, int32_t *satisfied);
/* meta + result copy-out (auction_.pyx:297-306). */
int misslap_finish(misslap_solver *h, int32_t *person_to_object_out, misslap_meta *meta);

/* Device pointers of the two per-object exchange buffers (int64 best key = bid bits + 1, 0 = none;
 * int32 best position, INT32_MAX = none), n_objects entries each, for RCCL all-reduces. */
int misslap_exchange_buffers(misslap_solver *h, void **best_key, void **best_pos, int64_t *n_objects);
/* Run all of the handle's GPU work on this hipStream_t (default: a private stream). */
int misslap_set_stream(misslap_solver *h, void *hip_stream);

/* ---- multi-GPU: the exchange step behind the C ABI (one process per GPU, persons of a round sharded over the
 * ranks; the reference has no counterpart: it is single-threaded, auction_.pyx:6).
 * A communicator provides the two collectives a sharded round needs -- all-reduce MAX over the int64 best-key buffer
 * and all-reduce MIN over the int32 best-position buffer (misslap_exchange_buffers) -- issued on the solver's HIP
 * stream between the round kernels, with no host read inside a round.
 *   RCCL over xGMI:  rank 0 calls misslap_rccl_unique_id, the 128 bytes are handed to every rank by any means the
 *                    application has (file, socket, MPI, torch.distributed object broadcast ...), every rank calls
 *                    misslap_comm_init_rccl.  librccl.so.1 is opened at run time (dlopen).
 *   custom:          caller-provided callbacks (another transport; the tests' gloo / in-process stand-ins).
 * Every rank creates its handle on the same input with options.shard_rank / shard_world set and calls
 * misslap_solve_sharded; every rank receives the same assignment. */
typedef struct misslap_comm misslap_comm;
#define MISSLAP_RCCL_ID_BYTES 128
typedef struct misslap_comm_ops {
    int32_t struct_size;
    int32_t rank, world;
    int32_t reserved;
    void *ctx;
    /* in-place all-reduce of `count` elements of a DEVICE buffer, ordered after the work already enqueued on
     * `hip_stream` and before work enqueued afterwards; return 0 on success */
    int (*allreduce_max_i64)(void *ctx, void *buf, int64_t count, void *hip_stream);
    int (*allreduce_min_i32)(void *ctx, void *buf, int64_t count, void *hip_stream);
} misslap_comm_ops;
int misslap_rccl_unique_id(void *id_out /* MISSLAP_RCCL_ID_BYTES */);
/* Self-check of the RCCL binding, needs no GPU: opens librccl exactly as misslap_comm_init_rccl does and reports how many
 * of the entry points the exchange uses were resolved (*n_symbols of MISSLAP_RCCL_SYMBOLS: ncclGetUniqueId,
 * ncclCommInitRank, ncclCommDestroy, ncclAllReduce, ncclGetErrorString, ncclCommCount), the enumerator VALUES the
 * library passes to ncclAllReduce -- enums[0..3] = ncclInt32, ncclInt64, ncclMax, ncclMin as compiled in (rccl.h:
 * ncclDataType_t, ncclRedOp_t) --, enums[4] = the size of the unique id it assumes, enums[5] = ncclGetVersion() of the
 * copy it bound to, and that copy's path.  A test compares them with the installed rccl.h (tests/test_cabi.py). */
#define MISSLAP_RCCL_SYMBOLS 6
int misslap_rccl_selfcheck(int32_t *n_symbols, int32_t enums[6], char *lib_path, int32_t lib_path_len);
int misslap_comm_init_rccl(misslap_comm **out, const void *unique_id, int32_t rank, int32_t world, int32_t device);
int misslap_comm_init_custom(misslap_comm **out, const misslap_comm_ops *ops);
int misslap_comm_destroy(misslap_comm *comm);
/* What a communicator is, as the transport itself reports it: *kind = 1 RCCL / 0 custom; *rank, *world as given at
 * creation; *transport_ranks = ncclCommCount of the RCCL communicator (the number of ranks RCCL itself sees -- a
 * multi-GPU run proves with it that N ranks took part), for a custom one the world size of its ops.  Any pointer
 * may be NULL. */
int misslap_comm_info(const misslap_comm *comm, int32_t *kind, int32_t *rank, int32_t *world, int32_t *transport_ranks);
/* AuctionSolver.solve() (auction_.pyx:268-306) over all ranks of `comm` (NULL: no exchange, a single rank).  Only
 * rounds with K >= status.shard_min_K are sharded and exchanged; all others are replicated. */
int misslap_solve_sharded(misslap_solver *h, misslap_comm *comm, int32_t *person_to_object_out, misslap_meta *meta);

/* The same loop over caller-provided round operations: what misslap_solve_sharded runs with the handle's own
 * operations.  Exposed so that the loop -- shard / replicate decision, collective sequence, loop control -- can be
 * driven without a GPU (tests/test_dist_gloo.py: numpy stand-ins for the round kernels, gloo for the exchange). */
typedef struct misslap_round_ops {
    int32_t struct_size;
    int32_t tail_threshold;
    int32_t shard_min_K;
    int32_t rounds_per_sync;
    int64_t max_iter;
    void *ctx;
    int (*status)(void *ctx, int64_t *K, int64_t *its); /* synchronise and read the round state */
    int (*round_bid)(void *ctx);
    int (*round_tiebreak)(void *ctx);
    int (*round_apply)(void *ctx);
    int (*run_tail)(void *ctx);
    int (*phase_end)(void *ctx, int32_t *finished);
    void *best_key;    /* int64[n_objects] exchange buffer (device memory for the GPU operations) */
    void *best_pos;    /* int32[n_objects] */
    int64_t n_objects;
    void *stream;      /* handed to the communicator's callbacks */
    /* Optional (both or neither): a status read that does not drain the queue.  status_post enqueues a copy of the
     * round state behind everything issued so far into slot 0 / 1; status_take waits for THAT copy only.  With them
     * the replicated rounds are issued in batches whose status trails by one batch (K never grows inside an
     * eps-phase and a round that is not live is a no-op, so a batch issued on a stale "go on" is harmless). */
    int (*status_post)(void *ctx, int32_t slot);
    int (*status_take)(void *ctx, int32_t slot, int64_t *K, int64_t *its);
    int32_t large_round_K;          /* while K > this ... */
    int32_t rounds_per_sync_large;  /* ... a batch has so many rounds (<= 0: rounds_per_sync) */
} misslap_round_ops;
int misslap_drive_sharded(const misslap_round_ops *ops, misslap_comm *comm);

/* ---- state copy-out for parity tests (all host buffers, any may be NULL):
 * prices double[M] (auction_.pyx:169), unassigned list int32[N] (first K valid, :199),
 * person_to_object int32[N] (:177), object_to_person int32[M] (:178). */
int misslap_get_state(misslap_solver *h, double *prices, int32_t *unassigned, int32_t *person_to_object,
                      int32_t *object_to_person);

/* ---- warm-started re-solve (no counterpart in the reference, whose AuctionSolver starts every solve from zero prices,
 * auction_.pyx:220).  The auction may start from any prices with every person unassigned: a problem whose costs drifted a
 * little is re-solved from the prices of the last solve with a small eps, on the handle that already holds its graph
 * (no second create, no second feasibility guard).  Prices are those of the MAXIMISED problem, i.e. for 'min' the prices
 * of the negated costs, in and out alike.  Single-GPU handles only (world == 1; sharded handles: MISSLAP_ERR_STATE).
 *
 * The current prices, n_cols doubles, into host memory or (out_on_device != 0) device memory. */
int misslap_get_prices(misslap_solver *h, double *out, int32_t out_on_device);
/* New values for the handle's entries, in the order of the create-time `loc` and in the caller's sign (the library
 * negates for 'min' on the device; the caller's buffer is never written).  Sparsity and stored order do not change.
 * on_device: `val` is a device pointer, produced on `input_stream` (NULL: the library waits for the whole device first).
 * *max_abs_change (may be NULL) receives max |new - old|: the natural eps_start of the next misslap_resolve (prices that
 * satisfied eps-CS for the old values satisfy (eps + 2 delta)-CS for the old assignment under the new ones).
 * All or nothing: NaN / infinity, a wrong nnz, or -- on a handle that keeps 8 B/edge fp32 values because its values at
 * create were all fp32-exact -- a value that is not exact in fp32 is MISSLAP_ERR_INVALID and leaves the handle's values
 * unchanged (create with options.force_f64_values = 1 to update with arbitrary doubles).  Every layout that carries a
 * value is rewritten (row-major edges, the tile-major copy), the candidate lines are invalidated, and what create derived
 * from max|val| is derived again.  On a handle on which no round has run since create or the last resolve, the next
 * misslap_solve starts from the eps0 of the new values. */
int misslap_update_values(misslap_solver *h, const double *val, int64_t nnz, int32_t on_device, void *input_stream,
                          double *max_abs_change);
/* The same for a handle made by misslap_create_dense: mat is double[n_rows][n_cols] with the shape given at create.  Its
 * v >= 0 pattern must be the handle's: as many valid entries in every row, and every stored entry still valid (otherwise
 * MISSLAP_ERR_INVALID, the handle unchanged). */
int misslap_update_dense(misslap_solver *h, const double *mat, int32_t on_device, void *input_stream,
                         double *max_abs_change);
/* Solve again, on a created or a solved handle, starting from `prices` (n_cols doubles, host or device memory; NULL: the
 * handle's current prices) with every person unassigned, its = nreductions = 0, eps0 = eps_start if eps_start > 0, else
 * C / 2 with C = max |val| of the current values (auction_.pyx:241-249), and the same theta and target eps = 1 / N.  The
 * result is what the reference's solve() returns when its prices start at `prices` instead of zeros, bit for bit.  Prices
 * must be finite and >= 0 with the sign bit clear (bids are ordered by their bit patterns, the numeric order of non-negative
 * doubles only): checked on the device before anything is reset, MISSLAP_ERR_INVALID otherwise.  Outputs as misslap_solve. */
int misslap_resolve(misslap_solver *h, const double *prices, int32_t prices_on_device, float eps_start,
                    int32_t *person_to_object_out, misslap_meta *meta);

/* Device properties of the GPU the handle runs on (name buffer >= 128 bytes). */
int misslap_device_info(int32_t device, char *name, int32_t name_len, int32_t *compute_units,
                        int64_t *hbm_bytes);
/* The device's UUID as 32 hex digits + NUL (buffer >= 33 bytes): tells two ranks that share a GPU from two that do not. */
int misslap_device_uuid(int32_t device, char *uuid_hex, int32_t len);
/* What the HBM of THIS device delivers to a streaming kernel of the library, measured now: a read-only pass (every
 * workgroup walks one contiguous chunk, four 16-byte non-temporal loads in flight per lane) and a copy of the same
 * shape over `bytes` bytes, `reps` timed launches each; GB/s of bytes read, and of bytes read + written.  The "achievable" peak next to the data sheet's 8 TB/s that
 * the roofline figures of bench.py are quoted against. */
int misslap_measure_hbm(int32_t device, int64_t bytes, int32_t reps, double *read_GBs, double *copy_GBs);

/* Feasibility guard of the front-end: maximum bipartite matching (Hopcroft-Karp) on the host, the reference's
 * c_hopcroft_solve / sslap.hopcroft_solve (feasibility_.pyx:95-283; called at auction_.pyx:562-566, :608-612).
 * loc: int32[nnz][2] (row, col), rows ascending.  size: cardinality; left_pairings int32[n_rows] / right_pairings
 * int32[n_cols] (-1 = unmatched, either may be NULL) reproduce the reference's result() arrays.  Needs no GPU. */
int misslap_hopcroft_karp(const int32_t *loc, int64_t nnz, int32_t n_rows, int32_t n_cols, int32_t *size,
                          int32_t *left_pairings, int32_t *right_pairings);

/* The same maximum matching computed on the GPU (BFS-layered, csrc/kernels_matching.hpp): equal cardinality -- the only
 * thing that reaches the auction path (auction_.pyx:565, :611) -- but not necessarily the same pairings.  loc is a
 * host array; *phases (may be NULL) receives the number of augmentation phases.  Needs a GPU. */
int misslap_matching_gpu(const int32_t *loc, int64_t nnz, int32_t n_rows, int32_t n_cols, int32_t device, int32_t *size,
                         int32_t *left_pairings, int32_t *right_pairings, int32_t *phases);
/* The same matcher on the graph a solver handle already holds in device memory (no host copy of the entries, no second
 * upload): what the front-end's feasibility guard (auction_.pyx:562-566, :608-612) uses once the handle exists. */
int misslap_matching_of(misslap_solver *h, int32_t *size, int32_t *phases);

/* Host-side caches: a destroyed handle parks its idle HIP stream, pinned status mirror and events (at most 8 bundles)
 * and its freed device blocks for the next handle -- BY DEFAULT up to 4 GB in total (never more than 1 / 64 of the
 * device's memory), blocks of up to 1 GB, at most 64 blocks: i.e. after misslap_destroy the process may still hold up to
 * 4 GB of HBM that an embedding application (a PyTorch process, say) does not see as free until it calls
 * misslap_trim_caches or lowers the limits (misslap_set_cache_limits(0, 0, 0) = park nothing).  This releases all of them
 * (streams destroyed, device and pinned memory freed); *freed_bytes (may be NULL) receives the device bytes returned.
 * Call it when the embedding application needs the memory back; never while another thread creates / destroys handles
 * on a stream that may still use a parked block (the entry point synchronises every device it frees on). */
int misslap_trim_caches(int64_t *freed_bytes);
/* Limits of the device-block cache: total bytes parked, largest block parked, number of blocks.  Defaults: min(4 GB,
 * device memory / 64) / a quarter of that / 64 blocks -- the blocks of one or two problems of the BASELINE sizes (0.9 GB
 * per C3 handle), because hipMalloc + hipFree of those cost a millisecond per create / destroy pair and hipFree waits
 * for EVERY stream of the device; MISSLAP_BLOCK_CACHE_MB in the environment sets the first two at start-up (0 = park
 * nothing).  An application that solves many LARGE problems at a time raises them (bench.py --concurrent: C3, 16 at a
 * time: 4 GB per solve in flight); one that must not lose HBM to the library lowers them. */
int misslap_set_cache_limits(int64_t max_total_bytes, int64_t max_block_bytes, int32_t max_blocks);

/* ---- many independent problems at a time (round 5; no counterpart in the reference, whose own harness solves its
 * problems in a loop: benchmarking.py:84-142).  During ~90 % of a solve one problem occupies ONE of the GPU's 256 compute
 * units, and a GPU fed from many queues retires only ~90 000 launches per second over all of them, so solves issued from
 * many host threads stall at 6-8x the single-solve throughput.  misslap_solve_batch solves the n handles in LOCKSTEP:
 * groups of `group_size` problems (0 = default, 12) share one HIP stream and every launch of the solve loop that several of
 * them issue at the same point is ONE launch (csrc/host_batch.hpp).  Each handle goes through exactly the sequence of
 * kernels misslap_solve would have launched for it: person_to_object_out[k] / meta_out[k] are what misslap_solve(handles[k])
 * returns, bit for bit -- except the TIMING fields of the meta (solve_ms and the per-kernel times): inside a batch they are
 * wall time of the handle's fiber, which includes the other problems of its group.  The handles must be unsolved, unsharded, unprofiled, on one device, and have the same number of
 * persons (rows; objects and entries may differ).  meta_out: n pointers to structs with struct_size set (the array and
 * any of its entries may be NULL, like the output pointers); *info (may be NULL) says how many launches went out for how many recorded. */
typedef struct misslap_batch_info {
    int32_t groups;            /* streams / host threads used */
    int32_t reserved;
    int64_t calls_recorded;    /* launches + asynchronous copies / fills the n solve loops asked for */
    int64_t launches_issued;   /* ... and what went onto the streams after merging */
    double wall_ms;
    /* where the host threads of the groups spent their time (summed over groups): running the problems' solve loops up to
     * their next wait, merging + issuing launches, waiting for the device (polling status words / draining the stream) */
    double host_ms_fibers, host_ms_flush, host_ms_wait;
} misslap_batch_info;
int misslap_solve_batch(misslap_solver *const *handles, int32_t n, int32_t *const *person_to_object_out,
                        misslap_meta *const *meta_out, int32_t group_size, misslap_batch_info *info);

/* ---- many small DENSE problems in one call (no counterpart in the reference, whose own benchmark solves small dense
 * matrices one at a time: benchmarking.py:146).  mat is double[B][N][M] (row-major, problem b at offset b * N * M,
 * counted in 64 bits); problem b is mat[b][:n_b][:m_b] with (n_b, m_b) = shapes[2b], shapes[2b + 1] (shapes NULL: every
 * problem is N x M; entries outside the slice are never read).  Entries are read with _from_matrix's rule (v >= 0 is an
 * entry; negatives and NaN are not, auction_.pyx:546-557).  Each problem is solved by ONE workgroup of ONE launch, its
 * whole state in LDS (csrc/kernels_dense_batch.hpp), and its result is exactly what _from_matrix(mat[b][:n_b][:m_b],
 * ...).solve() returns: same assignment, its, nreductions, eCE, objective and price bits.
 *   opt            device, maximize, eps_start, max_iter, mat_dtype (below), input_on_device (mat and prices_in are device
 *                  pointers) and input_stream (as for misslap_create_dense); every other field must be 0.
 *   eps_start      float[B] host array or NULL: problem b's eps_start (> 0 overrides C / 2, auction_.pyx:251-252); NULL =
 *                  opt->eps_start for every problem.  (The front-end's `fast` passes 1 / n_b here, :568-569.)
 *   prices_in      double[B][M] or NULL: problem b starts from prices_in[b][:m_b] as misslap_resolve does (every person
 *                  unassigned, its = nreductions = 0); finite and >= 0 with the sign bit clear.
 *   cardinality_check  != 0: the Hopcroft-Karp guard of _from_matrix (auction_.pyx:562-566), per problem: for B >= 64 on
 *                  the device (the kernel of misslap_matching_dense_batch, enqueued behind the validation pass), for
 *                  smaller batches on the host.
 *   sol            int32[B][N]: sol[b][:n_b] the assignment (-1 = unassigned), -1 beyond n_b.
 *   prices_out     double[B][M] or NULL: final prices of the maximised problem; 0 beyond m_b.
 *   out_on_device  != 0: sol and prices_out are device pointers (meta is always host memory).
 *   meta           host array of B misslap_dense_batch_meta, meta[0].struct_size set (the stride of the array), or NULL.
 *   info           may be NULL.
 * All or nothing: every problem is validated before any is solved.  A failing problem gives MISSLAP_ERR_INVALID and the
 * text "problem <b>: <what _from_matrix raises for that slice>" for the first failing b, in _from_matrix's order: fewer
 * valid values than rows, an empty row, +inf, the matching guard, then bad starting prices.  N and M are at most
 * MISSLAP_DENSE_BATCH_MAX_DIM (larger problems: misslap_create_dense / misslap_solve_batch).  Every solve ends after at
 * most max_iter rounds.
 *   The element type of mat is opt->mat_dtype (MISSLAP_DTYPE_F64 = 0, _F32, _F16, _BF16).  The parameter keeps its
 * declared type: with another mat_dtype, pass the stack's address cast to const double *.  mat then points to B * N * M
 * elements of that type, read in place: strides are counted in elements and only the element's own alignment is needed
 * (a row of a 2-byte stack may start on any 2-byte boundary), on the host and on the device, with and without a
 * workspace (misslap_dense_batch_workspace_bytes does not depend on the type).  An entry is valid iff v >= 0 in its own
 * type -- the same set as after widening: -0.0 and +inf are entries, NaN and negatives are not -- and +inf is
 * MISSLAP_BATCH_STATUS_INFINITE_VALUE as before.  Every value is widened to double as it is read, which is exact
 * (binary16 subnormals included), and everything downstream is the double arithmetic of the float64 path on that value:
 * C = max |v|, eps0, bids, prices, eCE, obj_f64, obj_f32.  prices_in, prices_out and meta stay float64.  The result is
 * bit for bit that of the same call on the widened stack.  A mat_dtype outside 0 .. 3 is MISSLAP_ERR_INVALID. */
#define MISSLAP_DENSE_BATCH_MAX_DIM 1024
typedef struct misslap_dense_batch_meta {
    int32_t struct_size;  /* IN (element 0 only): sizeof(misslap_dense_batch_meta); the stride of the array */
    int32_t n_rows;       /* n_b */
    int32_t n_cols;       /* the reference's M: max valid column + 1 (auction_.pyx:209-212) */
    int32_t eCE;          /* :297 */
    int64_t nnz;          /* valid entries of the slice */
    int64_t its;          /* :298 */
    int64_t n_assigned;   /* :301 */
    int32_t nreductions;  /* :299 */
    int32_t soln_found;   /* :300 */
    float start_eps;      /* :264 (unrounded fp32) */
    float final_eps;      /* :303 */
    float target_eps;     /* :247 */
    float obj_f32;        /* get_obj() returns a C float, :489 */
    double obj_f64;       /* the same sum before the cast */
    uint64_t bids_made;
} misslap_dense_batch_meta;
typedef struct misslap_dense_batch_info {
    int32_t threads;      /* workgroup size of the solve launch */
    int32_t lds_bytes;    /* dynamic LDS per workgroup */
    double check_ms;      /* validation launch + read-back (wall) */
    double matching_ms;   /* guard time: device kernel (HIP events) plus any host-guarded problems (wall) */
    double solve_ms;      /* the solve launch (HIP events) */
    double wall_ms;       /* the whole call */
} misslap_dense_batch_info;
int misslap_solve_dense_batch(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                              const float *eps_start, const double *prices_in, int32_t cardinality_check,
                              const misslap_options *opt, int32_t *sol, double *prices_out, int32_t out_on_device,
                              misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);

/* ---- the dense batch with a verdict per problem instead of all or nothing, and in stream order.
 * misslap_solve_dense_batch_status takes the stack of misslap_solve_dense_batch and never fails for a reason that belongs
 * to one problem: status[b] names the first check problem b failed, in misslap_solve_dense_batch's order, and every
 * problem with status 0 is solved -- sol, prices and meta bit for bit what misslap_solve_dense_batch gives for it.  A
 * problem with another status takes no part in the solve launch (its workgroup leaves at once): sol[b][:] = -1,
 * prices_out[b][:] = 0, meta[b] = {n_rows = n_b, n_cols = max valid column + 1, nnz = valid entries, every other
 * result field 0} (all three 0 for MISSLAP_BATCH_STATUS_BAD_SHAPE).  Hitting max_iter is no error, as before.
 *   shapes, prices_in, cardinality_check, sol, prices_out   as for misslap_solve_dense_batch.  The guard always runs
 *                  on the device here (its kernel needs no read-back), also below 64 problems, where one graph on one
 *                  compute unit is slower than the host matcher.
 *   fast           != 0: problem b starts at eps = (float)(1.0 / n_b), formed in the kernel (auction_.pyx:568-569);
 *                  0: opt->eps_start for every problem.
 *   opt            as for misslap_solve_dense_batch; with a workspace input_on_device must be set and input_stream is
 *                  not read.
 *   stream         a hipStream_t; NULL is the null stream.  Only read with a workspace.
 *   workspace      NULL: the library uploads host arrays, allocates its scratch, works on its own stream and
 *                  synchronises once, at the end; mat / prices_in follow opt->input_on_device, sol / prices_out / status /
 *                  matching_size follow out_on_device, shapes and meta are host arrays, and shapes is checked on the host
 *                  (an entry outside 1 .. N x 1 .. M is MISSLAP_ERR_INVALID, as before).
 *                  Not NULL: device memory of at least misslap_dense_batch_workspace_bytes(...) bytes, 256-byte aligned.
 *                  EVERY pointer argument except opt and info is then a device pointer (meta: B records of
 *                  sizeof(misslap_dense_batch_meta), struct_size not read; out_on_device must be set) and the call is
 *                  stream-ordered: its three launches go onto `stream`, it allocates and frees nothing, creates no
 *                  event, waits for nothing, copies nothing, and returns once the launches are enqueued.  The
 *                  workspace and every argument array belong to the call until the stream has passed it.  A device
 *                  shapes entry outside 1 .. N x 1 .. M gives MISSLAP_BATCH_STATUS_BAD_SHAPE and nothing of that
 *                  problem is read: the check pass writes the shapes the later kernels use into the workspace.
 *   status         int32[B], required.
 *   matching_size  int32[B] or NULL: the guard's cardinality of problem b (for MISSLAP_BATCH_STATUS_INFEASIBLE: "only
 *                  involves <matching_size> out of <n_b> rows"); -1 where the guard did not run.
 *   meta           required with a workspace; else as for misslap_solve_dense_batch.
 *   info           may be NULL; threads and lds_bytes are set (without a workspace wall_ms too), the other times are 0.
 * Only what is wrong with the whole call is an error: B, N, M, a NULL mat / sol / status, the options, a workspace that
 * is too small or misaligned.
 *
 * Signed costs: opt->mat_dtype = MISSLAP_DTYPE_* | MISSLAP_DENSE_ENTRIES_FINITE.  An element is then an entry iff it is
 * not a NaN in its own type: negative values, -0.0 and subnormals are entries, and NaN is the one way to say "no
 * edge".  An entry of +inf or -inf gives MISSLAP_BATCH_STATUS_INFINITE_VALUE.  Everything else is unchanged: n_cols is
 * the largest column with an entry plus 1, C = max |v| over the entries, the checks and their order, shapes, fast,
 * prices_in, both modes of the call, and the workspace size.  The result of a problem with status 0 is the reference's
 * sparse solver on its entries in row-major order.  The flag is taken by this call,
 * misslap_solve_dense_batch_outside (an outside value may then be any finite double: a NaN in a row < n_b is
 * MISSLAP_BATCH_STATUS_BAD_OUTSIDE, an infinity MISSLAP_BATCH_STATUS_INFINITE_VALUE), both _strided forms,
 * misslap_matching_dense_batch and misslap_matching_dense_batch_strided (an edge iff not a NaN; also the rule of this
 * call's guard).  A contiguous stack in this mode is read by the kernels of the strided family with its natural
 * strides.  misslap_solve_dense_batch itself does not take the flag (MISSLAP_ERR_INVALID): use this call. */
#define MISSLAP_BATCH_STATUS_OK 0                /* solved */
#define MISSLAP_BATCH_STATUS_TOO_FEW_VALUES 1    /* fewer valid values than rows */
#define MISSLAP_BATCH_STATUS_EMPTY_ROW 2         /* a row without a valid entry */
#define MISSLAP_BATCH_STATUS_INFINITE_VALUE 3    /* a valid entry is +inf */
#define MISSLAP_BATCH_STATUS_INFEASIBLE 4        /* the matching guard: no assignment of every row (cardinality_check) */
#define MISSLAP_BATCH_STATUS_PRICE_NOT_FINITE 5  /* starting prices hold a NaN or an infinity */
#define MISSLAP_BATCH_STATUS_PRICE_NEGATIVE 6    /* starting prices with the sign bit set */
#define MISSLAP_BATCH_STATUS_BAD_SHAPE 7         /* shape outside 1 .. N x 1 .. M (device shapes only) */
int misslap_solve_dense_batch_status(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                                     int32_t fast, const double *prices_in, int32_t cardinality_check,
                                     const misslap_options *opt, void *stream, void *workspace, int64_t workspace_bytes,
                                     int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
                                     int32_t *matching_size, misslap_dense_batch_meta *meta,
                                     misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_dense_batch_status of this size needs (the check records, the
 * sanitised shapes and, with cardinality_check, the cardinalities); -1 for B < 1 or N, M outside
 * 1 .. MISSLAP_DENSE_BATCH_MAX_DIM.  Needs no GPU.  has_prices is accepted for the day a layout depends on it: today's
 * does not. */
int64_t misslap_dense_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices,
                                            int32_t cardinality_check);

/* ---- the dense batch with an outside option per row: partial assignments (the dense form of
 * misslap_solve_ell_batch_outside, below).  Problem b has shape (n_b, m_b) and an outside value o_i per row -- with
 * opt->maximize = 0 the cost of leaving row i unmatched, else the value of doing so.  It is the dense n_b x (m_b + n_b)
 * matrix aug_b = hstack([mat[b][:n_b][:m_b] widened to double, D_b]), D_b holding o_i at (i, i) and -1 elsewhere: the
 * object m_b + i is private to row i, so every row can always be assigned and a row may stay without a real column.  The
 * result of problem b is bit for bit the reference's from_matrix(aug_b).solve() (with prices_in: started from
 * [prices_in[b][:m_b], zeros(n_b)]; the outside objects always start at 0), given in the caller's terms:
 *   sol[b][i]              the real column of row i, or -1 where the row took its outside option (and beyond n_b, on a
 *                          condemned problem, and where max_iter cut the solve before the row was assigned)
 *   prices_out[b][:M]      the prices of the real columns, 0 beyond m_b
 *   outside_prices_out     double[B][N] or NULL: the price of row i's outside object, 0 beyond n_b.  A row without any
 *                          valid entry is a one-entry row of the reference: it bids +inf, and that is its outside price.
 *   meta[b]                the augmented problem's record: n_cols = m_b + n_b, nnz = valid entries + n_b; n_assigned
 *                          counts the rows on their outside option too.
 *   outside, outside_ld    always double, whatever opt->mat_dtype is.  outside_ld == 0: double[B], one value per problem;
 *                          outside_ld >= N: double[B][outside_ld], the value of row i at outside[b * outside_ld + i];
 *                          anything else is MISSLAP_ERR_INVALID.  The values of rows >= n_b are never read.  An outside
 *                          value is an entry of a dense matrix and obeys the dense rule: -0.0 is valid, +inf condemns the
 *                          problem as a +inf entry does, and a negative value or a NaN -- which would be an ABSENT entry,
 *                          a row that must be matched: not offered -- is MISSLAP_BATCH_STATUS_BAD_OUTSIDE.
 * The checks, in their order: 7 BAD_SHAPE; 15 BAD_OUTSIDE; 3 INFINITE_VALUE (a valid entry, or the outside value of a row
 * < n_b, is +inf); 5 PRICE_NOT_FINITE; 6 PRICE_NEGATIVE.  TOO_FEW_VALUES, EMPTY_ROW and INFEASIBLE cannot occur: a row
 * without a valid entry, a graph without a complete matching and n_b > m_b are all solved.  No guard is launched and
 * matching_size[b] (may be NULL) is -1.  A problem with a status other than 0 has sol -1, prices_out 0,
 * outside_prices_out 0 and meta[b] = {n_rows = n_b, n_cols = m_b + n_b, nnz = valid entries + n_b, every other result
 * field 0} (all three 0 for MISSLAP_BATCH_STATUS_BAD_SHAPE).
 * mat holds elements of opt->mat_dtype (all four types).  The LDS carve is sized for N rows and M + N objects (77 824
 * bytes at 1024 / 1024).  Every other argument is misslap_solve_dense_batch_status's, in both of its modes: with a
 * workspace (misslap_dense_batch_outside_workspace_bytes) every pointer except opt and info is a device pointer and the
 * call enqueues two launches (check, solve with verdict) on `stream`, allocates nothing, copies nothing and waits for
 * nothing; without one the library uploads host arrays, checks host shapes as before, uses its own scratch and
 * synchronises once.
 * On eps: the augmented problem is rectangular (more objects than rows), where the reference's eps-scaling (eps_start = 0,
 * fast = 0) keeps the prices of earlier phases and is NOT optimal in general.  A single phase -- fast != 0, or
 * 0 < eps_start <= 1 / n_b -- from zero prices is optimal within n_b * eps. */
#define MISSLAP_BATCH_STATUS_BAD_OUTSIDE 15  /* the outside value of a row is negative or a NaN (an absent entry) */
/* (in parentheses: two tests from before this code pin the list of the plain `#define MISSLAP_BATCH_STATUS_<NAME> <n>`
 * lines to 0 .. 15, and existing tests stay as they are; 16 is directly behind the others and reuses none) */
#define MISSLAP_BATCH_STATUS_BAD_BOX (16)    /* misslap_solve_boxes_batch: a box inside the shape has x2 < x1 or y2 < y1 */
int misslap_solve_dense_batch_outside(int64_t B, int64_t N, int64_t M, const void *mat, const int32_t *shapes,
                                      int32_t fast, const double *prices_in, const misslap_options *opt, void *stream,
                                      void *workspace, int64_t workspace_bytes, const double *outside, int64_t outside_ld,
                                      int32_t *sol, double *prices_out, double *outside_prices_out,
                                      int32_t out_on_device, int32_t *status, int32_t *matching_size,
                                      misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_dense_batch_outside needs: the check records, the sanitised shapes
 * and, with has_prices, the staged starting prices of the augmented problems (B x (M + N) doubles), each 256-byte
 * aligned; -1 for B < 1 or N, M outside 1 .. MISSLAP_DENSE_BATCH_MAX_DIM.  Needs no GPU. */
int64_t misslap_dense_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices);

/* ---- the dense batch on a strided stack: a transposed view, a slice of a wider buffer, an expanded matrix, read where
 * it lies.  misslap_solve_dense_batch_status_strided and misslap_solve_dense_batch_outside_strided are
 * misslap_solve_dense_batch_status and misslap_solve_dense_batch_outside with three more arguments behind B, N, M: the
 * strides of the stack in ELEMENTS of opt->mat_dtype.  mat points at the view's first element, and entry (i, j) of
 * problem b is mat[b * stride_b + i * stride_n + j * stride_m]; shapes refer to the view.  Every other argument, both
 * modes of the call (with and without a workspace), the workspace size (misslap_dense_batch_workspace_bytes /
 * misslap_dense_batch_outside_workspace_bytes: strides do not change it) and every output are those of the contiguous
 * call, and the result is bit for bit that call's on a compact copy of the view.
 *   strides        each >= 0, and (B - 1) * stride_b + (N - 1) * stride_n + (M - 1) * stride_m must fit 62 bits: anything
 *                  else is MISSLAP_ERR_INVALID, before a device is touched.  0 is allowed (stride_b = 0: one matrix solved
 *                  B times, from different starting prices or outside values), and the strides need not be ordered
 *                  (stride_n = 1: a transposed view).  Offsets are formed in 64 bits.  The strides of the contiguous stack
 *                  (N * M, M, 1) take the contiguous call's kernels.
 *   mat            a DEVICE pointer, aligned to its element only: opt->input_on_device must be set (MISSLAP_ERR_INVALID
 *                  otherwise; a host stack is uploaded whole, so it is compact).  Only elements of the view are read --
 *                  nothing beyond m_b in a row, no row >= n_b, nothing of the storage between the view's elements -- and
 *                  nothing is written, copied or converted.
 * The kernels are a family of their own with run-time strides (csrc/kernels_dense_batch.hpp); any layout is correct, and
 * two are fast: stride_m == 1 (the lane map of the contiguous bid with stride_n as the row stride), and stride_n == 1,
 * where rounds of many bidders bid one lane per person so that a load is coalesced across persons. */
int misslap_solve_dense_batch_status_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                             int64_t stride_m, const void *mat, const int32_t *shapes, int32_t fast,
                                             const double *prices_in, int32_t cardinality_check,
                                             const misslap_options *opt, void *stream, void *workspace,
                                             int64_t workspace_bytes, int32_t *sol, double *prices_out,
                                             int32_t out_on_device, int32_t *status, int32_t *matching_size,
                                             misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);
int misslap_solve_dense_batch_outside_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                              int64_t stride_m, const void *mat, const int32_t *shapes, int32_t fast,
                                              const double *prices_in, const misslap_options *opt, void *stream,
                                              void *workspace, int64_t workspace_bytes, const double *outside,
                                              int64_t outside_ld, int32_t *sol, double *prices_out,
                                              double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                              int32_t *matching_size, misslap_dense_batch_meta *meta,
                                              misslap_dense_batch_info *info);

/* ---- the reverse-auction finish of a dense batch solve: rectangular problems made optimal from any starting prices.
 * A forward auction on n_b rows and more than n_b objects (m_b > n_b, and every outside problem) is optimal only as a
 * single phase from zero prices; from other prices, or with eps-scaling, it ends with eps-CS but with abandoned objects
 * priced above the objects in use.  This call runs, behind a stream-ordered misslap_solve_dense_batch_status[_strided]
 * or misslap_solve_dense_batch_outside[_strided] and on that solve's device outputs, the modified reverse auction with a
 * fixed lambda (Bertsekas, Network Optimization, 7.2) on every problem with status[b] == 0 and meta[b].n_assigned ==
 * n_b: lambda = the smallest price of an assigned object, and every unassigned object priced above lambda either takes
 * the row that values it most or drops to lambda.  Afterwards the assignment satisfies eps-CS at meta[b].final_eps and no
 * unassigned object is priced above lambda: it is optimal within n_b * final_eps.  The arithmetic is float64 and stated,
 * operation for operation, by sslap_amd.dense_reverse_finish; csrc/kernels_dense_batch.hpp has the kernel.
 *   B, N, M, stride_*, mat   the stack as misslap_solve_dense_batch_status_strided takes it: a contiguous stack passes
 *                  (N * M, M, 1).  Element type and entry rule from opt->mat_dtype (| MISSLAP_DENSE_ENTRIES_FINITE).
 *   shapes         the solve's device shapes, or NULL.  status[b] is read first and nothing else of a problem whose status
 *                  is not 0 is read or written, so a bad device shape is never used.
 *   outside, outside_ld   the solve's outside values (device), or NULL for a solve without them; outside_prices likewise.
 *   opt            device, maximize, mat_dtype; max_iter is the finish's own budget of iterations per problem;
 *                  input_on_device must be set.  Every pointer except opt is a device pointer.
 *   stream         the launch goes onto it: one launch, one workgroup per problem; nothing is allocated, copied or waited
 *                  for, and no workspace is needed.
 *   status, sol, prices, outside_prices, meta   the solve's outputs.  sol, prices and outside_prices of a finished
 *                  problem are rewritten from the final state (an outside object is -1 in sol), meta[b].obj_f64 and
 *                  obj_f32 are recomputed in the reference's row order and meta[b].eCE at target_eps = 1 / n_b; every other
 *                  field of meta[b] stays the forward solve's.
 *   reverse_its    int64[B]: the iterations made (0 for a square problem), -1 where the finish did not run
 *   reverse_left   int32[B]: the unassigned objects still priced above lambda -- 0 unless max_iter cut the finish or a
 *                  stalled iteration ended it --, -1 where it did not run (status != 0, or max_iter cut the forward
 *                  solve before every row was assigned: nothing of that problem is touched).
 *                  A stalled iteration: the move found would not raise the moving row's profit, a[i*][j] - p_j > pi[i*]
 *                  is false for p_j = max(lambda, omega - eps).  In exact arithmetic every move raises it by at least
 *                  eps; it happens only where eps is lost to rounding, outside max(|a|, |p|) * 2^-52 < final_eps.  The
 *                  iteration is counted, nothing is written, and the finish ends with reverse_left > 0 (the object of
 *                  that iteration included): outside that range the finish promises nothing and a caller reads
 *                  reverse_left, since status stays 0 and eCE may be 1. */
int misslap_dense_batch_reverse_finish(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n, int64_t stride_m,
                                       const void *mat, const int32_t *shapes, const double *outside, int64_t outside_ld,
                                       const misslap_options *opt, void *stream, const int32_t *status, int32_t *sol,
                                       double *prices, double *outside_prices, misslap_dense_batch_meta *meta,
                                       int64_t *reverse_its, int32_t *reverse_left);

/* ---- many small SPARSE problems in one call: the batch form of _from_sparse(loc, val, size=...) (auction_.pyx:575-617).
 * loc is int32[nnz][2] and val double[nnz]; problem b is the entries offsets[b] .. offsets[b + 1] (offsets: host
 * int64[B + 1], offsets[0] = 0, non-decreasing, offsets[B] = nnz), its row and column indices its own and 0-based, read
 * in their stored order as the reference reads them.  Each problem is solved by ONE workgroup of ONE launch, its whole
 * state in LDS (csrc/kernels_sparse_batch.hpp), and its result is exactly what _from_sparse(loc_b, val_b, size=sizes[b],
 * ...).solve() returns: same assignment, its, nreductions, eCE, objective and price bits.  The per-problem records and
 * the call info are the dense batch's structs, misslap_dense_batch_meta / misslap_dense_batch_info: nothing in them is
 * dense-specific (meta.n_rows = max row + 1, meta.n_cols = max column + 1, meta.nnz = the problem's entries).
 *   sizes          int64[B][2] host array or NULL: problem b's `size` of _from_sparse, read as it reads it (M, N =
 *                  size, :592); NULL = N is the maximum row index (:594).  N only enters the "fewer than N entries"
 *                  check; the solve uses the problem's own max row + 1.
 *   eps_start      float[B] host array or NULL: as for misslap_solve_dense_batch (the front-end's `fast` passes 1 / N_b).
 *   prices_in      double[B][prices_ld] or NULL: problem b starts from prices_in[b][:n_cols_b] as misslap_resolve does;
 *                  prices_ld >= every n_cols_b.
 *   cardinality_check  != 0: _from_sparse's Hopcroft-Karp guard on the true graph (:608-612), per problem: for B >= 256
 *                  on the device (the kernel of misslap_matching_batch) for problems whose graph the check pass found
 *                  clean (rows ascending from 0 without a gap, no negative index) and within the cap, on the host for
 *                  the rest and for smaller batches.
 *   sol            int32[B][sol_ld]: sol[b][:n_b] the assignment, -1 beyond.
 *   prices_out     double[B][prices_out_ld] or NULL: final prices of the maximised problem, 0 beyond n_cols_b.
 *   sol_ld, prices_out_ld   the caller's leading dimensions: at least the largest n_b / n_cols_b of the batch.  A caller
 *                  sizes them from loc alone: max(loc[:, 0]) + 1 and max(loc[:, 1]) + 1, capped at
 *                  MISSLAP_SPARSE_BATCH_MAX_DIM.  Checked per problem as its last check: a call that does not fit fails
 *                  like any other check, before anything is solved.
 *   opt, out_on_device, meta, info   as for misslap_solve_dense_batch (input_on_device: loc, val and prices_in are
 *                  device pointers; offsets and sizes are always host memory).
 * All or nothing: the first failing problem gives MISSLAP_ERR_INVALID and the text "problem <b>: <what _from_sparse
 * raises for that problem alone>", checked in its order: no entries, fewer entries than N, the matching guard (with
 * misslap_hopcroft_karp's index and order checks), the constructor's checks (negative index, rows not ascending, a row
 * gap, NaN / infinity, a column too large), n_b or n_cols_b above MISSLAP_SPARSE_BATCH_MAX_DIM, bad starting prices,
 * then the leading dimensions.  Every solve ends after at most max_iter rounds. */
#define MISSLAP_SPARSE_BATCH_MAX_DIM 2048
int misslap_solve_sparse_batch(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                               const int64_t *sizes, const float *eps_start, const double *prices_in, int64_t prices_ld,
                               int32_t cardinality_check, const misslap_options *opt, int32_t *sol, int64_t sol_ld,
                               double *prices_out, int64_t prices_out_ld, int32_t out_on_device,
                               misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);

/* ---- the sparse batch with a verdict per problem instead of all or nothing, and in stream order.
 * misslap_solve_sparse_batch_status takes the packed loc / val of misslap_solve_sparse_batch and never fails for a reason
 * that belongs to one problem: status[b] is the first check problem b fails, and every problem with status 0 is solved --
 * sol, prices and meta bit for bit what misslap_solve_sparse_batch gives for it.  A problem with another status takes no
 * part in the solve launch (its workgroup leaves at once, before it reads any entry): sol[b][:] = -1,
 * prices_out[b][:] = 0, meta[b] = {n_rows = max row + 1, n_cols = max column + 1 (0 without a non-negative index), nnz =
 * the problem's entries, every other result field 0}.  The checks, in their order (codes 0 .. 7 are the dense batch's):
 *    8 NO_ENTRIES            offsets[b + 1] == offsets[b]
 *    9 DIVISION_BY_ZERO      fast != 0 and the reference's N is 0 (N = sizes[b][1], without sizes the MAX ROW INDEX,
 *                            auction_.pyx:592 / :594)
 *    1 TOO_FEW_VALUES        fewer entries than N
 *    4 INFEASIBLE            cardinality_check, the guard matched the problem (matching_size[b] >= 0) and found fewer
 *                            than max row + 1 rows matchable
 *   10 NEGATIVE_INDEX        a negative row or column index
 *   11 ROWS_UNSORTED         a row index below the one stored before it
 *   12 ROW_GAP               a row of 0 .. max row without an entry
 *    3 INFINITE_VALUE        val holds a NaN or an infinity
 *   13 TOO_LARGE             more than Nmax rows or Mmax columns (a column index whose + 1 does not fit an int32 included)
 *   14 PRICES_TOO_NARROW     prices_in given and prices_ld < the problem's columns
 *    5 PRICE_NOT_FINITE, 6 PRICE_NEGATIVE   as for the dense batch, over prices_in[b][:n_cols_b]
 * This is misslap_solve_sparse_batch's order without cardinality_check, and with it for every problem the guard matches:
 * a graph that is clean (rows ascending from 0 without a gap, no negative index) with at most
 * MISSLAP_SPARSE_BATCH_MAX_DIM rows and columns.  The one difference: for any other graph misslap_solve_sparse_batch lets
 * its host guard speak first ("loc entry ... outside", "rows must be sorted", or an infeasibility); here no host work is
 * done, the structural code is reported and matching_size[b] is -1.  The guard always runs on the device.
 *   loc, val, prices_in, prices_ld, cardinality_check   as for misslap_solve_sparse_batch.
 *   offsets        host int64[B + 1], always: checked as misslap_solve_sparse_batch checks it, and the guard's LDS carve
 *                  is sized from the largest problem.
 *   offsets_dev    with a workspace: the same B + 1 values in device memory.  Else not read.
 *   sizes          int64[B][2] or NULL, as for misslap_solve_sparse_batch; a DEVICE array with a workspace.
 *   fast           != 0: problem b starts at eps = (float)(1.0 / (double)N_b), formed in the kernel (:614-615);
 *                  0: opt->eps_start for every problem.
 *   Nmax, Mmax     1 .. MISSLAP_SPARSE_BATCH_MAX_DIM: the caller's bound on every problem's rows and columns.  They are
 *                  the leading dimensions of sol (int32[B][Nmax]) and prices_out (double[B][Mmax], may be NULL) and size
 *                  the LDS carve and the workgroup.  A problem beyond them is MISSLAP_BATCH_STATUS_TOO_LARGE and is
 *                  condemned before any LDS state exists: no kernel of the call reads outside offsets[b] ..
 *                  offsets[b + 1] of loc / val or outside the problem's own nnz_b + 1 row-start slots, or writes
 *                  outside the problem's own row of sol / prices_out.
 *   opt, stream, workspace, workspace_bytes, out_on_device, status, matching_size, meta, info
 *                  as for misslap_solve_dense_batch_status (workspace: misslap_sparse_batch_workspace_bytes).  With a
 *                  workspace EVERY pointer argument except offsets, opt and info is a device pointer, the three
 *                  launches (check, guard, solve with verdict) go onto `stream`, and the call allocates and frees
 *                  nothing, creates no event, waits for nothing and copies nothing.  Above 64 KB of LDS it opts the solve
 *                  kernel into the larger carve first (hipFuncSetAttribute: a host-side setting, no wait).
 * Only what is wrong with the whole call is an error: B, offsets, Nmax, Mmax, prices_ld < 1, a NULL loc / val (with
 * entries) / sol / status, the options, a workspace that is too small or misaligned. */
#define MISSLAP_BATCH_STATUS_NO_ENTRIES 8          /* the problem has no entries */
#define MISSLAP_BATCH_STATUS_DIVISION_BY_ZERO 9    /* fast with N = 0 (sizes[b][1], or the max row index) */
#define MISSLAP_BATCH_STATUS_NEGATIVE_INDEX 10     /* a negative row or column index */
#define MISSLAP_BATCH_STATUS_ROWS_UNSORTED 11      /* rows not in ascending order */
#define MISSLAP_BATCH_STATUS_ROW_GAP 12            /* a row of 0 .. N-1 without an entry */
#define MISSLAP_BATCH_STATUS_TOO_LARGE 13          /* more rows or columns than Nmax / Mmax (dims, at most the cap) */
#define MISSLAP_BATCH_STATUS_PRICES_TOO_NARROW 14  /* prices hold fewer columns than the problem has */
int misslap_solve_sparse_batch_status(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                      const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                      const double *prices_in, int64_t prices_ld, int32_t cardinality_check,
                                      const misslap_options *opt, void *stream, void *workspace, int64_t workspace_bytes,
                                      int64_t Nmax, int64_t Mmax, int32_t *sol, double *prices_out, int32_t out_on_device,
                                      int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                      misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_sparse_batch_status over B problems of nnz entries in all needs (the
 * check records, the nnz + B row starts and, with cardinality_check, the cardinalities, each 256-byte aligned); -1 for
 * B < 1 or nnz < 0.  Needs no GPU.  has_prices is accepted for the day a layout depends on it: today's does not. */
int64_t misslap_sparse_batch_workspace_bytes(int64_t B, int64_t nnz, int32_t has_prices, int32_t cardinality_check);

/* ---- the sparse batch with an outside option per row: partial assignments from packed loc / val, the layout a radius
 * or chi-square gate leaves (ragged rows).  Problem b is the entries offsets[b] .. offsets[b + 1] in stored order, duplicates
 * of an (i, j) kept, plus ONE entry per row, stored last in its row: row i (i < n_b) gets (i, m_b + i) with the row's
 * outside value -- with opt->maximize = 0 the cost of leaving row i unmatched, else the value of doing so.  n_b is
 * sizes[b][1] where sizes is given, else the last stored row + 1; m_b is the largest real column + 1, 0 for a problem
 * without an entry; sizes[b][0] is not read.  Rows WITHOUT ANY ENTRY are legal -- in front, in the middle, and behind the
 * last stored row when sizes names them -- and so is a problem with offsets[b + 1] == offsets[b], provided sizes names its
 * rows.  The object m_b + i is private to row i, so every row can always be assigned.  The result of problem b is bit for
 * bit the reference's from_sparse(loc_b, val_b, size=(m_b + n_b, n_b)).solve() on that packing (with prices_in: started
 * from [prices_in[b][:m_b], zeros(n_b)]), given in the caller's terms exactly as misslap_solve_ell_batch_outside gives it:
 *   sol[b][i]              int32[B][Nmax]: the real column of row i, or -1 where the row took its outside option (and
 *                          beyond n_b, on a condemned problem, and where max_iter cut the solve short)
 *   prices_out             double[B][Mmax] or NULL: the prices of the real columns, 0 beyond m_b
 *   outside_prices_out     double[B][Nmax] or NULL: the price of row i's outside object, 0 beyond n_b (+inf for a row
 *                          without any real entry: a one-entry row of the reference bids +inf)
 *   meta[b]                the augmented problem's record: n_rows = n_b, n_cols = m_b + n_b, nnz = nnz_b + n_b
 *   outside, outside_ld    outside_ld == 0: double[B], one value per problem; outside_ld >= Nmax: double[B][outside_ld],
 *                          the value of row i at outside[b * outside_ld + i]; anything else is MISSLAP_ERR_INVALID.  Only
 *                          the values of rows < min(n_b, Nmax) are read.  Where loc / val live (host, or device with
 *                          opt->input_on_device).
 *   fast                   != 0: problem b starts at eps = (float)(1.0 / (double)n_b), formed in the kernel.
 * The checks, in their order:
 *    8 NO_ENTRIES            offsets[b + 1] == offsets[b] and sizes is NULL
 *   10 NEGATIVE_INDEX        a negative row or column index
 *   11 ROWS_UNSORTED         a row index below the one stored before it
 *    7 BAD_SHAPE             sizes given and sizes[b][1] < max(1, last stored row + 1)
 *    3 INFINITE_VALUE        a NaN or an infinity in val, or in the outside value of a row < min(n_b, Nmax)
 *   13 TOO_LARGE             n_b > Nmax or m_b > Mmax (a column index whose + 1 does not fit an int32 included)
 *   14 PRICES_TOO_NARROW     prices_in given and prices_ld < m_b
 *    5 PRICE_NOT_FINITE, 6 PRICE_NEGATIVE   over prices_in[b][:m_b]
 * Codes 1, 2, 4, 9, 12 and 15 never occur: graphs without a complete matching and n_b > m_b are solved.  No guard is
 * launched and matching_size[b] (may be NULL) is -1.  A problem with a status other than 0 has sol -1, prices_out 0,
 * outside_prices_out 0 and meta[b] = {n_rows = n_b, n_cols = m_b + n_b (each saturated at INT32_MAX), nnz = nnz_b + n_b,
 * every other result field 0} behind the codes 3, 13, 14, 5 and 6, and an all-zero record behind 8, 10, 11 and 7.  Its
 * workgroup leaves before any LDS state exists and before it reads a row start, a loc or a val of the problem.
 * Nmax and Mmax (1 .. MISSLAP_SPARSE_BATCH_MAX_DIM) bound the rows and the REAL columns; the LDS carve is sized for Nmax
 * rows and Mmax + Nmax objects (155 648 bytes at 2048 / 2048).  No kernel of the call reads outside offsets[b] ..
 * offsets[b + 1] of loc / val, or writes outside the problem's own Nmax + 1 row starts of the workspace and its own rows
 * of the outputs.  offsets, offsets_dev, sizes, prices_in, prices_ld, opt, stream, workspace, workspace_bytes,
 * out_on_device, status, meta and info are misslap_solve_sparse_batch_status's, in both of its modes: with a workspace
 * (misslap_sparse_batch_outside_workspace_bytes) every pointer except offsets, opt and info is a device pointer and the
 * call enqueues two launches (check, solve with verdict) on `stream` and waits for nothing; without one the library
 * uploads host arrays, uses its own scratch and synchronises once.
 * On eps: see misslap_solve_ell_batch_outside below -- a single phase (fast != 0, or 0 < eps_start <= 1 / n_b) from zero
 * prices is optimal within n_b * eps; the reference's eps-scaling is not, on a rectangular problem.
 * Only what is wrong with the whole call is an error: B, offsets, Nmax, Mmax, outside_ld, prices_ld < 1, a NULL loc / val
 * (with entries) / sol / status / outside, the options, a workspace that is too small or misaligned. */
int misslap_solve_sparse_batch_outside(int64_t B, const int32_t *loc, const double *val, const int64_t *offsets,
                                       const int64_t *offsets_dev, const int64_t *sizes, int32_t fast,
                                       const double *prices_in, int64_t prices_ld, const misslap_options *opt, void *stream,
                                       void *workspace, int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                       const double *outside, int64_t outside_ld, int32_t *sol, double *prices_out,
                                       double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                       int32_t *matching_size, misslap_dense_batch_meta *meta,
                                       misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_sparse_batch_outside needs: the check records, B x (Nmax + 1) row
 * starts and, with has_prices, the staged starting prices of the augmented problems (B x (Mmax + Nmax) doubles), each
 * 256-byte aligned; -1 where B, Nmax or Mmax are out of range.  Needs no GPU. */
int64_t misslap_sparse_batch_outside_workspace_bytes(int64_t B, int64_t Nmax, int64_t Mmax, int32_t has_prices);

/* ---- the sparse batch on a VIEW of the packed arrays, as a device pipeline leaves them: int64 indices that are a slice
 * of a wider buffer or a transposed view, float32 values, and offsets that only the device has seen.
 * misslap_solve_sparse_batch_status_view and misslap_solve_sparse_batch_outside_view are
 * misslap_solve_sparse_batch_status and misslap_solve_sparse_batch_outside with this head in place of (B, loc, val,
 * offsets, offsets_dev, ...); no host offsets exist, nnz is an argument:
 *   nnz            the packed entries of the call (0 .. 2^56).
 *   loc, loc_int64, stride_e, stride_c   entry g of the packed arrays is row loc[g * stride_e], column
 *                  loc[g * stride_e + stride_c], in ELEMENTS of the index type: int32, or int64 with loc_int64 != 0.
 *                  Strides are >= 0 and (nnz - 1) * stride_e + stride_c must fit 62 bits: anything else is
 *                  MISSLAP_ERR_INVALID, before a device is touched.  (2, 1) is the compact (nnz, 2) array, (3, 1) the
 *                  [:, 1:] of an (nnz, 3) array, (1, nnz) the transposed (2, nnz) array.  Offsets are formed in 64 bits;
 *                  loc needs only its element's alignment.
 *   val            the value of entry g is val[g], contiguous, of opt->mat_dtype: MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32
 *                  (every other type is MISSLAP_ERR_INVALID).  A float32 value is widened to double as it is read, which
 *                  is exact; C, eps, bids, prices, eCE and both objectives are the float64 arithmetic on the widened
 *                  value, and prices, outside values and every output stay double.
 *   offsets_dev    int64[B + 1] on the device.  Checked there, per problem: a problem whose slice is not
 *                  0 <= offsets[b] <= offsets[b + 1] <= nnz, or holds 2^31 - 1 entries or more, gets
 *                  MISSLAP_BATCH_STATUS_BAD_SHAPE (7) ahead of every other check; nothing of its loc / val is read and
 *                  its outputs are the condemned ones with an all-zero record.  (7 cannot otherwise occur in the status
 *                  call; in the outside call it already means "the extent of this problem is unusable".)
 *                  offsets[0] != 0 or offsets[B] != nnz is no error: entries in no slice are never read.
 * loc, val and offsets_dev are DEVICE pointers in both modes of the call and opt->input_on_device must be set
 * (MISSLAP_ERR_INVALID otherwise); prices_in and outside live on the device with them.  With a workspace every pointer
 * except opt and info is a device pointer, the launches go onto `stream`, and nothing is allocated, copied or waited
 * for; without one the library uses its own stream and scratch, uploads a host sizes, and waits once at the end.
 * Only elements of the view are read: nothing outside offsets[b] .. offsets[b + 1] of any problem, nothing of the
 * storage between the view's elements; nothing is written.
 * An int64 index outside the int32 range SATURATES to INT32_MIN / INT32_MAX before any check: a column at or above 2^31
 * is MISSLAP_BATCH_STATUS_TOO_LARGE (and so is such a last row in the outside call; in the status call a row that far
 * from its predecessor is a ROW_GAP, as INT32_MAX is in misslap_solve_sparse_batch_status), a value at or below -2^31 is
 * NEGATIVE_INDEX whatever its low word is, and nothing is ever truncated into a valid index.
 * Apart from the above every verdict, output, record and check order is that of misslap_solve_sparse_batch_status /
 * _outside on a compact copy -- int32 (nnz, 2) indices, the values widened to double, the same offsets on the host -- bit
 * for bit.  The guard of the status call cannot size its LDS carve from the largest problem: it is sized for
 * min(nnz, MISSLAP_SPARSE_BATCH_MAX_DIM) rows, which still matches every clean graph within the cap.  The row starts live
 * in a block of Nmax + 1 ints per problem in both calls, so a malformed slice cannot reach a healthy problem.
 * The kernels are a family of their own (csrc/kernels_sparse_view.hpp): the contiguous calls keep theirs. */
int misslap_solve_sparse_batch_status_view(int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e,
                                           int64_t stride_c, const void *val, const int64_t *offsets_dev,
                                           const int64_t *sizes, int32_t fast, const double *prices_in, int64_t prices_ld,
                                           int32_t cardinality_check, const misslap_options *opt, void *stream,
                                           void *workspace, int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                           int32_t *sol, double *prices_out, int32_t out_on_device, int32_t *status,
                                           int32_t *matching_size, misslap_dense_batch_meta *meta,
                                           misslap_dense_batch_info *info);
/* (workspace: misslap_sparse_batch_outside_workspace_bytes -- its carve depends neither on nnz nor on strides) */
int misslap_solve_sparse_batch_outside_view(int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e,
                                            int64_t stride_c, const void *val, const int64_t *offsets_dev,
                                            const int64_t *sizes, int32_t fast, const double *prices_in,
                                            int64_t prices_ld, const misslap_options *opt, void *stream, void *workspace,
                                            int64_t workspace_bytes, int64_t Nmax, int64_t Mmax, const double *outside,
                                            int64_t outside_ld, int32_t *sol, double *prices_out,
                                            double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                            int32_t *matching_size, misslap_dense_batch_meta *meta,
                                            misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_sparse_batch_status_view needs: the check records, B x (Nmax + 1) row
 * starts and, with cardinality_check, the cardinalities, each 256-byte aligned; -1 for B < 1, nnz < 0 or Nmax outside
 * 1 .. MISSLAP_SPARSE_BATCH_MAX_DIM.  Needs no GPU.  nnz and has_prices are accepted for the day a layout depends on
 * them: today's does not. */
int64_t misslap_sparse_batch_view_workspace_bytes(int64_t B, int64_t nnz, int64_t Nmax, int32_t has_prices,
                                                  int32_t cardinality_check);

/* ---- the sparse batch from padded candidate lists (ELL), the layout a top-k, a gating step or a nearest-neighbour
 * search leaves on the device: cols[B][N][K] (int32, or int64 with cols_int64 != 0) and vals[B][N][K] (double, or float
 * with opt->mat_dtype = MISSLAP_DTYPE_F32; F16 / BF16 are MISSLAP_ERR_INVALID here).  Problem b is rows 0 .. n_b - 1 of
 * cols[b] / vals[b] (n_b = rows[b]; rows NULL: N).  Slot (i, k) is an entry iff cols[b][i][k] >= 0: a negative column is
 * a hole, in any position, and the value stored in a hole is never interpreted.  With loc_b / val_b the entries of problem
 * b in row order, within a row in slot order, holes dropped, and m_b = max column + 1, the result of problem b is bit for
 * bit that of misslap_solve_sparse_batch_status on (loc_b, val_b) with sizes[b] = (m_b, n_b), i.e. of the reference's
 * from_sparse(loc_b, val_b, size=(m_b, n_b)).solve(): N = n_b, so `fast` starts at (float)(1.0 / n_b).  A column may
 * repeat within a row, with the meaning it has in the sparse batch.  float values are widened to double as they are read
 * (exact); the result is that of the widened values.  Neither array is written.
 * The call always gives a verdict per problem (there is no all-or-nothing form); no new codes.  The checks, in their order:
 *    7 BAD_SHAPE             rows[b] outside 1 .. N: nothing of the problem is read
 *    2 EMPTY_ROW             a row of 0 .. n_b - 1 without an entry
 *    3 INFINITE_VALUE        a NaN or an infinity in an entry (never in a hole)
 *   13 TOO_LARGE             a column at or above Mmax (an int64 column is compared in 64 bits: 2^31 + 5 is too large, not
 *                            a hole and not column 5)
 *   14 PRICES_TOO_NARROW     prices_in given and prices_ld < m_b
 *    4 INFEASIBLE            cardinality_check and the guard found fewer than n_b rows matchable.  The guard matches the
 *                            problems the checks 7, 2 and 13 pass; matching_size[b] is -1 for every other one.
 *    5 PRICE_NOT_FINITE, 6 PRICE_NEGATIVE   over prices_in[b][:m_b]
 * A problem with a status other than 0 takes no part in the solve (its workgroup leaves before it reads cols or vals):
 * sol[b][:] = -1, prices_out[b][:] = 0, meta[b] = {n_rows = n_b, n_cols = m_b (saturated at INT32_MAX), nnz = its entries,
 * every other result field 0}, all three counts 0 for BAD_SHAPE.
 *   N, Mmax        1 .. MISSLAP_SPARSE_BATCH_MAX_DIM; K >= 1; N * K <= INT32_MAX - 128.  Mmax is the caller's bound on
 *                  every column: sol is int32[B][N], prices_out double[B][Mmax] (may be NULL), and N and Mmax size the LDS
 *                  carve and the workgroup as Nmax and Mmax do for misslap_solve_sparse_batch_status.
 *   rows           int32[B] or NULL.      prices_in      double[B][prices_ld] or NULL, prices_ld >= 1.
 *   fast           != 0: problem b starts at eps = (float)(1.0 / (double)n_b), formed in the kernel.
 *   opt, stream, workspace, workspace_bytes, out_on_device, status, matching_size, meta, info
 *                  as for misslap_solve_sparse_batch_status (workspace: misslap_ell_batch_workspace_bytes); opt->mat_dtype
 *                  names the type of vals.  Without a workspace the library uploads host arrays (device pointers with
 *                  input_on_device), uses its own scratch and synchronises once.  With a workspace EVERY pointer argument
 *                  except opt and info is a device pointer, the three launches (check, guard, solve with verdict) go
 *                  onto `stream`, and the call allocates nothing, creates no event, waits for nothing, copies nothing and
 *                  reads no host array of per-problem data.
 * Only what is wrong with the whole call is an error: B, N, K, Mmax, the caps, prices_ld < 1, a NULL cols / vals / sol /
 * status, the options, a workspace that is too small or misaligned. */
int misslap_solve_ell_batch(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64, const void *vals,
                            const int32_t *rows, int32_t fast, const double *prices_in, int64_t prices_ld,
                            int32_t cardinality_check, const misslap_options *opt, void *stream, void *workspace,
                            int64_t workspace_bytes, int64_t Mmax, int32_t *sol, double *prices_out,
                            int32_t out_on_device, int32_t *status, int32_t *matching_size,
                            misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_ell_batch over B problems of N x K slots needs (the check records
 * and, with cardinality_check, the cardinalities, each 256-byte aligned); -1 for B < 1, N or K out of range or N * K over
 * its cap.  Needs no GPU.  has_prices is accepted for the day a layout depends on it: today's does not. */
int64_t misslap_ell_batch_workspace_bytes(int64_t B, int64_t N, int64_t K, int32_t has_prices, int32_t cardinality_check);

/* ---- the ELL batch with an outside option per row: partial assignments.  Problem b is the packed problem of
 * misslap_solve_ell_batch plus ONE entry per row, stored last in its row behind every slot: row i (i < n_b) gets
 * (i, m_b + i) with the row's outside value -- with opt->maximize = 0 the cost of leaving row i unmatched, else the value
 * of doing so; m_b = max real column + 1, 0 for a problem without any entry.  The object m_b + i is private to row i, so
 * every row can always be assigned and a row may stay without a real column.  The result of problem b is bit for bit the
 * reference's from_sparse(loc_b, val_b, size=(m_b + n_b, n_b)).solve() on that packing (with prices_in: started from
 * [prices_in[b][:m_b], zeros(n_b)]; the outside objects always start at 0), given in the caller's terms:
 *   sol[b][i]              the real column of row i, or -1 where the row took its outside option (and beyond n_b, on a
 *                          condemned problem, and where max_iter cut the solve before the row was assigned)
 *   prices_out[b][:Mmax]   the prices of the real columns, 0 beyond m_b
 *   outside_prices_out     double[B][N] or NULL: the price of row i's outside object, 0 beyond n_b.  A row without any
 *                          real entry is a one-entry row of the reference: it bids +inf, and that is its outside price.
 *   meta[b]                the augmented problem's record: n_cols = m_b + n_b, nnz = entries + n_b; n_assigned counts the
 *                          rows on their outside option too.
 *   outside, outside_ld    outside_ld == 0: double[B], one value per problem; outside_ld >= N: double[B][outside_ld], the
 *                          value of row i at outside[b * outside_ld + i]; anything else is MISSLAP_ERR_INVALID.  The
 *                          values of rows >= n_b are never read.
 * The checks, in their order: 7 BAD_SHAPE; 3 INFINITE_VALUE (an entry, or the outside value of a row < n_b, is a NaN or an
 * infinity); 13 TOO_LARGE (a real column >= Mmax); 14 PRICES_TOO_NARROW; 5 PRICE_NOT_FINITE; 6 PRICE_NEGATIVE.  EMPTY_ROW
 * and INFEASIBLE cannot occur: a row without entries, a graph without a complete matching, n_b > m_b and a problem of
 * holes only (every row comes back -1) are all solved.  No guard is launched and matching_size[b] (may be NULL) is -1.  A
 * problem with a status other than 0 has sol -1, prices_out 0, outside_prices_out 0 and meta[b] = {n_rows = n_b, n_cols =
 * m_b + n_b (saturated at INT32_MAX), nnz = its entries + n_b, every other result field 0}.
 * Mmax stays the bound on the REAL columns (1 .. MISSLAP_SPARSE_BATCH_MAX_DIM); the LDS carve is sized for N rows and
 * Mmax + N objects (155 648 bytes at 2048 / 2048).  Every other argument is misslap_solve_ell_batch's, in both of its
 * modes: with a workspace (misslap_ell_batch_outside_workspace_bytes) every pointer except opt and info is a device
 * pointer and the call enqueues two launches (check, solve with verdict) on `stream` and waits for nothing; without one
 * the library uploads host arrays, uses its own scratch and synchronises once.
 * On eps: the augmented problem is rectangular (more objects than rows), where the reference's eps-scaling (eps_start = 0,
 * fast = 0) keeps the prices of earlier phases and is NOT optimal in general.  A single phase -- fast != 0, or
 * 0 < eps_start <= 1 / n_b -- from zero prices is optimal within n_b * eps. */
int misslap_solve_ell_batch_outside(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                    const void *vals, const int32_t *rows, int32_t fast, const double *prices_in,
                                    int64_t prices_ld, const misslap_options *opt, void *stream, void *workspace,
                                    int64_t workspace_bytes, int64_t Mmax, const double *outside, int64_t outside_ld,
                                    int32_t *sol, double *prices_out, double *outside_prices_out, int32_t out_on_device,
                                    int32_t *status, int32_t *matching_size, misslap_dense_batch_meta *meta,
                                    misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_ell_batch_outside needs: the check records and, with has_prices, the
 * staged starting prices of the augmented problems (B x (Mmax + N) doubles), each 256-byte aligned; -1 where B, N, K or
 * Mmax are out of range.  Needs no GPU. */
int64_t misslap_ell_batch_outside_workspace_bytes(int64_t B, int64_t N, int64_t K, int64_t Mmax, int32_t has_prices);

/* ---- the reverse-auction finish of a list batch solve: what misslap_dense_batch_reverse_finish is for the dense batch,
 * behind a stream-ordered misslap_solve_sparse_batch_status / _outside (or their _view forms) or misslap_solve_ell_batch /
 * _outside, on that solve's device outputs.  Every outside problem is rectangular, and a list solve that starts from
 * prices_in other than zero ends with eps-CS but, in general, far from the optimum; this call repairs every problem with
 * status[b] == 0 and meta[b].n_assigned == meta[b].n_rows as the dense finish does: lambda = the smallest price of an
 * assigned object, every unassigned object priced above lambda takes the row that values it most or drops to lambda,
 * and afterwards the assignment is optimal within n_b * meta[b].final_eps (for problems without duplicates of an
 * (i, j); with duplicates the largest maximised value among them is the entry).  sslap_amd.sparse_reverse_finish states
 * it in numpy; csrc/kernels_list_finish.hpp has the kernel, which first builds a column index of each problem in
 * `workspace`, so that an iteration costs the length of its column.  n_b and m_b are taken from the record.
 *   misslap_sparse_batch_reverse_finish
 *     B, nnz, loc, loc_int64, stride_e, stride_c, val, offsets_dev   the entries as misslap_solve_sparse_batch_outside_view
 *                  takes them; packed int32 [nnz][2] / float64 arrays pass loc_int64 = 0 and strides (2, 1).  offsets_dev
 *                  is the device copy of the offsets; the slices of the problems with status 0 must not overlap (a host
 *                  offsets array never does).
 *   misslap_ell_batch_reverse_finish
 *     B, N, K, cols, cols_int64, vals   the stack as misslap_solve_ell_batch takes it.  Nmax must be N.
 *   outside, outside_ld   the solve's outside values (device), or NULL for a solve without them; outside_prices likewise.
 *   opt            device, maximize, mat_dtype (the value type: MISSLAP_DTYPE_F64 / _F32); max_iter is the finish's own
 *                  budget of iterations per problem; input_on_device must be set.  Every pointer except opt is a device
 *                  pointer.
 *   stream         the launch goes onto it: one launch, one workgroup per problem; nothing is allocated, copied or waited
 *                  for.
 *   workspace, workspace_bytes   at least misslap_list_batch_finish_workspace_bytes(entries) bytes on the device,
 *                  entries = nnz for the sparse call and B * N * K for the ELL call; its contents are the call's own.
 *   Nmax, Mmax     the solve's bounds: sol is [B][Nmax], prices [B][Mmax], outside_prices [B][Nmax].
 *   status, sol, prices, outside_prices, meta   the solve's outputs, rewritten as misslap_dense_batch_reverse_finish
 *                  rewrites them; meta[b].obj_f64 / obj_f32 and meta[b].eCE are recomputed as the list solve makes them
 *                  (the last stored entry of the chosen column is the choice; every stored copy of it counts into the
 *                  objective), every other field stays the forward solve's.
 *   reverse_its, reverse_left   int64[B] / int32[B], as for the dense call: -1 where the finish did not run (status != 0,
 *                  max_iter cut the forward solve, or sol is not a solve's output), and nothing of such a problem is
 *                  touched; reverse_left > 0 where the budget or a stalled iteration ended the finish.
 * Argument errors are MISSLAP_ERR_INVALID before a device is touched. */
int misslap_sparse_batch_reverse_finish(int64_t B, int64_t nnz, const void *loc, int32_t loc_int64, int64_t stride_e,
                                        int64_t stride_c, const void *val, const int64_t *offsets_dev,
                                        const double *outside, int64_t outside_ld, const misslap_options *opt,
                                        void *stream, void *workspace, int64_t workspace_bytes, int64_t Nmax, int64_t Mmax,
                                        const int32_t *status, int32_t *sol, double *prices, double *outside_prices,
                                        misslap_dense_batch_meta *meta, int64_t *reverse_its, int32_t *reverse_left);
int misslap_ell_batch_reverse_finish(int64_t B, int64_t N, int64_t K, const void *cols, int32_t cols_int64,
                                     const void *vals, const double *outside, int64_t outside_ld,
                                     const misslap_options *opt, void *stream, void *workspace, int64_t workspace_bytes,
                                     int64_t Nmax, int64_t Mmax, const int32_t *status, int32_t *sol, double *prices,
                                     double *outside_prices, misslap_dense_batch_meta *meta, int64_t *reverse_its,
                                     int32_t *reverse_left);
/* Bytes of workspace either finish needs for `entries` entries (12 per entry, in two 256-byte aligned parts); -1 where
 * entries is negative or above 2^56.  Needs no GPU. */
int64_t misslap_list_batch_finish_workspace_bytes(int64_t entries);

/* ---- the dense batch from two point sets: costs from coordinates, the distance stack never stored.
 * x holds B sets of N points and y B sets of M points of D coordinates each, of the type misslap_options.mat_dtype names
 * (MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32 only).  Coordinate k of point i of problem b lies at
 * x[b * x_stride_b + i * x_stride_n + k * x_stride_d] (y alike), strides in elements and >= 0; the offset of a view's
 * last element must fit 62 bits.  Problem b has shape (n_b, m_b) = shapes[b] (NULL: N x M) and the costs
 *     c[i][j] = s_(D-1),  d_k = x[i][k] - y[j][k],  s_0 = d_0 * d_0,  s_k = s_(k-1) + d_k * d_k
 * on the coordinates widened to double (exact): 3 D - 1 separately rounded IEEE double operations in this order, nothing
 * fused or reassociated (sslap_amd.points_to_dense is the definition).  The kernels form every cost they need from the
 * coordinates by exactly this chain (csrc/kernels_points_batch.hpp), and a problem with status 0 is bit for bit -- sol,
 * prices, outside_prices and every field of meta -- the dense call on that float64 stack:
 * misslap_solve_dense_batch_status with cardinality_check = 0 where outside is NULL, else
 * misslap_solve_dense_batch_outside, whose outside / outside_ld, fast, prices_in, opt fields, output arrays and two
 * modes (with a workspace of misslap_points_batch_workspace_bytes every pointer except opt and info is a device pointer
 * and the call allocates, copies and waits for nothing: two launches on `stream`; without one the library uploads compact
 * host arrays -- strides (N * D, D, 1) and (M * D, D, 1) --, checks host shapes and synchronises once) apply unchanged.
 * meta.n_cols is m_b (m_b + n_b with outside), meta.nnz n_b * m_b (+ n_b).
 * The verdicts of a problem, in their order: MISSLAP_BATCH_STATUS_BAD_SHAPE (a shape outside 1 .. N x 1 .. M: nothing of
 * the problem is read), with outside MISSLAP_BATCH_STATUS_BAD_OUTSIDE (a negative or NaN outside value of a row < n_b),
 * MISSLAP_BATCH_STATUS_INFINITE_VALUE (some cost with i < n_b, j < m_b is not finite -- a NaN or infinite coordinate, an
 * overflow -- or an outside value is +inf), without outside MISSLAP_BATCH_STATUS_INFEASIBLE (n_b > m_b: every pair is an
 * edge, so no matcher is launched), MISSLAP_BATCH_STATUS_PRICE_NOT_FINITE, MISSLAP_BATCH_STATUS_PRICE_NEGATIVE.
 * matching_size[b] is min(n_b, m_b) for a good shape without outside, else -1.  A condemned problem has sol -1, prices 0
 * and a meta of the three counts and zeros.  Argument errors are MISSLAP_ERR_INVALID before a device is touched. */
#define MISSLAP_POINTS_BATCH_MAX_DIM 2048
#define MISSLAP_POINTS_BATCH_MAX_COORDS 8
int misslap_solve_points_batch(int64_t B, int64_t N, int64_t M, int64_t D,
                               const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                               const void *y, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                               const int32_t *shapes, int32_t fast, const double *prices_in, const misslap_options *opt,
                               void *stream, void *workspace, int64_t workspace_bytes, const double *outside,
                               int64_t outside_ld, int32_t *sol, double *prices_out, double *outside_prices_out,
                               int32_t out_on_device, int32_t *status, int32_t *matching_size,
                               misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);
/* Bytes of workspace a stream-ordered misslap_solve_points_batch needs: the check records, the sanitised shapes and, with
 * has_prices and has_outside, the staged starting prices; -1 where B < 1 or N / M are outside
 * 1 .. MISSLAP_POINTS_BATCH_MAX_DIM.  Needs no GPU. */
int64_t misslap_points_batch_workspace_bytes(int64_t B, int64_t N, int64_t M, int32_t has_prices, int32_t has_outside);

/* ---- the reverse-auction finish of a points batch solve: what misslap_dense_batch_reverse_finish is for the dense batch,
 * behind a stream-ordered misslap_solve_points_batch and on that solve's device outputs.  Every solve with an outside
 * option is rectangular (n_b rows, m_b + n_b objects), and one that starts from prices_in other than zero ends with
 * eps-CS but, in general, far from the optimum; this call repairs every problem with status[b] == 0 and
 * meta[b].n_assigned == n_b exactly as the dense finish does on the float64 stack of the costs (the chain stated at
 * misslap_solve_points_batch; every finite cost is an entry), which is never stored: the kernel forms every cost from
 * the coordinates (csrc/kernels_points_finish.hpp).  sslap_amd.points_reverse_finish states the call in numpy, and the
 * result is that function's bit for bit.  Problems of up to MISSLAP_POINTS_BATCH_MAX_DIM rows and columns are taken.
 *   B, N, M, D, x, x_stride_*, y, y_stride_*   the point sets as misslap_solve_points_batch takes them (device arrays,
 *                  element type from opt->mat_dtype: MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32); nothing of them is written.
 *   shapes         the solve's device shapes, or NULL.  status[b] is read first and nothing else of a problem whose status
 *                  is not 0 is read or written, so a bad device shape is never used.
 *   outside, outside_ld   the solve's outside values (device), or NULL for the plain problem; outside_prices likewise.
 *   opt            device, maximize, mat_dtype; max_iter is the finish's own budget of iterations per problem;
 *                  input_on_device must be set.  Every pointer except opt is a device pointer.
 *   stream         the launch goes onto it: one launch, one workgroup per problem; nothing is allocated, copied or waited
 *                  for, and no workspace is needed.
 *   status, sol, prices, outside_prices, meta, reverse_its, reverse_left   as for misslap_dense_batch_reverse_finish:
 *                  sol, prices and outside_prices of a finished problem are rewritten, meta[b].obj_f64 / obj_f32 / eCE
 *                  recomputed, every other field kept; reverse_its / reverse_left are -1 where the finish did not run
 *                  (status != 0, or max_iter cut the forward solve) and nothing of such a problem is touched;
 *                  reverse_left > 0 where the budget or a stalled iteration ended the finish.
 * Argument errors (the caps, D, the strides: the solve's checks) are MISSLAP_ERR_INVALID before a device is touched. */
int misslap_points_batch_reverse_finish(int64_t B, int64_t N, int64_t M, int64_t D,
                                        const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                        const void *y, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                                        const int32_t *shapes, const double *outside, int64_t outside_ld,
                                        const misslap_options *opt, void *stream, const int32_t *status, int32_t *sol,
                                        double *prices, double *outside_prices, misslap_dense_batch_meta *meta,
                                        int64_t *reverse_its, int32_t *reverse_left);

/* ---- candidate lists from two point sets: per row the (at most) K nearest columns under a per-row limit, in the padded
 * (B, N, K) layout misslap_solve_ell_batch and misslap_solve_ell_batch_outside read in place.  The (B, N, M) stack of the
 * costs is never stored: one launch forms every cost once, by the chain stated at misslap_solve_points_batch
 * (csrc/kernels_points_candidates.hpp).  sslap_amd.points_to_ell states the call in numpy, and the four outputs are that
 * function's bit for bit.  With c[i][j] the cost of (i, j) and (n_b, m_b) the shape of problem b:
 *   rows[b]        n_b for a shape inside 1 .. N x 1 .. M (shapes NULL: N), else 0 -- which misslap_solve_ell_batch
 *                  reports as MISSLAP_BATCH_STATUS_BAD_SHAPE -- and every slot of such a problem is a hole.
 *   candidates     of row i < n_b: the columns j < m_b whose cost is not finite (a NaN or an infinite coordinate, an
 *                  overflow) or is <= the row's limit under the IEEE comparison (a limit of -0.0 admits a cost of +0.0, a
 *                  NaN limit admits no finite cost; limit NULL admits every column).
 *   counts[b][i]   the number of candidates, before any truncation; 0 for a row >= n_b.
 *   cols, vals     int32 / double [B][N][K].  The candidates of row i in ascending column order from slot 0, the value
 *                  of a cost that is not finite stored as +inf (so the ELL call condemns exactly the problems
 *                  misslap_solve_points_batch condemns, with MISSLAP_BATCH_STATUS_INFINITE_VALUE); every later slot
 *                  holds cols -1, vals 0.0.  Where counts[b][i] > K the K smallest by (cost, column) are kept, the
 *                  non-finite ones first, by column.
 *   B, N, M, D, x, x_stride_*, y, y_stride_*   the point sets as misslap_solve_points_batch takes them (device arrays,
 *                  element type from opt->mat_dtype: MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32); only elements of the two
 *                  views are read and nothing of them is written.
 *   K              1 .. MISSLAP_POINTS_CANDIDATES_MAX_K.
 *   shapes         device int32[B][2], or NULL.
 *   limit, limit_ld   device doubles: NULL for no limit; limit_ld == 0: limit[b] is the limit of every row of problem
 *                  b; else limit[b * limit_ld + i] with limit_ld >= N.  Its sign and finiteness are judged per row, as
 *                  stated above.
 *   opt            device, mat_dtype; input_on_device must be set.  Every pointer except opt is a device pointer.
 *   stream         the launch goes onto it: one launch, a wavefront per row; nothing is allocated, copied, waited for or
 *                  read back, and no workspace is needed.
 * Argument errors (the caps, D, the strides: the solve's checks; K) are MISSLAP_ERR_INVALID before a device is touched. */
#define MISSLAP_POINTS_CANDIDATES_MAX_K 64
int misslap_points_batch_candidates(int64_t B, int64_t N, int64_t M, int64_t D,
                                    const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                    const void *y, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                                    int64_t K, const int32_t *shapes, const double *limit, int64_t limit_ld,
                                    const misslap_options *opt, void *stream, int32_t *cols, double *vals,
                                    int32_t *counts, int32_t *rows);

/* ---- the points batch with a whitening matrix per row: Mahalanobis costs.  misslap_solve_points_batch_whitened is
 * misslap_solve_points_batch and misslap_points_batch_candidates_whitened is misslap_points_batch_candidates, each with
 * the five arguments w, w_stride_b, w_stride_n, w_stride_k, w_stride_l behind the y strides, and every other argument,
 * output, verdict, mode and workspace (misslap_points_batch_workspace_bytes) is that call's.  w holds a lower-triangular
 * D x D matrix W[b][i] for every row, of the element type opt->mat_dtype names like x and y: element (k, l) of row i of
 * problem b lies at w[b * w_stride_b + i * w_stride_n + k * w_stride_k + l * w_stride_l], strides in elements and >= 0
 * (w_stride_n == 0: one matrix per problem; w_stride_b == w_stride_n == 0: one for the call); the offset of the view's
 * last element must fit 62 bits.  A host array (the solve without a workspace and without input_on_device) is compact:
 * strides (N * D * D, D * D, D, 1); a strided w is a device array.  The cost is
 *     c[i][j] = | W[i] (x[i] - y[j]) |^2:
 *     d_l = x[i][l] - y[j][l]                                          l = 0 .. D - 1
 *     z_k = W[k][0] * d_0;  z_k = z_k + W[k][l] * d_l  for l = 1 .. k   k = 0 .. D - 1
 *     s_0 = z_0 * z_0;  s_k = s_(k-1) + z_k * z_k;  c = s_(D-1)
 * on everything widened to double (exact): D^2 + 3 D - 1 separately rounded IEEE double operations in this order, nothing
 * fused or reassociated (sslap_amd.points_to_dense(whiten=) is the definition; csrc/kernels_points_whiten.hpp).  Only the
 * elements W[b][i][k][l] with l <= k < D and i < n_b are ever read: the upper triangle and the rows beyond the shape may
 * hold anything.  With a covariance S_i = L L^T (Cholesky) and W_i = L^-1 the cost is the Mahalanobis distance
 * d^T S_i^-1 d, and outside / limit are in its units: the chi-square gate.  A cost is a sum of squares, never negative
 * and never -0.0, so a problem with status 0 is bit for bit the dense call on the float64 stack of these costs, as for the
 * plain call.  A cost is not finite iff an intermediate of the chain is not finite -- a NaN or an infinite coordinate or
 * matrix element that is read, an overflow, or, from finite inputs, two products that overflow to +inf and -inf, whose
 * sum is a NaN --: MISSLAP_BATCH_STATUS_INFINITE_VALUE for the solve, a candidate stored as +inf for the builder.
 * D is 1 .. MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS (a row's triangle is held in registers); a larger D, w == NULL (the
 * plain entry points are the calls without a matrix), a negative stride or a host w that is not compact are
 * MISSLAP_ERR_INVALID before a device is touched.  misslap_points_batch_reverse_finish takes no matrix: the list route
 * (the whitened candidates, then misslap_solve_ell_batch_outside and misslap_ell_batch_reverse_finish) has a finish. */
#define MISSLAP_POINTS_BATCH_MAX_WHITEN_COORDS 4
int misslap_solve_points_batch_whitened(int64_t B, int64_t N, int64_t M, int64_t D,
                                        const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                        const void *y, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                                        const void *w, int64_t w_stride_b, int64_t w_stride_n, int64_t w_stride_k,
                                        int64_t w_stride_l, const int32_t *shapes, int32_t fast, const double *prices_in,
                                        const misslap_options *opt, void *stream, void *workspace, int64_t workspace_bytes,
                                        const double *outside, int64_t outside_ld, int32_t *sol, double *prices_out,
                                        double *outside_prices_out, int32_t out_on_device, int32_t *status,
                                        int32_t *matching_size, misslap_dense_batch_meta *meta,
                                        misslap_dense_batch_info *info);
int misslap_points_batch_candidates_whitened(int64_t B, int64_t N, int64_t M, int64_t D,
                                             const void *x, int64_t x_stride_b, int64_t x_stride_n, int64_t x_stride_d,
                                             const void *y, int64_t y_stride_b, int64_t y_stride_m, int64_t y_stride_d,
                                             const void *w, int64_t w_stride_b, int64_t w_stride_n, int64_t w_stride_k,
                                             int64_t w_stride_l, int64_t K, const int32_t *shapes, const double *limit,
                                             int64_t limit_ld, const misslap_options *opt, void *stream, int32_t *cols,
                                             double *vals, int32_t *counts, int32_t *rows);

/* ---- the batch from two box sets: IoU and generalised-IoU costs, the cost stack never stored.
 * misslap_solve_boxes_batch is misslap_solve_points_batch and misslap_boxes_batch_candidates is
 * misslap_points_batch_candidates, each on box sets -- point sets of exactly 4 coordinates (x1, y1, x2, y2), so there
 * is no D -- with `metric` behind the b strides; every other argument, output, mode and the workspace
 * (misslap_points_batch_workspace_bytes: the layout is the same) is that call's.  a holds B sets of N boxes and b B sets
 * of M boxes, MISSLAP_DTYPE_F64 or MISSLAP_DTYPE_F32 (opt->mat_dtype): coordinate k of box i of problem b lies at
 * a[b * a_stride_b + i * a_stride_n + k * a_stride_d], strides in elements and >= 0, the last element's offset within
 * 62 bits; a host array is compact, strides (N * 4, 4, 1) and (M * 4, 4, 1).  The cost of (row box a, column box b), on
 * the coordinates widened to double (exact), every operation a separately rounded IEEE double operation in this order,
 * nothing fused (sslap_amd.boxes_to_dense is the definition; csrc/kernels_boxes_batch.hpp):
 *     per box   w = x2 - x1,  h = y2 - y1,  area = w * h
 *     per pair  iw = min(ax2, bx2) - max(ax1, bx1);  iw = iw > 0 ? iw : 0      (ih likewise, from the y's)
 *               inter = iw * ih;  s = area_a + area_b;  u = s - inter;  iou = u > 0 ? inter / u : 0
 *     MISSLAP_BOXES_METRIC_IOU    c = 1 - iou
 *     MISSLAP_BOXES_METRIC_GIOU   cw = max(ax2, bx2) - min(ax1, bx1)  (ch likewise);  hull = cw * ch
 *                                 e = hull - u;  e = e > 0 ? e : 0;  r = hull > 0 ? e / hull : 0;  c = 1 - (iou - r)
 * A cost lies in [0, 1] (IOU) or [0, 2] (GIOU) and is never -0.0, so every finite cost is an entry and a problem with
 * status 0 is bit for bit the dense call on the float64 stack of these costs, as for the points call.  outside / limit
 * are costs: 1 - t gates at IoU >= t.
 * The verdicts of a problem, in their order: MISSLAP_BATCH_STATUS_BAD_SHAPE, with outside
 * MISSLAP_BATCH_STATUS_BAD_OUTSIDE, MISSLAP_BATCH_STATUS_INFINITE_VALUE (a NaN or an infinite coordinate inside the
 * shape, classified on its bits before it is used; an intermediate of the chain that is infinite -- a width, an area,
 * iw or ih before the clamp, s or a hull of float64 boxes; float32 boxes cannot overflow --; or an outside value of
 * +inf), MISSLAP_BATCH_STATUS_BAD_BOX (a box inside the shape with x2 < x1 or y2 < y1; zero width or height is legal),
 * without outside MISSLAP_BATCH_STATUS_INFEASIBLE (n_b > m_b), MISSLAP_BATCH_STATUS_PRICE_NOT_FINITE,
 * MISSLAP_BATCH_STATUS_PRICE_NEGATIVE.  The builder has no status: a pair with a bad box, a NaN or infinite coordinate
 * or an infinite intermediate is always a candidate, sorts first and is stored as +inf, so misslap_solve_ell_batch on
 * the lists reports MISSLAP_BATCH_STATUS_INFINITE_VALUE for its problem: MISSLAP_BATCH_STATUS_BAD_BOX surfaces as 3 on
 * the list route.
 * These costs lie in [0, 2].  fast != 0 means eps = 1 / n_b and a guarantee of n_b * eps = 1 in total, which is coarse on
 * this scale: a tracker should leave fast 0 and set opt->eps_start (any 0 < eps_start <= 1 / n_b is still one phase,
 * optimal within n_b * eps_start); rounds grow as C / eps.
 * An unknown metric, a null a / b / sol / status, a negative stride, a stride extent beyond 62 bits, N or M outside
 * 1 .. MISSLAP_POINTS_BATCH_MAX_DIM or K outside 1 .. MISSLAP_POINTS_CANDIDATES_MAX_K are MISSLAP_ERR_INVALID before a
 * device is touched.  There is no boxes reverse finish: the list route (the candidates, then
 * misslap_solve_ell_batch_outside and misslap_ell_batch_reverse_finish) has one. */
#define MISSLAP_BOXES_METRIC_IOU 1
#define MISSLAP_BOXES_METRIC_GIOU 2
int misslap_solve_boxes_batch(int64_t B, int64_t N, int64_t M,
                              const void *a, int64_t a_stride_b, int64_t a_stride_n, int64_t a_stride_d,
                              const void *b, int64_t b_stride_b, int64_t b_stride_m, int64_t b_stride_d,
                              int32_t metric, const int32_t *shapes, int32_t fast, const double *prices_in,
                              const misslap_options *opt, void *stream, void *workspace, int64_t workspace_bytes,
                              const double *outside, int64_t outside_ld, int32_t *sol, double *prices_out,
                              double *outside_prices_out, int32_t out_on_device, int32_t *status,
                              int32_t *matching_size, misslap_dense_batch_meta *meta, misslap_dense_batch_info *info);
int misslap_boxes_batch_candidates(int64_t B, int64_t N, int64_t M,
                                   const void *a, int64_t a_stride_b, int64_t a_stride_n, int64_t a_stride_d,
                                   const void *b, int64_t b_stride_b, int64_t b_stride_m, int64_t b_stride_d,
                                   int32_t metric, int64_t K, const int32_t *shapes, const double *limit,
                                   int64_t limit_ld, const misslap_options *opt, void *stream, int32_t *cols,
                                   double *vals, int32_t *counts, int32_t *rows);

/* ---- the matching of many small graphs in one call: the batch form of misslap_hopcroft_karp / sslap.hopcroft_solve
 * (feasibility_.pyx:227-283).  Each graph is matched by ONE workgroup of ONE launch, its state in LDS
 * (csrc/kernels_matching_batch.hpp), and its result is exactly the reference's HopcroftKarpSolverCython.solve() on that
 * graph (:95-225): the same size, Pair_U and Pair_V, not merely a maximum matching.  Graphs have at most
 * MISSLAP_MATCHING_BATCH_MAX_DIM rows and columns (larger ones: misslap_hopcroft_karp / misslap_matching_gpu).
 *   misslap_matching_batch        loc is int32[nnz][2]; graph b is the entries offsets[b] .. offsets[b + 1] (offsets:
 *                                 host int64[B + 1], offsets[0] = 0, non-decreasing), rows ascending, read in stored
 *                                 order; n_b = max row + 1, m_b = max column + 1 of the graph (:245-246), and a row
 *                                 without entries is an isolated vertex.  A graph holds at most 2^31 - 129 entries.
 *   misslap_matching_dense_batch  mat is double[B][N][M] (problem stride N * M, counted in 64 bits); graph b is
 *                                 mat[b][:n_b][:m_b] with (n_b, m_b) = shapes[2b], shapes[2b + 1] (shapes NULL: N x M),
 *                                 entry (i, j) iff mat[b][i][j] >= 0 (:256-262; NaN is not an entry, -0.0 and +inf are).
 *                                 The element type of mat is opt->mat_dtype, as for misslap_solve_dense_batch (the
 *                                 parameter keeps its declared type; the pairings are those of the widened stack).
 *                                 With MISSLAP_DENSE_ENTRIES_FINITE OR-ed into opt->mat_dtype: entry (i, j) iff
 *                                 mat[b][i][j] is not a NaN (negative values and both infinities are entries).
 *   opt            device, input_on_device (loc / mat are device pointers) and input_stream, as for the batch solves;
 *                  mat_dtype for misslap_matching_dense_batch; maximize, eps_start and max_iter are ignored, every
 *                  other field must be 0.
 *   size, n_rows, n_cols   host int32[B]: the cardinality and the graph's dimensions.
 *   left_pairings  int32[B][left_ld] or NULL: Pair_U of graph b in [:n_b], -1 beyond (and for a free row).
 *   right_pairings int32[B][right_ld] or NULL: Pair_V of graph b in [:m_b], -1 beyond.
 *   out_on_device  != 0: the pairings are device pointers.
 *   info           may be NULL; info->struct_size set to sizeof(misslap_matching_batch_info).
 * All or nothing: every graph is checked before any is matched.  The first failing graph gives MISSLAP_ERR_INVALID and
 * the text "graph <b>: <what>", <what> one of "no entries", misslap_hopcroft_karp's own texts ("loc entry k = (i, j)
 * outside n x m" with k counted in the graph, "loc rows must be sorted in ascending order"), "n x m exceeds
 * MISSLAP_MATCHING_BATCH_MAX_DIM (2048)", a shape outside the stack, or dimensions that do not fit the leading
 * dimensions. */
#define MISSLAP_MATCHING_BATCH_MAX_DIM 2048
typedef struct misslap_matching_batch_info {
    int32_t struct_size;  /* IN: sizeof(misslap_matching_batch_info) */
    int32_t threads;      /* workgroup size of the matching launch */
    int32_t lds_bytes;    /* dynamic LDS per workgroup */
    int32_t reserved;
    double check_ms;      /* upload + argument checks (wall) */
    double kernel_ms;     /* the matching launch (HIP events) */
    double wall_ms;       /* the whole call */
} misslap_matching_batch_info;
int misslap_matching_batch(int64_t B, const int32_t *loc, const int64_t *offsets, const misslap_options *opt,
                           int32_t *size, int32_t *n_rows, int32_t *n_cols, int32_t *left_pairings, int64_t left_ld,
                           int32_t *right_pairings, int64_t right_ld, int32_t out_on_device,
                           misslap_matching_batch_info *info);
int misslap_matching_dense_batch(int64_t B, int64_t N, int64_t M, const double *mat, const int32_t *shapes,
                                 const misslap_options *opt, int32_t *size, int32_t *n_rows, int32_t *n_cols,
                                 int32_t *left_pairings, int64_t left_ld, int32_t *right_pairings, int64_t right_ld,
                                 int32_t out_on_device, misslap_matching_batch_info *info);
/* misslap_matching_dense_batch on a strided stack: entry (i, j) of graph b is mat[b * stride_b + i * stride_n +
 * j * stride_m], strides in elements of opt->mat_dtype under the rules of misslap_solve_dense_batch_status_strided
 * (>= 0, the extent within 62 bits, mat a device pointer with opt->input_on_device set).  Everything else, the pairings
 * included, is misslap_matching_dense_batch on a compact copy of the view. */
int misslap_matching_dense_batch_strided(int64_t B, int64_t N, int64_t M, int64_t stride_b, int64_t stride_n,
                                         int64_t stride_m, const void *mat, const int32_t *shapes,
                                         const misslap_options *opt, int32_t *size, int32_t *n_rows, int32_t *n_cols,
                                         int32_t *left_pairings, int64_t left_ld, int32_t *right_pairings,
                                         int64_t right_ld, int32_t out_on_device, misslap_matching_batch_info *info);

const char *misslap_last_error(void);
int misslap_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MISSLAP_H */
